"""The arranged stretch plans of k_persist's CARRY form, without a GPU: emx_plan_arrange (the host's form of what k_plan_arrange and
k_native_plan_batch_stretch write, csrc/emx_kernels.hpp plan_arrange_host) against the position-ordered plans of the step and of the
step before (emx_host_plan_philox).

A stretch step of two splits lists split 0 after the step before: slot s holds the walker of that step's split-1 slot s where the
walker belongs to this step's split 0 (a keep slot: the wave that ran it still holds its row); the other slots hold walkers that were
in split 0 before, which nobody writes meanwhile.  The listing changes no draw: every slot's entry is the walker's own."""
import ctypes as C

import numpy as np
import pytest

from emcee_amd import _lib
from emx_testlib import philox_plan

A = 2.0
SIZES = (32, 512, 4096, 65536)
SEEDS = (1, 0xDEADBEEF12345, 2 ** 63 + 12345)
# (step before, step): small, mid-run, and the carries of the step counter's low word
STEPS = (1, 2, 17, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 3)


def arranged(seed, step, has_prev, N):
    lib = _lib.load()
    order, p0 = np.full(N, -1, dtype=np.int32), np.full(N, -1, dtype=np.int32)
    s0, uacc = np.full(N, np.nan), np.full(N, np.nan)
    mask = np.full((N // 2 + 15) // 16, -1, dtype=np.int32)
    rc = lib.emx_plan_arrange(seed, step, has_prev, N, A, order.ctypes.data, p0.ctypes.data, s0.ctypes.data, uacc.ctypes.data, mask.ctypes.data)
    assert rc == 0
    return dict(order=order, p0=p0, s0=s0, uacc=uacc, mask=mask)


def keep_bits(mask, n0):
    s = np.arange(n0)
    return ((mask[s >> 4] >> (s & 15)) & 1).astype(bool)


_PLANS = {}


def plain(seed, step, N):
    key = (seed, step, N)
    if key not in _PLANS:
        md = _lib.MoveDesc(_lib.MOVE_STRETCH, 2, 0, 0, A, 0.0, 0.0, 0.0)
        p = philox_plan(seed, step, N, md)
        for v in p.values():
            v.setflags(write=False)
        _PLANS[key] = p
    return _PLANS[key]


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("seed", SEEDS)
def test_arranged_split_is_the_same_split_in_carry_order(N, seed):
    n0 = N // 2
    for step in STEPS if N <= 4096 else STEPS[:1] + STEPS[3:5]:
        cur, prev = plain(seed, step, N), plain(seed, step - 1, N)
        assert list(cur["off"]) == [0, n0, N]
        arr = arranged(seed, step, 1, N)
        # a permutation of the position-ordered split 0; split 1 untouched
        assert np.array_equal(np.sort(arr["order"][:n0]), np.sort(cur["order"][:n0]))
        for k in ("order", "p0", "s0", "uacc"):
            assert np.array_equal(arr[k][n0:], cur[k][n0:]), k
        keep = keep_bits(arr["mask"], n0)
        assert not (arr["mask"] >> 16).any()
        if n0 % 16:
            assert not (arr["mask"][-1] >> (n0 % 16))
        # keep slot s: the walker of the step before's split-1 slot s, exactly where that walker is in this step's split 0
        prev1 = prev["order"][n0:]
        in_cur0 = np.zeros(N, dtype=bool)
        in_cur0[cur["order"][:n0]] = True
        assert np.array_equal(keep, in_cur0[prev1])
        assert np.array_equal(arr["order"][:n0][keep], prev1[keep])
        # the others: in split 0 of the step before, ascending in this step's positions
        in_prev0 = np.zeros(N, dtype=bool)
        in_prev0[prev["order"][:n0]] = True
        fill = arr["order"][:n0][~keep]
        assert in_prev0[fill].all()
        pos_of = np.empty(N, dtype=np.int64)
        pos_of[cur["order"]] = np.arange(N)
        assert (np.diff(pos_of[fill]) > 0).all()
        # every slot's entry is the walker's own
        src = pos_of[arr["order"][:n0]]
        for k in ("p0", "s0", "uacc"):
            assert np.array_equal(arr[k][:n0], cur[k][src]), k
        # about half of a split stays (the two splits are independent): the form has something to carry
        assert 0.3 * n0 <= keep.sum() <= 0.7 * n0 or N <= 32


@pytest.mark.parametrize("N", SIZES)
def test_a_step_without_a_predecessor_is_in_position_order(N):
    for seed, step in ((SEEDS[0], 0), (SEEDS[1], 5), (SEEDS[2], 2 ** 32)):
        cur = plain(seed, step, N)
        arr = arranged(seed, step, 0, N)
        for k in ("order", "p0", "s0", "uacc"):
            assert np.array_equal(arr[k], cur[k]), k
        assert not arr["mask"].any()


def test_bad_arguments_are_refused():
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data
    assert lib.emx_plan_arrange(1, 1, 1, 33, A, p, p, p, p, p) == -1          # odd
    assert lib.emx_plan_arrange(1, 1, 1, 0, A, p, p, p, p, p) == -1
    assert lib.emx_plan_arrange(1, 0, 1, 32, A, p, p, p, p, p) == -1          # no step before step 0
    assert lib.emx_plan_arrange(1, 1, 1, 32, A, None, p, p, p, p) == -1


def test_header_table_and_tuning_key_agree():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "emx.h")).read()
    m = re.search(r"int\s+emx_plan_arrange\s*\(([^)]*)\)", txt)
    assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES["emx_plan_arrange"][1]) == 10
    assert '"persist_carry"' in txt and "emx_persist_carry_launches" in _lib.SIGNATURES
