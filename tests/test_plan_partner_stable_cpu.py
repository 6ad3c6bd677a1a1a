"""The partner-stable masks of k_persist's CARRY form, without a GPU: emx_plan_partner_stable (the host's form of the words the plan
kernel writes behind the keep masks, csrc/emx_kernels.hpp plan_partner_stable_host) against the arranged plans of the step and of the
step before (emx_plan_arrange).

Slot s of an arranged split 0 of step t reads the row of its partner p0[s], a walker of split 1 of step t.  Where that walker was in
split 0 of step t - 1 nobody writes its row during the second half of step t - 1, so the kernel asks for it a half-step early; the
mask says where.  Split 0 of step t - 1 is the first half of that step's `order`, however it is listed."""
import numpy as np
import pytest

from emcee_amd import _lib

A = 2.0
SEED = 0x5EED5
SIZES = (32, 512, 2080)
STEPS = (1, 2, 3, 4)


def arranged(step, N):
    lib = _lib.load()
    order, p0 = np.full(N, -1, dtype=np.int32), np.full(N, -1, dtype=np.int32)
    s0, uacc = np.full(N, np.nan), np.full(N, np.nan)
    mask = np.full((N // 2 + 15) // 16, -1, dtype=np.int32)
    assert lib.emx_plan_arrange(SEED, step, 1 if step else 0, N, A, order.ctypes.data, p0.ctypes.data, s0.ctypes.data, uacc.ctypes.data,
                                mask.ctypes.data) == 0
    return dict(order=order, p0=p0)


def stable_words(step, N, seed=SEED):
    mask = np.full((N // 2 + 15) // 16, -1, dtype=np.int32)
    assert _lib.load().emx_plan_partner_stable(seed, step, N, A, mask.ctypes.data) == 0
    return mask


def bits_of(mask, n0):
    s = np.arange(n0)
    return ((mask[s >> 4] >> (s & 15)) & 1).astype(bool)


@pytest.mark.parametrize("N", SIZES)
def test_bit_set_exactly_where_the_partner_was_in_split_0_of_the_step_before(N):
    n0 = N // 2
    for step in STEPS:
        cur, prev = arranged(step, N), arranged(step - 1, N)
        in_prev0 = np.zeros(N, dtype=bool)
        in_prev0[prev["order"][:n0]] = True
        words = stable_words(step, N)
        assert len(words) == (n0 + 15) // 16
        assert np.array_equal(bits_of(words, n0), in_prev0[cur["p0"][:n0]]), step
        # a partner of split 0 is a walker of split 1
        assert not np.isin(cur["p0"][:n0], cur["order"][:n0]).any()
        # nothing beyond the split's slots, nothing beyond a tile's sixteen bits
        assert not (words >> 16).any()
        if n0 % 16:
            assert not (words[-1] >> (n0 % 16))


def test_about_half_of_the_partners_are_stable():
    """2 080 walkers: 1 040 partners, each in split 0 of the step before with probability about a half (the splits of two steps are
    independent): 520 +- 6 sigma (sigma = sqrt(1 040) / 2 = 16.1) is 0.407 ... 0.593 of them."""
    N, n0 = 2080, 1040
    for step in STEPS:
        frac = bits_of(stable_words(step, N), n0).mean()
        assert 0.4 <= frac <= 0.6, (step, frac)


def test_last_word_is_clear_beyond_the_split():
    for N in (34, 2082):           # 17 and 1 041 slots: one slot in the last tile
        n0 = N // 2
        for step in STEPS:
            words = stable_words(step, N)
            assert len(words) == (n0 + 15) // 16 and not (words[-1] >> (n0 % 16)) and not (words >> 16).any()
    for step in STEPS:
        assert not (stable_words(step, 2080)[-1] >> 16)


def test_bad_arguments_are_refused():
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.int32)
    p = buf.ctypes.data
    assert lib.emx_plan_partner_stable(1, 1, 33, A, p) == -1          # odd
    assert lib.emx_plan_partner_stable(1, 1, 0, A, p) == -1
    assert lib.emx_plan_partner_stable(1, 0, 32, A, p) == -1          # no step before step 0
    assert lib.emx_plan_partner_stable(1, 1, 32, A, None) == -1
    assert lib.emx_plan_partner_stable(1, 1, 32, A, p) == 0


def test_header_table_and_tuning_key_agree():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "emx.h")).read()
    m = re.search(r"int\s+emx_plan_partner_stable\s*\(([^)]*)\)", txt)
    assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES["emx_plan_partner_stable"][1]) == 5
    assert '"persist_partner_prefetch"' in txt and "emx_persist_pprefetch_launches" in _lib.SIGNATURES
