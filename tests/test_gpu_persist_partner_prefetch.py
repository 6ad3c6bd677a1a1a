"""The partner prefetch of k_persist's CARRY form (csrc/emx_kernels.hpp; tuning "persist_partner_prefetch", include/emx.h
emx_persist_pprefetch_launches): in the second half of a step a wave asks for the partner rows of the NEXT step's first half-step that
nobody writes meanwhile -- the partners that were in split 0 of this step (emx_plan_partner_stable: one mask word a tile, written by
the plan kernel behind the keep masks) -- and loads only the others behind the barrier.  A prefetched row is the row a load behind the
barrier would have returned, so every bit must be that of the form without it and of the launch-per-half-step kernels."""
import numpy as np
import pytest

from emcee_amd import _lib
from emcee_amd.device import EmxError

from test_gpu_persist_carry import SEED, ens_of, host_arranged, result, ring_slots, spec_of

pytestmark = pytest.mark.gpu

# 512 x 64: sixteen tiles a split, the smallest device-wide grid; 2 080 x 64: 65 tiles, one wave a workgroup; 8 192 x 62: padded ndim;
# 1 024 x 16 / 32 / 48: one, two and three 16-column blocks (DPB 1 ... 3; the others are DPB 4)
SHAPES = [(512, 64), (2080, 64), (8192, 62), (1024, 16), (1024, 32), (1024, 48)]
CALLS = (1, 16, 17, 20, 3)      # 57 steps: launches of one step, launches that begin inside a plan batch of sixteen steps and span a batch boundary
# the stretch scale by ndim: an acceptance of about a quarter at ndim 62 / 64 and 16 (tests/test_gpu_persist_carry.py REGIMES)
SCALE = {16: 3.0, 32: 2.0, 48: 2.0}


def ens_ppf(spec, persist, ppf):
    ens = ens_of(spec, persist, 1)
    ens.set_tuning("persist_partner_prefetch", ppf)
    return ens


def host_stable(seed, step, N, a=2.0):
    mask = np.empty((N // 2 + 15) // 16, dtype=np.int32)
    assert _lib.load().emx_plan_partner_stable(seed, step, N, a, mask.ctypes.data) == 0
    return mask


@pytest.mark.parametrize("N,D", [(512, 64), (2080, 64), (8192, 62)])
def test_device_masks_equal_the_host_form(N, D):
    """The plan ring after one step (batch 0: steps 0 ... 15) and after seventeen (batch 1: steps 16 ... 31, step 16 after step 15 of
    the batch before): behind the keep masks of every arranged step, words ntiles ... 2 ntiles of the p1 column, the partner-stable
    masks emx_plan_partner_stable gives; the keep masks themselves are emx_plan_arrange's as before.
    (A seed of this test's own: the ring's slots are found by their contents, and the half of the ring that no batch has filled yet is
    whatever the allocator hands out -- after a test with the same seed and size, that test's plans.)"""
    seed = SEED + 0x9E3779B1 * N
    ens = ens_ppf(spec_of(N, D, 2.0), 1, 1)
    ens.set_philox(seed, 0)
    n0 = N // 2
    nt = (n0 + 15) // 16
    for nrun, steps in ((1, range(1, 16)), (16, range(16, 32))):
        ens.run(nrun, 1, False)
        ens.sync()
        slots = ring_slots(ens, N)
        assert len(slots) >= 32
        for step in steps:
            h = host_arranged(seed, step, 1, N)
            hit = [s for s in slots if np.array_equal(s["order"], h["order"])]
            assert len(hit) == 1, step
            p1 = hit[0]["p1"]
            assert np.array_equal(p1[:nt], h["mask"]), step
            st = host_stable(seed, step, N)
            assert np.array_equal(p1[nt:2 * nt], st), step
            assert st.any() and not (st >> 16).any()
    assert ens.status() == 0
    ens.close()


@pytest.mark.parametrize("N,D", SHAPES)
def test_prefetched_partner_rows_change_no_bit(N, D):
    spec = spec_of(N, D, SCALE.get(D, 1.6))
    recs = {}
    for name, persist, ppf in (("prefetch", 1, 1), ("behind", 1, 0), ("launches", 0, 1)):
        ens = ens_ppf(spec, persist, ppf)
        naccepted = np.zeros(N, dtype=np.int64)
        for n in CALLS:
            ens.run(n, 1, False)
            naccepted += ens.accepted_mask().astype(np.int64)      # (the accept marks of every call's last step)
        recs[name] = result(ens)           # (asserts status 0)
        recs[name]["naccepted"] = naccepted
        ens.close()
    frac = recs["launches"]["acc"].mean()
    print("%d x %d: acceptance of the last step %.4f" % (N, D, frac))
    assert 0.02 < frac < 0.98, frac             # accepted and rejected proposals both: rows that moved and rows that did not
    ip, ib, il = (recs[k]["info"] for k in ("prefetch", "behind", "launches"))
    assert ip["qualifies"] and ip["launches"] == len(CALLS) and ip["halfsteps"] == 2 * sum(CALLS) and ip["recovered"] == 0
    assert ip["pprefetch_launches"] == ip["carry_launches"] == ip["launches"] and ip["local_launches"] == 0
    assert ib["carry_launches"] == ib["launches"] == len(CALLS) and ib["pprefetch_launches"] == 0
    assert il["launches"] == 0 and il["pprefetch_launches"] == 0
    for key in ("x", "lp", "acc", "naccepted"):
        assert np.array_equal(recs["prefetch"][key], recs["behind"][key]), "prefetch against persist_partner_prefetch = 0: " + key
        assert np.array_equal(recs["prefetch"][key], recs["launches"][key]), "prefetch against the launches: " + key


def test_runs_interleaved_with_state_installs_and_the_step_api():
    """A launch's first half-step loads every partner row whatever the masks say: between the runs the state is replaced and steps are
    taken through the step API, whose one-step plans are not arranged."""
    N, D = 2080, 64
    spec = spec_of(N, D, 2.0, seed=7)
    rs = np.random.RandomState(5)
    other = spec["p0"][rs.permutation(N)] * 0.5
    trio = [ens_ppf(spec, 1, 1), ens_ppf(spec, 1, 0), ens_ppf(spec, 0, 1)]
    for e in trio:
        e.run(5, 1, False)
        e.set_state(other)
        e.eval_state_log_prob()
        e.run(14, 1, False)
        for _ in range(3):
            k, nsplit = e.step_begin(store=False)
            for s in range(nsplit):
                e.halfstep(s)
            e.step_end()
        e.run(9, 1, False)
        x, lp = e.get_state()
        e.set_state(x[::-1].copy())
        e.eval_state_log_prob()
        e.run(21, 1, False)
    a, b, c = (result(e) for e in trio)
    assert a["info"]["pprefetch_launches"] == a["info"]["carry_launches"] == a["info"]["launches"] >= 5
    assert b["info"]["carry_launches"] == b["info"]["launches"] >= 5 and b["info"]["pprefetch_launches"] == 0
    assert c["info"]["launches"] == 0
    for key in ("x", "lp", "acc"):
        assert np.array_equal(a[key], b[key]), key
        assert np.array_equal(a[key], c[key]), key
    for e in trio:
        e.close()


def test_the_tuning_key_is_checked_when_it_is_set():
    ens = ens_ppf(spec_of(512, 64, 2.0), 1, 1)
    for bad in (2, -1):
        with pytest.raises(EmxError):
            ens.set_tuning("persist_partner_prefetch", bad)
    ens.set_tuning("persist_partner_prefetch", 0)
    ens.run(4, 1, False)
    info = ens.persist_info()
    assert info["launches"] == info["carry_launches"] == 1 and info["pprefetch_launches"] == 0
    ens.set_tuning("persist_partner_prefetch", 1)
    ens.run(4, 1, False)
    info = ens.persist_info()
    assert info["launches"] == info["carry_launches"] == 2 and info["pprefetch_launches"] == 1
    ens.close()
