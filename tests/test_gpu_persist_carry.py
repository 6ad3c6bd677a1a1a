"""k_persist's CARRY form (csrc/emx_kernels.hpp; tuning "persist_carry", include/emx.h emx_persist_carry_launches): device-wide
stretch launches that store no rows run over Philox plans whose split 0 is arranged after the step before (emx_plan_arrange), keep
the rows of the walkers that stay in a wave's slots over the step boundary in registers and prefetch the others.  A listing order
changes no draw and a kept row is the row the wave wrote itself, so every bit must be that of the launch-per-half-step kernels and
of the form without it."""
import numpy as np
import pytest

from emcee_amd import _lib
from emcee_amd.device import EmxError
from oracle import sampler_oracle as so

from test_gpu_full_size import full_spec
from test_gpu_parity import make_ens

pytestmark = pytest.mark.gpu

S = so.MoveSpec
SEED = 0x5EED5
CALLS = (13, 19, 13)        # 45 steps: launches begin inside a plan batch of sixteen steps and cross batch and launch boundaries
# 512 x 64: sixteen tiles a split, the smallest device-wide grid; 1 024 x 16: one 16-column block (DPB = 1); 2 080 x 64: 65 tiles, one
# wave a workgroup; 8 192 x 62: padded ndim
SHAPES = [(512, 64), (1024, 16), (2080, 64), (8192, 62)]
# The acceptance of the last step on the launch-per-half-step path: below 2 %, about a quarter, above 90 %.  The knob is the stretch
# move's scale `a`, not the target's: with a = 2 no target scale leaves that range's ends within reach at these ndim -- a flat target
# accepts every z > 1 and, by the factor z^(ndim - 1), next to no z < 1 (59 %), a narrow one makes the ensemble contract (41 %) --
# while a large `a` proposes far out of an ensemble in equilibrium and a = 1.001 hardly moves a walker.  (The window of z that is
# accepted at all narrows with ndim: at ndim 16 the same regimes need a wider move.)
# "about a quarter" is 0.15 ... 0.35.  With a = 2 the ndim 62 / 64 shapes reach 0.16 - 0.19 (measured: 512 x 64 0.1875, 2 080 x 64 0.1707,
# 8 192 x 62 0.1597), so they take a = 1.6, whose window of accepted z is 1.5 times as likely, and reach 0.2578 (512 x 64), 0.2428
# (2 080 x 64) and 0.2393 (8 192 x 62) with it; 1 024 x 16 reaches 0.2324 with a = 3.  The other regimes: 0.0098 / 0.0146 / 0.0168 /
# 0.0161 and 0.9980 / 0.9990 / 0.9986 / 0.9972 in the order of SHAPES.
REGIMES = {"rare": ({16: 400.0}, 50.0, 0.0, 0.02), "quarter": ({16: 3.0}, 1.6, 0.15, 0.35), "mostly": ({}, 1.001, 0.90, 1.0)}


def spec_of(N, D, a, seed=3):
    return full_spec(N, D, "dense", [S("stretch", a=a)], seed=seed)


def ens_of(spec, persist, carry, step=0):
    ens = make_ens(spec, spec["p0"])
    ens.set_rng_mode(_lib.RNG_PHILOX)
    ens.set_philox(SEED, step)
    ens.set_tuning("persist", persist)
    ens.set_tuning("persist_local", 0)           # the device-wide form at every size
    ens.set_tuning("persist_carry", carry)
    ens.set_tuning("persist_timeout_ms", 100)
    return ens


def result(ens):
    assert ens.status() == 0
    x, lp = ens.get_state()
    return dict(x=x, lp=lp, acc=ens.accepted_mask(), info=ens.persist_info())


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("N,D", SHAPES)
def test_carried_rows_change_no_bit(N, D, regime):
    by_ndim, a, lo, hi = REGIMES[regime]
    a = by_ndim.get(D, a)
    spec = spec_of(N, D, a)
    recs = {}
    for name, persist, carry in (("carry", 1, 1), ("reload", 1, 0), ("launches", 0, 1)):
        ens = ens_of(spec, persist, carry)
        naccepted = np.zeros(N, dtype=np.int64)
        for n in CALLS:
            ens.run(n, 1, False)
            naccepted += ens.accepted_mask().astype(np.int64)      # (the accept marks of every call's last step)
        recs[name] = result(ens)
        recs[name]["naccepted"] = naccepted
        ens.close()
    frac = recs["launches"]["acc"].mean()
    print("%d x %d, a = %g: acceptance of the last step %.4f" % (N, D, a, frac))
    assert lo <= frac <= hi, frac
    ic, ir, il = (recs[k]["info"] for k in ("carry", "reload", "launches"))
    assert ic["qualifies"] and ic["launches"] == len(CALLS) and ic["halfsteps"] == 2 * sum(CALLS) and ic["recovered"] == 0
    assert ic["carry_launches"] == ic["launches"] and ic["local_launches"] == 0
    assert ir["launches"] == len(CALLS) and ir["carry_launches"] == 0 and ir["local_launches"] == 0
    assert il["launches"] == 0 and il["carry_launches"] == 0
    for key in ("x", "lp", "acc", "naccepted"):
        assert np.array_equal(recs["carry"][key], recs["launches"][key]), "CARRY against the launches: " + key
        assert np.array_equal(recs["carry"][key], recs["reload"][key]), "CARRY against persist_carry = 0: " + key


def ring_slots(ens, N):
    import torch
    from emcee_amd.parallel import _DevView
    out = []
    for r in range(1024):                       # (the ring's slots are the ids the library knows from 16 on)
        try:
            ptr, nbytes = ens.device_ptr(16 + r)
        except EmxError:
            break
        if not ptr or nbytes != 48 * N:
            continue
        raw = torch.as_tensor(_DevView(ptr, nbytes // 8), device=torch.device("cuda", 0)).view(torch.int64).cpu().numpy()
        b = raw.view(np.uint8)
        out.append(dict(order=b[:4 * N].view(np.int32), p0=b[4 * N:8 * N].view(np.int32), s0=b[8 * N:16 * N].view(np.float64),
                        p1=b[24 * N:28 * N].view(np.int32)))
    return out


def host_arranged(seed, step, has_prev, N, a=2.0):
    lib = _lib.load()
    order, p0 = np.empty(N, dtype=np.int32), np.empty(N, dtype=np.int32)
    s0, uacc = np.empty(N), np.empty(N)
    mask = np.empty((N // 2 + 15) // 16, dtype=np.int32)
    assert lib.emx_plan_arrange(seed, step, has_prev, N, a, order.ctypes.data, p0.ctypes.data, s0.ctypes.data, uacc.ctypes.data, mask.ctypes.data) == 0
    return dict(order=order, p0=p0, s0=s0, mask=mask)


@pytest.mark.parametrize("N,D", [(512, 64), (2080, 64), (8192, 62)])
def test_device_plans_equal_the_host_form(N, D):
    """The plan ring after one step (batch 0: steps 0 ... 15, step 0 without a step before it) and after seventeen (batch 1: steps
    16 ... 31, step 16 arranged after step 15 of the batch before): every step's slot holds what emx_plan_arrange says, word for word
    -- order, p0, s0 and the keep masks in the head of the unwritten p1 column."""
    ens = ens_of(spec_of(N, D, 2.0), 1, 1)
    n0 = N // 2
    for nrun, steps in ((1, range(0, 16)), (16, range(16, 32))):
        ens.run(nrun, 1, False)
        ens.sync()
        slots = ring_slots(ens, N)
        assert len(slots) >= 32          # two batches of sixteen steps
        for step in steps:
            h = host_arranged(SEED, step, 1 if step > 0 else 0, N)
            hit = [s for s in slots if np.array_equal(s["order"][n0:], h["order"][n0:])]
            assert len(hit) == 1, step
            d = hit[0]
            assert np.array_equal(d["order"], h["order"]), step
            assert np.array_equal(d["p0"], h["p0"]), step
            assert np.array_equal(d["s0"], h["s0"]), step
            if step > 0:
                assert np.array_equal(d["p1"][:len(h["mask"])], h["mask"]), step
                assert h["mask"].any() and not np.array_equal(h["order"], host_arranged(SEED, step, 0, N)["order"])
    assert ens.status() == 0
    ens.close()


def test_runs_interleaved_with_state_installs_and_the_step_api():
    """A launch's first half-step loads every row whatever the masks say: between the runs the state is replaced (set_state) and steps
    are taken through the step API, which reads the arranged plans like any listing of the split."""
    N, D = 2080, 64
    spec = spec_of(N, D, 2.0, seed=7)
    rs = np.random.RandomState(5)
    other = spec["p0"][rs.permutation(N)] * 0.5
    ens, ref = ens_of(spec, 1, 1), ens_of(spec, 0, 1)
    for e in (ens, ref):
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
    a, b = result(ens), result(ref)
    assert a["info"]["carry_launches"] == a["info"]["launches"] >= 5 and b["info"]["launches"] == 0
    for key in ("x", "lp", "acc"):
        assert np.array_equal(a[key], b[key]), key
    ens.close()
    ref.close()


def test_the_tuning_key_is_checked_when_it_is_set():
    ens = ens_of(spec_of(512, 64, 2.0), 1, 1)
    for bad in (2, -1):
        with pytest.raises(EmxError):
            ens.set_tuning("persist_carry", bad)
    ens.set_tuning("persist_carry", 0)
    ens.run(4, 1, False)
    assert ens.persist_info()["launches"] == 1 and ens.persist_info()["carry_launches"] == 0
    ens.close()
