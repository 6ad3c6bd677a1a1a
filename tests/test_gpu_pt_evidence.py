"""PTSampler.get_evidence on the device (emx_pt_evidence, csrc/emx_pt_evidence.hip): the per-block triples and every field of
Evidence against the exact reference of tests/evidence_ref.py computed on the stored plane (get_log_likelihood / get_betas),
within the bounds its docstring derives; no bit depending on the object range; likelihoods with zero-support regions, where
thermodynamic integration has no answer; the ladder check; the fused tempered path's plane; and the sampled evidence of the
box-truncated Gaussian at 10 rungs, where the stepping-stone estimate is closer to -2 log 20 than thermodynamic integration.

Shapes (PE_SLICE = 4 096 samples a slice, 256 threads x 16 samples):
  small     G 3, T 4, N 20, 67 stored steps, K 4: N no multiple of 64, nt not divisible by K, a ladder that ends above 0
  wide      N 300 (a row wider than a workgroup), discard 3, thin 2 (the strided path), a ladder that ends at 0
  one rung  T 1, K 1
  long      N 8, 2 300 steps, K 2: a block of 9 200 samples is cut into 3 slices, the last one partly filled
  odd       N 21, T 3: members whose rows start at an odd double, so that the pairs are not 16-byte aligned"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import evidence_ref as er  # noqa: E402
from emcee_amd import PTSampler  # noqa: E402
from emcee_amd.targets import BatchCallable  # noqa: E402

pytestmark = pytest.mark.gpu

EXACT = -2.0 * np.log(20.0)


def gauss(q):
    return -0.5 * (q * q).sum(-1) - float(np.log(2 * np.pi))


def disc(radius, sd):
    def fn(q):
        r2 = (q * q).sum(-1)
        return torch.where(r2 < radius * radius, -0.5 * r2 / (sd * sd), torch.full_like(r2, -float("inf")))
    return fn


def box(D, a=10.0):
    return (-a * np.ones(D), a * np.ones(D))


def sampler(G, T, N, nsteps, Tmax, fn=gauss, seed=1, start=1.0, **kw):
    s = PTSampler(T, N, 2, BatchCallable(fn), log_prior=box(2), Tmax=Tmax, nbatch=G, seeds=[seed + g for g in range(G)], **kw)
    s.run_mcmc(np.random.RandomState(seed).uniform(-start, start, size=(G, T, N, 2)), nsteps)
    return s


def against_the_reference(s, what, **kw):
    """get_evidence(**kw) and the per-block triples against the exact reference on the stored plane -> (Evidence, reference)"""
    K = kw.get("nblocks", 8)
    sel = {k: v for k, v in kw.items() if k != "nblocks"}
    L, lad = s.get_log_likelihood(**sel), s.get_betas(**sel)
    nt = L.shape[2]
    b = lad[:, nt - K * (nt // K)]
    assert np.array_equal(lad[:, nt - K * (nt // K):], np.broadcast_to(b[:, None], lad[:, nt - K * (nt // K):].shape))
    ref = er.exact(b, L, K)
    ev = s.get_evidence(**kw)
    A, M, S, bd, changed, bl = s._evidence_blocks(**kw)
    assert bl == nt // K and not changed.any() and np.array_equal(bd, b) and np.array_equal(ev.betas, b)
    worst = dict(er.check_blocks(A, M, S, ref, what), **er.check(ev, ref, what))
    print("%s: worst err / bound %s" % (what, {k: "%.2g" % v for k, v in worst.items()}))
    return ev, ref


@pytest.fixture(scope="module")
def small():
    s = sampler(3, 4, 20, 67, None)
    yield s
    s.close()


# ---------------------------------------------------------------------------------------------------------------- the reference
def test_small_shape_against_the_exact_reference(small):
    ev, _ = against_the_reference(small, "small", nblocks=4)
    assert ev.block_length == 16 and (ev.tail != 0).all() and np.isfinite(ev.logz_ss).all()
    against_the_reference(small, "small K=1", nblocks=1, discard=5)
    against_the_reference(small, "small thin", nblocks=5, discard=2, thin=3)


@pytest.mark.parametrize("name,G,T,N,nsteps,Tmax,kw", [
    ("wide", 1, 2, 300, 24, np.inf, dict(nblocks=3, discard=3, thin=2)),
    ("one rung", 2, 1, 20, 30, None, dict(nblocks=1)),
    ("long", 1, 2, 8, 2300, np.inf, dict(nblocks=2)),
    ("odd", 2, 3, 21, 40, None, dict(nblocks=3, discard=1)),
])
def test_shapes_against_the_exact_reference(name, G, T, N, nsteps, Tmax, kw):
    s = sampler(G, T, N, nsteps, Tmax, seed=len(name))
    ev, ref = against_the_reference(s, name, **kw)
    assert (ev.tail == 0).all() == (Tmax == np.inf and T > 1)
    if name == "long":
        assert ref["n"] == 1150 * 8 > 2 * 4096
        against_the_reference(s, "long thin", nblocks=2, thin=2)
    if name == "one rung":
        assert np.array_equal(ev.logz_ss, ev.tail) and np.isnan(ev.err_ss).all()
    s.close()


# ---------------------------------------------------------------------------------------------------------------- the launch
def test_no_bit_depends_on_the_object_range_or_the_call(small):
    whole = small._evidence_blocks(nblocks=4, discard=1)
    again = small._evidence_blocks(nblocks=4, discard=1)
    assert all(np.array_equal(u, v) for u, v in zip(whole[:5], again[:5]))
    for lo, hi in ((1, 2), (0, 2), (2, 3)):
        part = small._evidence_blocks(nblocks=4, discard=1, lo=lo, hi=hi)
        assert all(np.array_equal(u[lo:hi], v) for u, v in zip(whole[:5], part[:5])) and part[5] == whole[5]


# ---------------------------------------------------------------------------------------------------------------- zero support
def test_a_likelihood_that_is_minus_infinity_on_most_of_the_prior():
    s = sampler(2, 4, 20, 300, np.inf, fn=disc(0.01, 0.005), seed=5, start=0.005)
    L = s.get_log_likelihood()
    assert s.betas[-1] == 0 and np.isneginf(L[:, -1, 225:]).all()          # the case: the beta = 0 rung's last block has no weight
    assert np.isfinite(L[:, :-1]).all()
    ev, ref = against_the_reference(s, "disc 0.01", nblocks=4)
    assert (ev.mean_logl[:, -1] == -np.inf).all() and not np.isfinite(ev.logz_ti).any()
    assert not np.isnan(ev.log_ratios).any() and not np.isnan(ev.logz_ss).any() and not np.isnan(ev.block_logz_ss).any()
    assert (ev.block_logz_ss[:, -1] == -np.inf).all()
    s.close()


def test_a_disc_of_radius_five_has_a_finite_stepping_stone_evidence():
    s = sampler(2, 4, 20, 300, np.inf, fn=disc(5.0, 1.0), seed=6)
    ev, ref = against_the_reference(s, "disc 5", nblocks=4, discard=50)
    assert np.isfinite(ev.logz_ss).all() and np.isfinite(ev.err_ss).all()
    assert (ev.mean_logl[:, -1] == -np.inf).all() and not np.isfinite(ev.logz_ti).any()
    s.close()


# ---------------------------------------------------------------------------------------------------------------- the ladder
def test_a_ladder_that_changed_is_refused_and_a_frozen_one_is_used():
    s = sampler(3, 4, 20, 40, None, seed=7, adaptive=True, adaptation_lag=20, adaptation_time=2)
    assert not np.array_equal(s.ladder, np.tile(s.betas, (3, 1)))
    with pytest.raises(ValueError, match=r"object \d.*the ladder changed.*Freeze adaptation \(adaptive = False\)"):
        s.get_evidence(nblocks=4)
    s.adaptive = False
    s.run_mcmc(None, 40)
    with pytest.raises(ValueError, match=r"object \d.*the ladder changed"):
        s.get_evidence(nblocks=4, discard=30)
    ev, _ = against_the_reference(s, "frozen", nblocks=4, discard=40)
    assert np.array_equal(ev.betas, s.ladder) and ev.block_length == 10
    s.close()


# ---------------------------------------------------------------------------------------------------------------- the fused plane
def test_the_fused_path_stores_the_same_plane(tmp_path):
    import subprocess
    import test_gpu_pt_fused as tf
    so = str(tmp_path / "libuser_pt_fused_3.so")
    r = subprocess.run(tf._compile_cmd(3, so), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    shape = G, T, N, D = 3, 4, 32, 3
    f, k, mdl = tf.pair({3: tf._load(so)}, shape, "stretch", "box", 17, swap_every=1)
    p0 = 0.8 * np.random.RandomState(18).randn(G, T, N, D)
    f.run_mcmc(p0, 30)
    k.run_mcmc(p0, 30)
    assert np.array_equal(f.get_log_likelihood(), k.get_log_likelihood())       # the existing contract
    a, b = f.get_evidence(nblocks=3, discard=3), k.get_evidence(nblocks=3, discard=3)
    assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a[:11], b[:11])) and a[11:] == b[11:] == (3, 9)
    assert np.isfinite(a.logz_ss).all()
    f.close()
    k.close()
    mdl.close()


# ---------------------------------------------------------------------------------------------------------------- the truth
def test_sampled_evidence_at_ten_rungs_beats_thermodynamic_integration():
    """tests/test_gpu_pt.py's evidence model (the 2-d unit Gaussian in the +-10 box, log Z = -2 log 20) at 10 rungs down to beta = 0,
    where it needs 40"""
    G, T, N, D, nsteps = 4, 10, 32, 2, 2000
    s = PTSampler(T, N, D, BatchCallable(gauss), log_prior=box(D), Tmax=np.inf, nbatch=G, seeds=[31, 32, 33, 34])
    s.run_mcmc(np.random.RandomState(9).uniform(-1, 1, size=(G, T, N, D)), nsteps)
    ev = s.get_evidence(discard=200)
    mc = np.std(ev.logz_ss)
    print("logz_ss", ev.logz_ss, "+-", ev.err_ss, "logz_ti", ev.logz_ti, "+-", ev.err_ti, "exact", EXACT, "std over the objects", mc)
    assert np.all(np.abs(ev.logz_ss - EXACT) < max(0.05, 4 * mc)), (ev.logz_ss, EXACT, mc)
    assert np.all(np.abs(ev.logz_ss - EXACT) < np.abs(ev.logz_ti - EXACT)), (ev.logz_ss, ev.logz_ti)
    s.close()
