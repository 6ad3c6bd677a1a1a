"""EnsembleSampler.get_summary: emx_summary (csrc/emx_summary_single.hpp) against NumPy on the host copy of the same chain
(get_chain / get_log_prob, never the code under test), with the checks of tests/test_gpu_batch_summary.py::check_against_host.

Order statistics, the MAP sample and the quantiles' interpolation are exact.  The mean and the covariance are held to
first-order worst-case bounds of ANY summation order (derived, not measured; u = 2^-53):
  |mean - fsum(x) / n|  <=  n u sum|x| / n                          (math.fsum is the exact reference)
  |cov_jk - C_jk|       <=  8 n u sqrt(C_jj C_kk),  C = np.cov      (Cauchy-Schwarz, as in test_gpu_batch_summary.py)
Rejected proposals repeat rows, so every chain here has ties.

Shapes: the smallest that reach each code path -- the explicit-fma Gram (ndim < 16), the first MFMA width (16), a padded one
(33 -> 48), both sides of the switch (15 / 17), many chunks of walkers (8 192 x 64), a chain regrown between two runs, -inf
log-probs, the exact-mode chain writer and the blob plane of a DeviceFused target."""
import math

import numpy as np
import pytest

from emcee_amd import EnsembleBatch, EnsembleSampler, moves, summary, targets

from test_gpu_batch_summary import dense_target, rank_set

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
_CACHE = {}


# ---------------------------------------------------------------------------------------------------------------- helpers
def make_case(name):
    """-> a sampler that has run and stored its chain (cached: the tests only read it)"""
    if name in _CACHE:
        return _CACHE[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    kw, calls, thin_by = {}, None, 1
    if name == "diag_66x7":
        N, D, steps = 66, 7, 37
        tg = targets.DiagGaussian(0.1 * rs.randn(D), 1.0 / (0.2 + rs.rand(D)))
        kw = dict(moves=moves.StretchMove(a=3))
    elif name == "dense_256x16":
        N, D, steps, tg = 256, 16, 40, dense_target(rs, 16)
    elif name == "iso_130x33":
        N, D, steps, tg = 130, 33, 20, targets.IsoGaussian()
    elif name in ("iso_48x15", "iso_48x17"):
        N, D, steps, tg = 48, int(name[-2:]), 12, targets.IsoGaussian()
    elif name == "dense_8192x64_philox":
        N, D, steps, tg = 8192, 64, 8, dense_target(rs, 64)
        kw = dict(rng="philox")
    elif name == "iso_4096x8_regrown":
        N, D, steps, tg, thin_by = 4096, 8, 64, targets.IsoGaussian(), 2
        calls = (40, 24)
    elif name == "box_32x1":
        N, D, steps, tg = 32, 1, 30, targets.UniformBox()
    elif name == "iso_64x5_mt":
        N, D, steps, tg = 64, 5, 30, targets.IsoGaussian()
    else:
        raise KeyError(name)
    p0 = rs.randn(N, D)
    if name == "box_32x1":
        p0 = rs.rand(N, 1)
        p0[:16, 0] += 100.0              # these walkers never enter [0, 1]: their stored log-probs are -inf, the first 0 is walker 16's
    s = EnsembleSampler(N, D, tg, **kw)
    s.random_state = np.random.RandomState(77).get_state()
    st = p0
    for k in calls or (steps,):
        st = s.run_mcmc(st, k, thin_by=thin_by, skip_initial_state_check=True)
    assert s.iteration == steps and s.backend._dev is not None
    _CACHE[name] = s
    return s


def check_against_host(s, discard, thin, quantiles=(0.16, 0.5, 0.84), label="", get=None, value=None):
    x = (value or s.get_chain)(discard=discard, thin=thin, flat=True)       # (n, W)
    x = x.reshape(len(x), -1)
    lp = s.get_log_prob(discard=discard, thin=thin, flat=True)              # (n), (step, walker) order
    n, W = x.shape
    what = "%s discard=%d thin=%d n=%d" % (label, discard, thin, n)
    ranks = rank_set(n, np.random.RandomState(n))
    start = discard + thin - 1
    # ---- the raw device call: order statistics
    n_dev, mean, cov, order, mx, mlp = s.backend._dev.summary(start, s.iteration, thin, ranks, True, plane=2 if value else 0)
    assert n_dev == n, what
    xs = np.sort(x, axis=0)
    assert np.array_equal(order, xs[ranks, :]), what
    # ---- the public call
    r = (get or s.get_summary)(discard=discard, thin=thin, quantiles=quantiles)
    assert isinstance(r, summary.BatchSummary)
    assert r.nsamples == n and r.mean.shape == (W,) and r.cov.shape == (W, W) and r.quantiles.shape == (len(quantiles), W)
    assert np.array_equal(r.mean, mean) and np.array_equal(r.cov, cov, equal_nan=True) and np.array_equal(r.map_coords, mx) and r.map_log_prob == mlp
    lo, hi, g = summary.quantile_ranks(n, np.asarray(quantiles, dtype=np.float64))
    assert np.array_equal(r.quantiles, summary.lerp(xs[lo, :], xs[hi, :], g[:, None])), what
    if len(quantiles):
        ref_q = np.quantile(x, quantiles, axis=0)
        bound_q = 4 * U * np.abs(x).max(axis=0)[None, :]
        print("%s: quantiles max err %.3g (bound %.3g)" % (what, np.abs(r.quantiles - ref_q).max(), bound_q.min()))
        assert (np.abs(r.quantiles - ref_q) <= bound_q).all(), what
    # ---- mean
    worst = 0.0
    for d in range(W):
        col = x[:, d]
        exact = math.fsum(col) / n
        bound = n * U * math.fsum(np.abs(col)) / n
        worst = max(worst, abs(r.mean[d] - exact) / bound if bound else 0.0)
        assert abs(r.mean[d] - exact) <= bound, (what, d, r.mean[d], exact, bound)
    print("%s: mean worst err / bound = %.3g" % (what, worst))
    # ---- covariance
    assert np.array_equal(r.cov, r.cov.T, equal_nan=True), what
    if n > 1:
        Cm = np.atleast_2d(np.cov(x.T))
        sd = np.sqrt(np.diag(Cm))
        bound = 8 * n * U * np.outer(sd, sd)
        err = np.abs(r.cov - Cm)
        print("%s: cov worst err / bound = %.3g" % (what, float((err / np.where(bound > 0, bound, 1.0)).max())))
        assert (err <= bound).all(), (what, err.max(), bound.min())
    else:
        assert np.isnan(r.cov).all()
    # ---- MAP
    at = int(np.argmax(lp))
    assert r.map_log_prob == lp.max() and r.map_log_prob == lp[at], what
    assert np.array_equal(r.map_coords, x[at]), (what, at)
    return r


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("discard,thin", [(0, 1), (5, 3), (36, 1)])
def test_small_ndim_nothing_a_tile_multiple(discard, thin):
    check_against_host(make_case("diag_66x7"), discard, thin, label="diag_66x7")


@pytest.mark.parametrize("name", ["dense_256x16", "iso_130x33", "iso_48x15", "iso_48x17", "dense_8192x64_philox", "iso_64x5_mt"])
def test_summary_equals_numpy_on_the_host_copy(name):
    s = make_case(name)
    check_against_host(s, 0, 1, label=name)
    if s.nwalkers <= 256:
        check_against_host(s, 3, 2, quantiles=(0.0, 1.0), label=name)
        check_against_host(s, 3, 2, quantiles=tuple(np.linspace(0.01, 0.99, 16)), label=name)


def test_chain_regrown_between_two_runs():
    s = make_case("iso_4096x8_regrown")
    assert s.get_chain().shape == (64, 4096, 8)
    check_against_host(s, 0, 1, label="regrown")
    check_against_host(s, 7, 5, label="regrown")


def test_box_minus_inf_first_maximum_and_the_all_minus_inf_selection():
    s = make_case("box_32x1")
    lp, x = s.get_log_prob(), s.get_chain()
    assert np.isneginf(lp[:, :16]).all() and (lp[:, 16:] == 0).all()
    for discard, thin in ((0, 1), (4, 3), (29, 1)):
        r = check_against_host(s, discard, thin, label="box")
        assert r.map_log_prob == 0 and np.array_equal(r.map_coords, x[discard + thin - 1, 16])
    # a selection whose every log-prob is -inf returns its first sample: the stuck walkers alone, as a 16-walker ensemble
    t = EnsembleSampler(16, 1, targets.UniformBox(), rng="philox")
    t.run_mcmc(100.0 + np.random.RandomState(1).rand(16, 1), 20, skip_initial_state_check=True)
    assert np.isneginf(t.get_log_prob()).all()
    for discard, thin in ((0, 1), (7, 3)):
        r = check_against_host(t, discard, thin, label="all -inf")
        assert np.isneginf(r.map_log_prob) and np.array_equal(r.map_coords, t.get_chain(discard=discard, thin=thin)[0, 0])


def test_blob_summary_on_the_device_blob_plane():
    from test_gpu_ensemble_fused_blobs import Model
    m = Model(5, 3)
    s = EnsembleSampler(32, 5, m.blobs(), rng="philox")
    s.run_mcmc(m.start(32), 25, skip_initial_state_check=True)
    assert s.backend._dev is not None and s.backend._dev_nblobs() == 3
    for discard, thin in ((0, 1), (4, 2)):
        r = check_against_host(s, discard, thin, label="blobs", get=s.get_blob_summary, value=s.get_blobs)
        assert r.mean.shape == (3,)
    check_against_host(s, 0, 1, label="blob sampler's coordinates")
    m.close()


def test_repeat_calls_and_partial_outputs_return_the_same_bits():
    for name in ("diag_66x7", "iso_130x33"):
        s = make_case(name)
        a = s.get_summary(discard=2, thin=2)
        b = s.get_summary(discard=2, thin=2)
        for u, v in zip(a, b):
            assert np.array_equal(u, v)
        nocov = s.get_summary(discard=2, thin=2, cov=False)
        assert nocov.cov is None
        noq = s.get_summary(discard=2, thin=2, quantiles=())
        assert noq.quantiles.shape == (0, s.ndim)
        for f in ("nsamples", "mean", "quantiles", "map_coords", "map_log_prob"):
            assert np.array_equal(getattr(nocov, f), getattr(a, f)), f
        for f in ("nsamples", "mean", "cov", "map_coords", "map_log_prob"):
            assert np.array_equal(getattr(noq, f), getattr(a, f)), f


@pytest.mark.parametrize("name", ["diag_66x7", "box_32x1", "iso_4096x8_regrown"])
def test_no_bit_depends_on_the_launch_shape(name):
    """tuning "summary_compact": passes 2 ... 7 of the selection on the chain itself (0), on a compacted list where it is short
    (1) or always (2)"""
    s = make_case(name)
    ens = s.backend._dev
    start, thin = 3, 2
    n = len(range(start, s.iteration, thin)) * s.nwalkers
    ranks = rank_set(n, np.random.RandomState(0))
    got = []
    for mode in (1, 0, 2, 1):
        ens.set_tuning("summary_compact", mode)
        got.append(ens.summary(start, s.iteration, thin, ranks, True))
    for g in got[1:]:
        assert all(np.array_equal(u, v) for u, v in zip(g, got[0]))
    x = s.get_chain(discard=start - thin + 1, thin=thin, flat=True)
    assert np.array_equal(got[0][3], np.sort(x, axis=0)[ranks])


def test_batch_of_one_and_the_single_sampler_agree():
    seed, N, D = 31, 32, 5
    p0 = np.random.RandomState(4).randn(N, D)
    bt = EnsembleBatch(1, N, D, targets.IsoGaussian(), seeds=[seed])
    bt.run_mcmc(p0[None], 60)
    s = EnsembleSampler(N, D, targets.IsoGaussian(), rng="philox")
    s.random_state = np.random.RandomState(seed).get_state()
    s.run_mcmc(p0, 60)
    assert np.array_equal(s.get_chain(), bt[0].get_chain())
    for kw in (dict(), dict(discard=7, thin=3)):
        a, b = check_against_host(s, kw.get("discard", 0), kw.get("thin", 1), label="single"), bt[0].get_summary(**kw)
        assert a.nsamples == b.nsamples and np.array_equal(a.quantiles, b.quantiles)
        assert np.array_equal(a.map_coords, b.map_coords) and a.map_log_prob == b.map_log_prob
        x = s.get_chain(flat=True, **kw)
        n = len(x)
        assert (np.abs(a.mean - b.mean) <= 2 * n * U * np.abs(x).sum(axis=0) / n).all()      # each within n u sum|x| / n of the exact mean
        sd = x.std(axis=0, ddof=1)
        assert (np.abs(a.cov - b.cov) <= 16 * n * U * np.outer(sd, sd)).all()                # each within 8 n u sd sd of np.cov
    bt.close()


def test_a_summary_in_the_middle_of_a_run_changes_no_later_sample():
    def run(look):
        s = EnsembleSampler(66, 7, targets.IsoGaussian(), rng="philox")
        s.random_state = np.random.RandomState(5).get_state()
        st = s.run_mcmc(np.random.RandomState(6).randn(66, 7), 20)
        if look:
            s.get_summary(discard=3, thin=2)
            s.get_summary(cov=False)
        s.run_mcmc(st, 20)
        return s
    a, b = run(False), run(True)
    assert np.array_equal(a.get_chain(), b.get_chain()) and np.array_equal(a.get_log_prob(), b.get_log_prob())
    check_against_host(b, 0, 1, label="after continuing")


def test_host_chain_of_a_user_written_move_takes_the_numpy_path():
    def proposal(x, rng):
        return x + 0.3 * rng.randn(*x.shape), np.zeros(len(x))
    s = EnsembleSampler(24, 3, targets.IsoGaussian(), moves=moves.MHMove(proposal))
    s.run_mcmc(np.random.RandomState(2).randn(24, 3), 30)
    assert s.backend._dev is None
    r = s.get_summary(discard=4, thin=2)
    x, lp = s.get_chain(discard=4, thin=2, flat=True), s.get_log_prob(discard=4, thin=2, flat=True)
    assert r.nsamples == len(x) and np.array_equal(r.mean, x.mean(axis=0)) and np.array_equal(r.cov, np.cov(x.T))
    assert np.array_equal(r.quantiles, np.quantile(x, (0.16, 0.5, 0.84), axis=0))
    at = int(np.argmax(lp))
    assert r.map_log_prob == lp[at] and np.array_equal(r.map_coords, x[at])
