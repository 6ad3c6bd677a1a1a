"""The kernels that analyse the stored chain -- emx_summary (csrc/emx_summary_single.hpp), emx_summary_batch
(csrc/emx_batch_summary.hip), the histogram kernels (emx_hist.hpp, emx_batch_hist.hpp), emx_autocorr (csrc/emx_aux.hip) and
emx_autocorr_batch (csrc/emx_batch_acf.hip) -- on chains far from the origin and under power-of-two scaling, against the exact
references of tests/chain_families.py (its docstring derives the bounds; tests/test_chain_families_cpu.py holds the references up).

Every family is a DiagGaussian run in Philox mode.  For the offset families the reference data is the exactly recentred host copy
x - mu; NumPy on the chain itself loses the digits the device could lose and is never the reference here.

  summary   counts, order statistics, the quantile interpolation and the MAP sample: exact.  Mean and covariance: the bounds of
            chain_families, the worst error / bound printed for every case.
  scaled    the chain is the centred chain times 2^(k_d) bit for bit, and so is every summary, histogram and autocorrelation time.
  tau       rtol 1e-8 (the project's tolerance for tau) against the estimator on the recentred copy, windows equal -- with the
            reference window's margin asserted, so that equality is a real check.

Before the residual pass and the two-part mean (the plain two-pass forms, one MI355X run of this file): covariance 20 ... 840 times
its bound at offset_34 and 5.8e4 ... 2.5e6 times at offset_40, mean 1.2 ... 3.8 times its bound at every offset, tau off by
5.8e-7 ... 1.7e-5 at offset_34 and 9.4e-5 ... 6.8e-4 at offset_40 (1.6e-10 ... 5.7e-10 at offset_20, inside rtol 1e-8); centred, scaled
and the histograms passed.  With them: mean <= 0.91 and covariance <= 0.03 of the bound in every case, tau within 1.3e-15.

Shapes are the smallest that reach each path: the explicit-fma Gram (66 x 7), the first MFMA width (48 x 16), a padded one
(48 x 17), the batch kernels' two Gram forms (3 of 32 x 5, 2 of 40 x 17) and PTSampler (3 rungs of 32 x 4) on the batch kernels."""
import numpy as np
import pytest

import chain_families as cf
from emcee_amd import EnsembleBatch, EnsembleSampler, PTSampler, autocorr, summary, targets
from emcee_amd.targets import BatchCallable

from test_gpu_batch_histograms import check as batch_hist_check
from test_gpu_batch_summary import rank_set
from test_gpu_ensemble_histograms import check as hist_check

pytestmark = pytest.mark.gpu

SELECTIONS = ((0, 1), (5, 3))
SINGLE = {"66x7": (66, 7, 37), "48x16": (48, 16, 12), "48x17": (48, 17, 12)}
BATCH = {"3_of_32x5": (3, 32, 5, 40), "2_of_40x17": (2, 40, 17, 12)}
PT = (3, 32, 4, 40)             # rungs, walkers, ndim, steps
_RUNS = {}


# ---------------------------------------------------------------------------------------------------------------- the runs
def _seed(*key):
    return sum(ord(c) for c in repr(key[:-1])) % 100000         # not the family: every family of a shape shares seeds


def run_single(N, D, steps, name, cache=True):
    """-> (sampler with `steps` stored steps, family)"""
    key = ("single", N, D, steps, name)
    if cache and key in _RUNS:
        return _RUNS[key]
    seed = _seed(*key)
    fam = cf.family(name, D, seed)
    s = EnsembleSampler(N, D, targets.DiagGaussian(fam["mu"], fam["ivar"]), rng="philox")
    s.random_state = np.random.RandomState(seed + 1).get_state()
    s.run_mcmc(cf.start_cloud(fam, (N,), seed + 2), steps, skip_initial_state_check=True)
    assert s.iteration == steps and s.backend._dev is not None
    if cache:
        _RUNS[key] = (s, fam)
    return s, fam


def run_batch(B, N, D, steps, name, cache=True):
    key = ("batch", B, N, D, steps, name)
    if cache and key in _RUNS:
        return _RUNS[key]
    seed = _seed(*key)
    fam = cf.family(name, D, seed)
    bt = EnsembleBatch(B, N, D, targets.DiagGaussian(fam["mu"], fam["ivar"]), seeds=[seed + 10 + b for b in range(B)])
    bt.run_mcmc(cf.start_cloud(fam, (B, N), seed + 2), steps, skip_initial_state_check=True)
    assert bt.iteration == steps
    if cache:
        _RUNS[key] = (bt, fam)
    return bt, fam


def run_pt(name):
    key = ("pt",) + PT + (name,)
    if key in _RUNS:
        return _RUNS[key]
    import torch
    T, N, D, steps = PT
    seed = _seed(*key)
    fam = cf.family(name, D, seed)
    mu_t, iv_t = torch.as_tensor(fam["mu"], device="cuda"), torch.as_tensor(fam["ivar"], device="cuda")

    def loglike(q):
        r = q - mu_t
        return -0.5 * (iv_t * r * r).sum(-1)
    s = PTSampler(T, N, D, BatchCallable(loglike), Tmax=8.0, nbatch=1, seeds=[seed + 1])
    s.run_mcmc(cf.start_cloud(fam, (1, T, N), seed + 2), steps, skip_initial_state_check=True)
    _RUNS[key] = (s, fam)
    return s, fam


# ---------------------------------------------------------------------------------------------------------------- the checks
def check_members(x, lp, ranks, raw, got, fam, quantiles, what):
    """x (M, n, D) and lp (M, n): the host copy; raw = (n, mean, cov, order, map_x, map_lp) of the device call with `ranks`, got the
    public BatchSummary, both with the leading M axis -> (worst mean err / bound, worst cov err / bound)"""
    M, n, D = x.shape
    n_dev, mean, cov, order, mx, mlp = raw
    assert n_dev == n == got.nsamples, what
    xs = np.sort(x, axis=1)
    assert np.array_equal(order, xs[:, ranks, :]), what
    assert np.array_equal(got.mean, mean) and np.array_equal(got.cov, cov) and np.array_equal(got.map_coords, mx), what
    assert np.array_equal(got.map_log_prob, mlp), what
    lo, hi, g = summary.quantile_ranks(n, np.asarray(quantiles, dtype=np.float64))
    assert np.array_equal(got.quantiles, summary.lerp(xs[:, lo, :], xs[:, hi, :], g[None, :, None])), what
    assert np.array_equal(cov, cov.transpose(0, 2, 1)), what
    worst_m = worst_c = 0.0
    for m in range(M):
        at = int(np.argmax(lp[m]))
        assert mlp[m] == lp[m, at] and np.array_equal(mx[m], x[m, at]), (what, m)
        r = cf.recentre(x[m], fam["mu"])
        mr, cr = cf.mean_ratio(mean[m], r, fam["mu"]), cf.cov_ratio(cov[m], r)
        worst_m, worst_c = max(worst_m, float(mr.max())), max(worst_c, float(cr.max()))
    print("%s: mean worst err / bound = %.3g, cov worst err / bound = %.3g" % (what, worst_m, worst_c))
    assert worst_m <= 1, (what, "mean", worst_m)
    assert worst_c <= 1, (what, "cov", worst_c)
    return worst_m, worst_c


def lift(r):
    return summary.BatchSummary(r.nsamples, *[None if a is None else np.asarray(a)[None] for a in r[1:]])


def partial_outputs_share_bits(get, full, what):
    nocov, noq = get(cov=False), get(quantiles=())
    assert nocov.cov is None and noq.quantiles.shape[-2] == 0, what
    for f in ("nsamples", "mean", "quantiles", "map_coords", "map_log_prob"):
        assert np.array_equal(getattr(nocov, f), getattr(full, f)), (what, f)
    for f in ("nsamples", "mean", "cov", "map_coords", "map_log_prob"):
        assert np.array_equal(getattr(noq, f), getattr(full, f)), (what, f)


# ---------------------------------------------------------------------------------------------------------------- summaries
@pytest.mark.parametrize("name", cf.FAMILIES)
@pytest.mark.parametrize("shape", sorted(SINGLE))
def test_single_sampler_summary(shape, name):
    N, D, steps = SINGLE[shape]
    s, fam = run_single(N, D, steps, name)
    q = (0.16, 0.5, 0.84)
    for discard, thin in SELECTIONS:
        what = "single %s %s discard=%d thin=%d" % (shape, name, discard, thin)
        x = s.get_chain(discard=discard, thin=thin, flat=True)
        lp = s.get_log_prob(discard=discard, thin=thin, flat=True)
        ranks = rank_set(len(x), np.random.RandomState(len(x)))
        raw = s.backend._dev.summary(discard + thin - 1, s.iteration, thin, ranks, True)
        raw = (raw[0],) + tuple(np.asarray(a)[None] for a in raw[1:])
        full = s.get_summary(discard=discard, thin=thin, quantiles=q)
        check_members(x[None], lp[None], ranks, raw, lift(full), fam, q, what)
        partial_outputs_share_bits(lambda **kw: s.get_summary(discard=discard, thin=thin, **kw), full, what)


@pytest.mark.parametrize("name", cf.FAMILIES)
@pytest.mark.parametrize("shape", sorted(BATCH))
def test_batch_summary(shape, name):
    B, N, D, steps = BATCH[shape]
    bt, fam = run_batch(B, N, D, steps, name)
    q = (0.16, 0.5, 0.84)
    for discard, thin in SELECTIONS:
        what = "batch %s %s discard=%d thin=%d" % (shape, name, discard, thin)
        x = bt.get_chain(discard=discard, thin=thin, flat=True)
        lp = bt.get_log_prob(discard=discard, thin=thin, flat=True)
        ranks = rank_set(x.shape[1], np.random.RandomState(x.shape[1]))
        raw = bt._summary_device(discard, thin, ranks, True)
        full = bt.get_summary(discard=discard, thin=thin, quantiles=q)
        check_members(x, lp, ranks, raw, full, fam, q, what)
        partial_outputs_share_bits(lambda **kw: bt.get_summary(discard=discard, thin=thin, **kw), full, what)
        # a member on its own, and members in passes of one: the same bits
        one = bt[B - 1].get_summary(discard=discard, thin=thin, quantiles=q)
        assert all(np.array_equal(u, v[B - 1]) for u, v in zip(one[1:], full[1:])), what
        bt.set_tuning("batch_summary_members", 1)
        again = bt._summary_device(discard, thin, ranks, True)
        bt.set_tuning("batch_summary_members", 0)
        assert all(np.array_equal(u, v) for u, v in zip(again, raw)), what


@pytest.mark.parametrize("name", cf.FAMILIES)
def test_ptsampler_summary_goes_through_the_batch_kernels(name):
    s, fam = run_pt(name)
    T, N, D, steps = PT
    q = (0.16, 0.5, 0.84)
    for discard, thin in SELECTIONS:
        what = "pt %s discard=%d thin=%d" % (name, discard, thin)
        x = s.get_chain(discard=discard, thin=thin, flat=True).reshape(T, -1, D)          # (1, T, n, D)
        lp = s.get_log_prob(discard=discard, thin=thin, flat=True).reshape(T, -1)         # tempered
        ranks = rank_set(x.shape[1], np.random.RandomState(x.shape[1]))
        raw = s._b._summary_device(discard, thin, ranks, True)
        r = s.get_summary(discard=discard, thin=thin, quantiles=q)
        assert r.mean.shape == (1, T, D) and r.cov.shape == (1, T, D, D)
        full = summary.BatchSummary(r.nsamples, *[np.asarray(a).reshape((T,) + np.asarray(a).shape[2:]) for a in r[1:]])
        check_members(x, lp, ranks, raw, full, fam, q, what)
        partial_outputs_share_bits(lambda **kw: s.get_summary(discard=discard, thin=thin, **kw), r, what)


@pytest.mark.parametrize("name", ["offset_34", "offset_40"])
def test_summary_compact_changes_no_bit_on_an_offset_family(name):
    """every key of an offset column shares its top 16 bits and more: the compaction list is the whole selection"""
    N, D, steps = SINGLE["66x7"]
    s, fam = run_single(N, D, steps, name)
    ens = s.backend._dev
    start, thin = 3, 2
    x = s.get_chain(discard=start - thin + 1, thin=thin, flat=True)
    ranks = rank_set(len(x), np.random.RandomState(0))
    got = []
    for mode in (1, 0, 2, 1):
        ens.set_tuning("summary_compact", mode)
        got.append(ens.summary(start, s.iteration, thin, ranks, True))
    for g in got[1:]:
        assert all(np.array_equal(u, v) for u, v in zip(g, got[0])), name
    assert np.array_equal(got[0][3], np.sort(x, axis=0)[ranks])
    assert cf.cov_ratio(got[0][2], cf.recentre(x, fam["mu"])).max() <= 1


# ---------------------------------------------------------------------------------------------------------------- scale covariance
def _hist_same_scaled(a, b, sc):
    """Histograms b of the scaled chain against a of the centred one: edges times the scale, counts equal"""
    assert a.nsamples == b.nsamples and np.array_equal(a.pairs, b.pairs)
    for d in range(len(sc)):
        assert np.array_equal(np.asarray(a.edges[d]) * sc[d], b.edges[d]) and np.array_equal(np.asarray(a.pair_edges[d]) * sc[d], b.pair_edges[d])
        assert np.array_equal(a.counts[d], b.counts[d]), d
    assert len(a.pair_counts) == len(b.pair_counts) and all(np.array_equal(u, v) for u, v in zip(a.pair_counts, b.pair_counts))


def _scale_checks(a, b, sc, tau_of):
    """a: the centred run, b: the scaled one (samplers or batches)"""
    xa, xb = a.get_chain(), b.get_chain()
    assert np.array_equal(xa * sc, xb) and np.array_equal(a.get_log_prob(), b.get_log_prob())       # the premise
    for discard, thin in SELECTIONS:
        ra, rb = a.get_summary(discard=discard, thin=thin), b.get_summary(discard=discard, thin=thin)
        assert ra.nsamples == rb.nsamples and np.array_equal(ra.map_log_prob, rb.map_log_prob)
        assert np.array_equal(ra.mean * sc, rb.mean)
        assert np.array_equal(ra.cov * np.outer(sc, sc), rb.cov)
        assert np.array_equal(ra.quantiles * sc, rb.quantiles) and np.array_equal(ra.map_coords * sc, rb.map_coords)
        flat = xa[..., discard + thin - 1::thin, :, :].reshape(-1, len(sc))
        lo, hi = flat.min(axis=0), flat.max(axis=0)
        rng = np.stack([lo + 0.2 * (hi - lo), hi - 0.1 * (hi - lo)], axis=1)                        # some samples fall outside
        for r_a, r_b in ((None, None), (rng, rng * sc[:, None])):
            for pair_bins in (64, 1):
                _hist_same_scaled(a.get_histograms(bins=64, range=r_a, pair_bins=pair_bins, discard=discard, thin=thin),
                                  b.get_histograms(bins=64, range=r_b, pair_bins=pair_bins, discard=discard, thin=thin), sc)
        if tau_of is not None:
            ta, tb = tau_of(a, discard, thin), tau_of(b, discard, thin)
            assert np.array_equal(ta[0], tb[0]) and np.array_equal(ta[1], tb[1]) and np.isfinite(ta[0]).all()


@pytest.mark.parametrize("shape", sorted(SINGLE) + ["32x5"])
def test_single_sampler_scale_covariance(shape):
    N, D, steps = SINGLE.get(shape, (32, 5, 257))
    (a, _), (b, fam) = run_single(N, D, steps, "centred"), run_single(N, D, steps, "scaled")
    assert np.array_equal(np.log2(fam["scale"]), cf.scale_exponents(D))
    _scale_checks(a, b, fam["scale"], (lambda s, discard, thin: s.backend._dev.autocorr(discard, thin, 5.0)[:2]) if steps > 100 else None)


@pytest.mark.parametrize("shape", sorted(BATCH) + ["3_of_32x5_long"])
def test_batch_scale_covariance(shape):
    B, N, D, steps = BATCH.get(shape, (3, 32, 5, 257))
    (a, _), (b, fam) = run_batch(B, N, D, steps, "centred"), run_batch(B, N, D, steps, "scaled")
    _scale_checks(a, b, fam["scale"], (lambda s, discard, thin: s._autocorr_device(discard, thin)[:2]) if steps > 100 else None)


# ---------------------------------------------------------------------------------------------------------------- autocorrelation
ACF_SELECTIONS = ((0, 1), (50, 4))


def _tau_against_reference(x, fam, device, what):
    """x (nt, N, D): the host copy of the selection; device: (tau, windows) of the code under test -> worst relative tau error"""
    r = cf.recentre(x, fam["mu"])
    tau, win, margin = cf.reference_tau(r)
    assert (margin > 1e-6).all(), (what, "the reference window is about to tip", margin)
    np.testing.assert_allclose(device[0], tau, rtol=1e-8, atol=0, err_msg=what)
    assert np.array_equal(device[1], win), (what, device[1], win)
    # the host estimator on the chain as it is, far from the origin
    h_tau = autocorr.integrated_time(x, tol=0, quiet=True)
    h_win = [autocorr.tau_from_mean_acf(autocorr._batched_acf(x[:, :, d]).mean(axis=1), 5)[0] for d in range(x.shape[2])]
    np.testing.assert_allclose(h_tau, tau, rtol=1e-8, atol=0, err_msg=what + " (host)")
    assert np.array_equal(h_win, win), (what, "host")
    return float(np.abs(device[0] / tau - 1).max()), float(np.abs(h_tau / tau - 1).max())


@pytest.mark.parametrize("name", cf.FAMILIES)
def test_single_sampler_autocorr(name):
    s, fam = run_single(32, 5, 256, name, cache=False)
    for stored in (256, 257):                       # a power of two, then one past it: the next FFT length
        if stored == 257:
            s.run_mcmc(None, 1)
        assert s.iteration == stored
        for discard, thin in ACF_SELECTIONS:
            what = "single acf %s stored=%d discard=%d thin=%d" % (name, stored, discard, thin)
            tau, win, nt = s.backend._dev.autocorr(discard, thin, 5.0)
            x = s.get_chain(discard=discard, thin=thin)
            assert nt == len(x)
            worst = _tau_against_reference(x, fam, (tau, win), what)
            print("%s: tau worst relative error %.3g (device), %.3g (host)" % ((what,) + worst))
            assert np.array_equal(s.get_autocorr_time(discard=discard, thin=thin, quiet=True), thin * tau)


@pytest.mark.parametrize("name", cf.FAMILIES)
def test_batch_autocorr(name):
    B, N, D = 3, 32, 5
    bt, fam = run_batch(B, N, D, 256, name, cache=False)
    for stored in (256, 257):
        if stored == 257:
            bt.run_mcmc(None, 1)
        assert bt.iteration == stored
        for discard, thin in ACF_SELECTIONS:
            tau, win, nt = bt._autocorr_device(discard=discard, thin=thin)
            x = bt.get_chain(discard=discard, thin=thin)
            assert nt == x.shape[1]
            for b in range(B):
                what = "batch acf %s stored=%d discard=%d thin=%d member %d" % (name, stored, discard, thin, b)
                worst = _tau_against_reference(x[b], fam, (tau[b], win[b]), what)
                print("%s: tau worst relative error %.3g (device), %.3g (host)" % ((what,) + worst))
            full = bt.get_autocorr_time(discard=discard, thin=thin, quiet=True, on_device=True)
            assert np.array_equal(full, thin * tau)
            assert np.array_equal(bt[1].get_autocorr_time(discard=discard, thin=thin, quiet=True, on_device=True), full[1])
    bt.close()


@pytest.mark.parametrize("name", ["offset_34", "offset_40"])
def test_acf_chunking_changes_no_bit_on_an_offset_family(name):
    B, N, D = 3, 32, 5
    bt, fam = run_batch(B, N, D, 257, name)
    ref = bt._autocorr_device(discard=20, thin=2)
    for series in (7, N * D + 13, 0):
        bt.set_tuning("batch_acf_series", series)
        got = bt._autocorr_device(discard=20, thin=2)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2] == ref[2], (name, series)
    x = bt.get_chain(discard=20, thin=2)
    for b in range(B):
        _tau_against_reference(x[b], fam, (ref[0][b], ref[1][b]), "chunking %s member %d" % (name, b))


# ---------------------------------------------------------------------------------------------------------------- histograms
def _explicit_range(fam, D):
    return np.stack([fam["mu"] - 1.5 * fam["sd"], fam["mu"] + 2.0 * fam["sd"]], axis=1)     # some samples fall outside


@pytest.mark.parametrize("pair_bins", [64, 1])
def test_single_sampler_histograms_at_offset_34(pair_bins):
    N, D, steps = SINGLE["66x7"]
    s, fam = run_single(N, D, steps, "offset_34")
    for discard, thin in SELECTIONS:
        x = s.get_chain(discard=discard, thin=thin, flat=True)
        h = hist_check(x, s.get_histograms(bins=64, pair_bins=pair_bins, discard=discard, thin=thin), 64, pair_bins=pair_bins, label="range=None")
        assert all(c.sum() == len(x) for c in h.counts)
        rng = _explicit_range(fam, D)
        h = hist_check(x, s.get_histograms(bins=64, range=rng, pair_bins=pair_bins, discard=discard, thin=thin), 64, rng=rng, pair_bins=pair_bins,
                       label="explicit range")
        assert any(c.sum() < len(x) for c in h.counts)


@pytest.mark.parametrize("pair_bins", [64, 1])
def test_batch_histograms_at_offset_34(pair_bins):
    B, N, D, steps = BATCH["3_of_32x5"]
    bt, fam = run_batch(B, N, D, steps, "offset_34")
    for discard, thin in SELECTIONS:
        x = bt.get_chain(discard=discard, thin=thin, flat=True)
        batch_hist_check(bt.get_histograms(bins=64, pair_bins=pair_bins, discard=discard, thin=thin), x, 64, pair_bins=pair_bins, what="range=None")
        rng = _explicit_range(fam, D)
        r = bt.get_histograms(bins=64, range=rng, pair_bins=pair_bins, discard=discard, thin=thin)
        batch_hist_check(r, x, 64, rng=rng, pair_bins=pair_bins, what="explicit range")
        assert any(c.sum() < B * x.shape[1] for c in r.counts)
