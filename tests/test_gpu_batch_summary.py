"""EnsembleBatch.get_summary: emx_summary_batch (csrc/emx_batch_summary.hip) against NumPy on the host copy of the same
chain (get_chain / get_log_prob, never the code under test).

Order statistics, the MAP sample and the quantiles' interpolation are exact.  The mean and the covariance are held to
first-order worst-case bounds of ANY summation order (derived, not measured; u = 2^-53):
  |mean - fsum(x) / n|  <=  n u sum|x| / n                          (math.fsum is the exact reference)
  |cov_jk - C_jk|       <=  8 n u sqrt(C_jj C_kk),  C = np.cov      (Cauchy-Schwarz: sum|a_j a_k| <= (n - 1) sqrt(C_jj C_kk);
                                                                     each side's summation error is below (n + 3) u of that,
                                                                     8 covers both sides and the centring)
Rejected proposals repeat rows, so every chain here has ties."""
import math

import numpy as np
import pytest

from emcee_amd import EnsembleBatch, PTSampler, moves, summary, targets
from emcee_amd.targets import BatchCallable

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


# ---------------------------------------------------------------------------------------------------------------- helpers
def gauss_params(rs, B, D):
    return 0.1 * rs.randn(B, D), 1.0 / (0.2 + rs.rand(B, D))


def batched_fn(mu, ivar):
    import torch
    mu_t = torch.as_tensor(mu, device="cuda")[:, None, :]
    iv_t = torch.as_tensor(ivar, device="cuda")[:, None, :]

    def fn(q):
        return -0.5 * (iv_t * (q - mu_t) ** 2).sum(-1)
    return fn


def dense_target(rs, D):
    A = rs.randn(D, D)
    icov = np.linalg.inv(A @ A.T / D + 0.5 * np.eye(D))
    return targets.DenseGaussian(0.1 * rs.randn(D), 0.5 * (icov + icov.T))


def make_case(name, rs):
    """-> (B, N, D, target, moves factory, initial state)"""
    B = 3
    if name == "iso_32x5_stretch":
        return B, 32, 5, targets.IsoGaussian(), lambda: moves.StretchMove(), rs.randn(B, 32, 5)
    if name == "diag_100x10_de_snooker":
        mu, iv = gauss_params(rs, B, 10)
        return B, 100, 10, [targets.DiagGaussian(mu[b], iv[b]) for b in range(B)], \
            lambda: [(moves.DEMove(), 0.8), (moves.DESnookerMove(), 0.2)], rs.randn(B, 100, 10)
    if name == "dense_64x3":
        return B, 64, 3, dense_target(rs, 3), lambda: moves.StretchMove(), rs.randn(B, 64, 3)
    if name == "dense_64x32":
        return B, 64, 32, dense_target(rs, 32), lambda: moves.StretchMove(), rs.randn(B, 64, 32)
    if name == "box_32x1":
        p0 = rs.rand(B, 32, 1)
        p0[1, :16, 0] += 100.0          # these walkers never enter [0, 1]: their stored log-probs are -inf, the first 0 is walker 16's
        return B, 32, 1, targets.UniformBox(), lambda: moves.StretchMove(), p0
    if name == "callable_32x4":
        mu, iv = gauss_params(rs, B, 4)
        return B, 32, 4, BatchCallable(batched_fn(mu, iv)), lambda: moves.StretchMove(), rs.randn(B, 32, 4)
    raise KeyError(name)


CASES = ["iso_32x5_stretch", "diag_100x10_de_snooker", "dense_64x3", "dense_64x32", "box_32x1", "callable_32x4"]


def sampled(name, nsteps, seed=0):
    rs = np.random.RandomState(seed)
    B, N, D, tg, mf, p0 = make_case(name, rs)
    bt = EnsembleBatch(B, N, D, tg, moves=mf(), seeds=[100 + b for b in range(B)])
    bt.run_mcmc(p0, nsteps, skip_initial_state_check=True)
    return bt


def rank_set(n, rs):
    """0, n - 1, adjacent pairs, a repeated rank, random ones: at most 32, unsorted"""
    r = [0, n - 1, n // 2, min(n // 2 + 1, n - 1), n // 2, n // 6, min(n // 6 + 1, n - 1)] + rs.randint(0, n, size=9).tolist()
    return np.array(r, dtype=np.int64)


def check_against_host(bt, discard, thin, quantiles=(0.16, 0.5, 0.84), label=""):
    x = bt.get_chain(discard=discard, thin=thin, flat=True)              # (B, n, D)
    lp = bt.get_log_prob(discard=discard, thin=thin, flat=True)          # (B, n), (step, walker) order
    B, n, D = x.shape
    what = "%s discard=%d thin=%d n=%d" % (label, discard, thin, n)
    rs = np.random.RandomState(n)
    ranks = rank_set(n, rs)
    # ---- the raw device call: order statistics
    n_dev, mean, cov, order, mx, mlp = bt._summary_device(discard, thin, ranks, True)
    assert n_dev == n, what
    xs = np.sort(x, axis=1)
    assert np.array_equal(order, xs[:, ranks, :]), what
    # ---- the public call
    s = bt.get_summary(discard=discard, thin=thin, quantiles=quantiles)
    assert s.nsamples == n and s.mean.shape == (B, D) and s.cov.shape == (B, D, D) and s.quantiles.shape == (B, len(quantiles), D)
    assert np.array_equal(s.mean, mean) and np.array_equal(s.cov, cov) and np.array_equal(s.map_coords, mx) and np.array_equal(s.map_log_prob, mlp)
    lo, hi, g = summary.quantile_ranks(n, np.asarray(quantiles, dtype=np.float64))
    assert np.array_equal(s.quantiles, summary.lerp(xs[:, lo, :], xs[:, hi, :], g[None, :, None])), what
    if len(quantiles):
        ref_q = np.quantile(x, quantiles, axis=1).transpose(1, 0, 2)
        bound_q = 4 * U * np.abs(x).max(axis=1)[:, None, :]
        print("%s: quantiles max err %.3g (bound %.3g)" % (what, np.abs(s.quantiles - ref_q).max(), bound_q.min()))
        assert (np.abs(s.quantiles - ref_q) <= bound_q).all(), what
    # ---- mean
    for b in range(B):
        for d in range(D):
            col = x[b, :, d]
            exact = math.fsum(col) / n
            bound = n * U * math.fsum(np.abs(col)) / n
            assert abs(s.mean[b, d] - exact) <= bound, (what, b, d, s.mean[b, d], exact, bound)
    # ---- covariance
    assert np.array_equal(s.cov, s.cov.transpose(0, 2, 1)), what
    if n > 1:
        worst = 0.0
        for b in range(B):
            Cm = np.atleast_2d(np.cov(x[b].T))
            sd = np.sqrt(np.diag(Cm))
            bound = 8 * n * U * np.outer(sd, sd)
            err = np.abs(s.cov[b] - Cm)
            worst = max(worst, float((err / np.where(bound > 0, bound, 1.0)).max()))
            assert (err <= bound).all(), (what, b, err.max(), bound.min())
        print("%s: cov worst err / bound = %.3g" % (what, worst))
    else:
        assert np.isnan(s.cov).all()                                     # ddof = 1 of one sample, as np.cov
    # ---- MAP
    for b in range(B):
        at = int(np.argmax(lp[b]))
        assert s.map_log_prob[b] == lp[b].max() and s.map_log_prob[b] == lp[b, at], (what, b)
        assert np.array_equal(s.map_coords[b], x[b, at]), (what, b, at)
    return s


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("name", CASES)
def test_summary_equals_numpy_on_the_host_copy(name):
    bt = sampled(name, 256)
    for stored in (256, 257):
        if stored == 257:
            bt.run_mcmc(None, 1)
        assert bt.iteration == stored
        for discard, thin in ((0, 1), (50, 4), (stored - 1, 1)):
            check_against_host(bt, discard, thin, label=name)
    # other quantile sets: the ends, none, sixteen
    check_against_host(bt, 10, 3, quantiles=(0.0, 1.0), label=name)
    check_against_host(bt, 10, 3, quantiles=(), label=name)
    check_against_host(bt, 10, 3, quantiles=tuple(np.linspace(0.01, 0.99, 16)), label=name)
    bt.close()


def test_box_log_probs_hold_minus_inf_and_the_first_maximum_wins():
    bt = sampled("box_32x1", 64)
    lp = bt.get_log_prob()
    assert np.isneginf(lp[1, :, :16]).all() and (lp[1, :, 16:] == 0).all() and (lp[0] == 0).all()
    s = bt.get_summary()
    x = bt.get_chain()
    assert (s.map_log_prob == 0).all()
    assert np.array_equal(s.map_coords[0], x[0, 0, 0]) and np.array_equal(s.map_coords[1], x[1, 0, 16])
    bt.close()


def test_a_member_whose_every_log_prob_is_minus_inf_returns_its_first_sample():
    rs = np.random.RandomState(3)
    p0 = rs.rand(3, 32, 1)
    p0[2] += 100.0                                  # member 2 never enters the box
    bt = EnsembleBatch(3, 32, 1, targets.UniformBox(), seeds=[5, 6, 7])
    bt.run_mcmc(p0, 40, skip_initial_state_check=True)
    assert np.isneginf(bt.get_log_prob()[2]).all()
    for discard, thin in ((0, 1), (7, 3)):
        s = check_against_host(bt, discard, thin, label="all -inf")
        assert np.isneginf(s.map_log_prob[2])
        assert np.array_equal(s.map_coords[2], bt.get_chain(discard=discard, thin=thin)[2, 0, 0])
    bt.close()


def test_cov_false_returns_none_and_computes_no_gram():
    bt = sampled("iso_32x5_stretch", 100, seed=2)
    full = bt.get_summary(discard=5, thin=2)
    s = bt.get_summary(discard=5, thin=2, cov=False)
    assert s.cov is None
    for a, b in zip(s, full):
        if b is not full.cov:
            assert np.array_equal(a, b)
    assert bt[1].get_summary(cov=False).cov is None
    bt.close()


@pytest.mark.parametrize("name", ["iso_32x5_stretch", "dense_64x32"])
def test_no_bit_depends_on_the_launch_shape(name):
    bt = sampled(name, 300, seed=5)
    n = len(range(20 + 2 - 1, 300, 2)) * bt.nwalkers
    ranks = rank_set(n, np.random.RandomState(0))
    ref = bt._summary_device(20, 2, ranks, True)
    check_against_host(bt, 20, 2, label=name)

    def same(a, b):
        return all(np.array_equal(u, v) for u, v in zip(a, b))
    for members in (1, 2, 0):
        bt.set_tuning("batch_summary_members", members)
        assert same(bt._summary_device(20, 2, ranks, True), ref), "batch_summary_members=%d" % members
    one = bt._summary_device(20, 2, ranks, True, 1, 2)
    assert one[0] == ref[0] and all(np.array_equal(u[0], v[1]) for u, v in zip(one[1:], ref[1:]))
    full = bt.get_summary(discard=20, thin=2)
    for b in range(bt.nbatch):
        m = bt[b].get_summary(discard=20, thin=2)
        assert m.nsamples == full.nsamples
        for u, v in zip(m[1:], full[1:]):
            assert u.shape == v.shape[1:] and np.array_equal(u, v[b])
    bt.close()


def test_ptsampler_summary_is_the_batch_summary_reshaped():
    G, T, N, D = 2, 3, 32, 2
    fn = lambda q: -0.5 * (q * q).sum(-1) - np.log(2 * np.pi)  # noqa: E731
    s = PTSampler(T, N, D, BatchCallable(fn), log_prior=(-10 * np.ones(D), 10 * np.ones(D)), Tmax=20.0, nbatch=G, seeds=[3, 4])
    s.run_mcmc(np.random.RandomState(0).uniform(-1, 1, size=(G, T, N, D)), 120)
    r = s.get_summary(discard=20, thin=2)
    flat = s._b.get_summary(discard=20, thin=2)
    assert r.nsamples == flat.nsamples == 50 * N
    assert r.mean.shape == (G, T, D) and r.cov.shape == (G, T, D, D) and r.quantiles.shape == (G, T, 3, D)
    assert r.map_coords.shape == (G, T, D) and r.map_log_prob.shape == (G, T)
    for u, v in zip(r[1:], flat[1:]):
        assert np.array_equal(u, v.reshape(u.shape))
    lp = s.get_log_prob(discard=20, thin=2, flat=True)                   # (G, T, n) tempered
    x = s.get_chain(discard=20, thin=2, flat=True)
    for gidx in range(G):
        for t in range(T):
            at = int(np.argmax(lp[gidx, t]))
            assert r.map_log_prob[gidx, t] == lp[gidx, t, at]
            assert np.array_equal(r.map_coords[gidx, t], x[gidx, t, at])
            np.testing.assert_allclose(r.mean[gidx, t], x[gidx, t].mean(axis=0), rtol=0, atol=1e-12)
    assert s.get_summary(cov=False).cov is None
    s.close()


def test_the_sampler_is_untouched():
    a = sampled("diag_100x10_de_snooker", 60, seed=7)
    b = sampled("diag_100x10_de_snooker", 60, seed=7)
    b.get_summary(discard=5, thin=2)
    b[1].get_summary()
    a.run_mcmc(None, 40)
    b.run_mcmc(None, 40)
    assert np.array_equal(a.get_chain(), b.get_chain()) and np.array_equal(a.get_log_prob(), b.get_log_prob())
    assert np.array_equal(a.get_last_sample().coords, b.get_last_sample().coords)
    check_against_host(b, 0, 1, label="after continuing")
    a.close()
    b.close()
