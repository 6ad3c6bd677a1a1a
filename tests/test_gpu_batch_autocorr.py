"""EnsembleBatch.get_autocorr_time(on_device=True): emx_autocorr_batch (csrc/emx_batch_acf.hip) must compute, for every
member and parameter, what the host estimator integrated_time computes on that member's chain -- the tolerances
test_gpu_sampler_api.py holds emx_autocorr to: tau at rtol 1e-8, Sokal windows exactly -- and what the single Philox-mode
sampler's emx_autocorr computes for the same member (rtol 1e-12).  Chunk boundaries (tuning "batch_acf_series") must not
change a bit."""
import logging
import time

import numpy as np
import pytest

from emcee_amd import EnsembleBatch, EnsembleSampler, autocorr, moves, targets
from emcee_amd.targets import BatchCallable

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- helpers
def host_estimate(bt, discard, thin, c):
    """(tau, windows) of every member from a host copy of its chain: integrated_time and tau_from_mean_acf"""
    x = bt.get_chain(discard=discard, thin=thin)
    B, _, _, D = x.shape
    tau = np.stack([autocorr.integrated_time(x[b], c=c, tol=0, quiet=True) for b in range(B)])
    win = np.array([[autocorr.tau_from_mean_acf(autocorr._batched_acf(x[b, :, :, d]).mean(axis=1), c)[0] for d in range(D)]
                    for b in range(B)])
    return tau, win, x.shape[1]


def assert_matches_host(bt, discard, thin, c=5, rtol=1e-8, atol=0.0):
    tau, win, nt = bt._autocorr_device(discard=discard, thin=thin, c=c)
    h_tau, h_win, h_nt = host_estimate(bt, discard, thin, c)
    assert nt == h_nt
    np.testing.assert_allclose(tau, h_tau, rtol=rtol, atol=atol, err_msg="discard=%d thin=%d c=%g" % (discard, thin, c))
    np.testing.assert_array_equal(win, h_win, err_msg="discard=%d thin=%d c=%g" % (discard, thin, c))
    return tau, win, nt


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
    """-> (B, N, D, target, moves factory)"""
    B = 3
    if name == "iso_32x5_stretch":
        return B, 32, 5, targets.IsoGaussian(), lambda: moves.StretchMove()
    if name == "diag_100x10_de_snooker":
        mu, iv = gauss_params(rs, B, 10)
        return B, 100, 10, [targets.DiagGaussian(mu[b], iv[b]) for b in range(B)], \
            lambda: [(moves.DEMove(), 0.8), (moves.DESnookerMove(), 0.2)]
    if name == "dense_64x3":
        return B, 64, 3, dense_target(rs, 3), lambda: moves.StretchMove()
    if name == "callable_32x4":
        mu, iv = gauss_params(rs, B, 4)
        return B, 32, 4, BatchCallable(batched_fn(mu, iv)), lambda: moves.StretchMove()
    raise KeyError(name)


def sampled(name, nsteps, seed=0):
    rs = np.random.RandomState(seed)
    B, N, D, tg, mf = make_case(name, rs)
    bt = EnsembleBatch(B, N, D, tg, moves=mf(), seeds=[100 + b for b in range(B)])
    bt.run_mcmc(rs.randn(B, N, D), nsteps)
    return bt


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("name", ["iso_32x5_stretch", "diag_100x10_de_snooker", "dense_64x3", "callable_32x4"])
def test_device_equals_host_estimator(name):
    bt = sampled(name, 256)
    for stored in (256, 257):                   # nt a power of two, then one past it (the next FFT length)
        if stored == 257:
            bt.run_mcmc(None, 1)
        assert bt.iteration == stored
        for discard, thin in ((0, 1), (50, 4), (stored - 1, 1)):
            tau, win, nt = assert_matches_host(bt, discard, thin)
            assert nt == len(range(discard + thin - 1, stored, thin))
        # the public call: thin * tau, the member view agreeing with its row
        full = bt.get_autocorr_time(discard=50, thin=4, quiet=True, on_device=True)
        tau, _, _ = bt._autocorr_device(discard=50, thin=4)
        assert np.array_equal(full, 4 * tau)
        for b in range(bt.nbatch):
            assert np.array_equal(bt[b].get_autocorr_time(discard=50, thin=4, quiet=True, on_device=True), full[b])
    bt.close()


def test_window_constant_c_and_degenerate_cases():
    """c is not restricted (as in the reference).  c = 0: no lag is below c tau, the window is the last lag.  c = 1e6: the
    window is where tau(m) has fallen to ~m / c; for a centred series tau(nt - 1) is 0 in exact arithmetic (the ACF sums to
    1/2), so there tau can be rounding noise of 1e-14: compared with atol 1e-12 besides rtol 1e-8."""
    bt = sampled("iso_32x5_stretch", 300, seed=3)
    for c in (1e-9, 0.5, 5, 1e6, 0.0, -1.0):
        tau, win, nt = assert_matches_host(bt, 0, 1, c=c, atol=1e-12)
        if c == 1e-9:
            assert (win == 1).all()             # lag 0 is below (0 < c tau(0) = c), lag 1 is not
        if c == 1e6:
            assert (win > 50).all()
        if c == 0.0:
            assert (win == nt - 1).all()
    bt.close()


def test_constant_coordinate_is_nan_and_never_flagged():
    B, N, D = 3, 32, 3
    rs = np.random.RandomState(4)
    p0 = rs.randn(B, N, D)
    p0[1, :, 2] = 0.5                            # the stretch move keeps it exactly 0.5
    bt = EnsembleBatch(B, N, D, targets.IsoGaussian(), seeds=[1, 2, 3])
    bt.run_mcmc(p0, 200, skip_initial_state_check=True)
    assert (bt.get_chain()[1, :, :, 2] == 0.5).all()
    tau, win, nt = bt._autocorr_device()
    h_tau, h_win, _ = host_estimate(bt, 0, 1, 5)
    assert np.array_equal(np.isnan(tau), np.isnan(h_tau)) and np.isnan(tau[1, 2]) and np.isnan(tau).sum() == 1
    assert win[1, 2] == nt - 1 and np.array_equal(win, h_win)
    fin = np.isfinite(tau)
    np.testing.assert_allclose(tau[fin], h_tau[fin], rtol=1e-8)
    tol = 0.5 * nt / tau[fin].max()              # nothing finite is flagged: the NaN must not be either
    out = bt.get_autocorr_time(tol=tol, on_device=True)
    assert np.isnan(out[1, 2])
    assert np.isnan(bt[1].get_autocorr_time(tol=tol, on_device=True)[2])


def test_member_equals_single_sampler_emx_autocorr():
    B, N, D = 4, 32, 5
    rs = np.random.RandomState(9)
    mu, iv = gauss_params(rs, B, D)
    tg = [targets.DiagGaussian(mu[b], iv[b]) for b in range(B)]
    p0 = rs.randn(B, N, D)
    seeds = [11, 22, 33, 44]
    mf = lambda: [moves.StretchMove(), moves.DEMove()]  # noqa: E731
    bt = EnsembleBatch(B, N, D, tg, moves=mf(), seeds=seeds)
    bt.run_mcmc(p0, 400)
    for b in range(B):
        s = EnsembleSampler(N, D, tg[b], moves=mf(), rng="philox")
        s.random_state = np.random.RandomState(seeds[b]).get_state()
        s.run_mcmc(p0[b], 400)
        assert np.array_equal(s.get_chain(), bt[b].get_chain())
        assert s.backend._dev is not None                   # its get_autocorr_time takes emx_autocorr
        for kw in (dict(), dict(discard=50, thin=4)):
            np.testing.assert_allclose(bt.get_autocorr_time(quiet=True, on_device=True, **kw)[b], s.get_autocorr_time(quiet=True, **kw),
                                       rtol=1e-12)


def test_chunk_boundaries_do_not_change_bits():
    bt = sampled("iso_32x5_stretch", 300, seed=5)
    ND = bt.nwalkers * bt.ndim
    ref = None
    for series in (0, 1, 7, ND - 1, ND + 13, 0):         # boundaries inside members, across them, one series a chunk
        bt.set_tuning("batch_acf_series", series)
        got = bt._autocorr_device(discard=20, thin=2)
        if ref is None:
            ref = got
            assert_matches_host(bt, 20, 2)
            continue
        assert np.array_equal(got[0], ref[0]), "batch_acf_series=%d" % series
        assert np.array_equal(got[1], ref[1]) and got[2] == ref[2]
        for b in range(bt.nbatch):
            assert np.array_equal(bt[b].get_autocorr_time(discard=20, thin=2, quiet=True, on_device=True), 2 * ref[0][b])
    bt.close()


def test_tol_raises_or_warns_naming_members(caplog):
    bt = sampled("diag_100x10_de_snooker", 120, seed=6)
    tau, _, nt = bt._autocorr_device()
    worst = tau.max(axis=1)
    order = np.sort(worst)
    tol = nt / (0.5 * (order[0] + order[1]))             # members above the lowest one are flagged
    flagged = [b for b in range(bt.nbatch) if (tol * tau[b] > nt).any()]
    assert 0 < len(flagged) < bt.nbatch
    with pytest.raises(autocorr.AutocorrError) as e:
        bt.get_autocorr_time(tol=tol, on_device=True)
    assert ("members " if len(flagged) > 1 else "member ") + ", ".join(map(str, flagged)) + "." in str(e.value)
    assert np.array_equal(e.value.tau, tau)
    with caplog.at_level(logging.WARNING, logger="emcee_amd.autocorr"):
        out = bt.get_autocorr_time(tol=tol, quiet=True, on_device=True)
    assert np.array_equal(out, tau) and ", ".join(map(str, flagged)) in caplog.text
    ok = [b for b in range(bt.nbatch) if b not in flagged][0]
    assert np.array_equal(bt[ok].get_autocorr_time(tol=tol, on_device=True), tau[ok])
    with pytest.raises(autocorr.AutocorrError, match="member %d\\." % flagged[0]):
        bt[flagged[0]].get_autocorr_time(tol=tol, on_device=True)


def test_growing_chain_across_powers_of_two():
    bt = sampled("iso_32x5_stretch", 100, seed=8)
    for more in (27, 1, 1, 126, 1, 300):                 # stored 127, 128, 129, 255, 256, 556
        bt.run_mcmc(None, more)
        assert_matches_host(bt, 0, 1)
        assert_matches_host(bt, 10, 3)
    bt.close()


def test_throughput_1024_members():
    """1 024 members of 32 x 5 with 2 000 stored steps: one device call for all members is faster than the host path for 16"""
    B, N, D = 1024, 32, 5
    rs = np.random.RandomState(12)
    bt = EnsembleBatch(B, N, D, targets.IsoGaussian(), seeds=list(range(B)))
    bt.run_mcmc(rs.randn(B, N, D), 2000, skip_initial_state_check=True)
    bt.get_autocorr_time(quiet=True, on_device=True)      # plans and scratch
    t0 = time.perf_counter()
    dev = bt.get_autocorr_time(quiet=True, on_device=True)
    t_dev = time.perf_counter() - t0
    t0 = time.perf_counter()
    host = np.stack([bt[b].get_autocorr_time(quiet=True) for b in range(16)])
    t_host = time.perf_counter() - t0
    np.testing.assert_allclose(dev[:16], host, rtol=1e-8)
    assert t_dev < t_host, (t_dev, t_host)
    bt.close()
