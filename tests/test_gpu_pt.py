"""PTSampler on the GPU: without swaps every rung is bit for bit the EnsembleBatch member of the tempered callable; the swap pass
is bit for bit a NumPy oracle fed by emx_host_pt_swap_draws; runs compose step by step; stored rows are post-swap; the sampler
hops between modes and estimates the evidence; launches, NaN and exceptions behave as documented."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from emcee_amd import EnsembleBatch, PTSampler, _lib, moves  # noqa: E402
from emcee_amd.pt import thermodynamic_integration_log_evidence  # noqa: E402
from emcee_amd.targets import BatchCallable  # noqa: E402

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- helpers
def gauss_fn(mu, ivar):
    """(B, n, D) -> (B, n): per-member diagonal Gaussian, element-wise in a fixed loop over the coordinates (row-independent)"""
    mu_t = torch.as_tensor(mu, device="cuda")[:, None, :]
    iv_t = torch.as_tensor(ivar, device="cuda")[:, None, :]
    D = mu.shape[1]

    def fn(q):
        acc = torch.zeros(q.shape[:2], dtype=torch.float64, device=q.device)
        for d in range(D):
            r = q[:, :, d] - mu_t[:, :, d]
            acc = acc + iv_t[:, :, d] * r * r
        return -0.5 * acc
    return fn


def box_fn(lo, hi):
    lo_t, hi_t = torch.as_tensor(lo, device="cuda"), torch.as_tensor(hi, device="cuda")

    def fn(q):
        inside = ((q >= lo_t) & (q <= hi_t)).all(-1)
        return torch.where(inside, torch.zeros((), dtype=torch.float64, device=q.device),
                           torch.full((), -np.inf, dtype=torch.float64, device=q.device))
    return fn


def pt_view(fn, G, T):
    """a (B, n, D) function as PTSampler's (G, T, n, D) -> (G, T, n)"""
    return lambda q: fn(q.reshape(G * T, q.shape[2], q.shape[3])).reshape(G, T, q.shape[2])


def tempered(beta, L, P):
    with np.errstate(invalid="ignore"):
        out = beta * L + P
    out = np.where(beta == 0, P, out)
    return np.where(P == -np.inf, -np.inf, out)


def draws(seed, step, N, T):
    perm = np.zeros((T - 1, N), dtype=np.int32)
    logu = np.zeros((T - 1, N))
    assert _lib.load().emx_host_pt_swap_draws(int(seed), int(step), N, T, perm, logu) == 0
    return perm, logu


def swap_oracle(X, L, P, betas, seeds, step):
    """ptemcee's swap pass on (G, T, N, ...) arrays with the library's draws; -> (X, L, P, lp, accepts (G, T - 1))"""
    X, L, P = X.copy(), L.copy(), P.copy()
    G, T, N = L.shape
    acc = np.zeros((G, T - 1), dtype=np.uint64)
    for g in range(G):
        perm, logu = draws(seeds[g], step, N, T)
        for i in range(T - 1, 0, -1):
            j = perm[i - 1]
            with np.errstate(invalid="ignore"):
                ok = (betas[i - 1] - betas[i]) * (L[g, i] - L[g, i - 1, j]) > logu[i - 1]
            k = np.flatnonzero(ok)
            jk = j[k]
            for A in (X, L, P):
                hot, cold = A[g, i, k].copy(), A[g, i - 1, jk].copy()
                A[g, i, k], A[g, i - 1, jk] = cold, hot
            acc[g, i - 1] = len(k)
    lp = tempered(betas[None, :, None], L, P)
    return X, L, P, lp, acc


def group_seeds(s):
    """each group's rung-0 Philox seed (the key of its swap draws)"""
    return [int(s._b._philox[g * s.ntemps]) for g in range(s.nbatch)]


def start(rs, G, T, N, D, scale=1.0, centre=0.0):
    return centre + scale * rs.randn(G, T, N, D)


# ---------------------------------------------------------------------------------------------------------------- no swaps
@pytest.mark.parametrize("mv", ["stretch", "de_snooker"])
def test_without_swaps_every_rung_is_the_batch_member_of_its_tempered_callable(mv):
    G, T, N, D, nsteps = 3, 4, 32, 3, 40
    rs = np.random.RandomState(5)
    mu, ivar = 0.2 * rs.randn(G * T, D), 1.0 / (0.3 + rs.rand(G * T, D))
    lo, hi = -2.0 * np.ones(D), 2.0 * np.ones(D)
    betas = np.array([1.0, 0.5, 0.1, 0.0])
    fn, prior = gauss_fn(mu, ivar), box_fn(lo, hi)
    mfac = (lambda: moves.StretchMove()) if mv == "stretch" else (lambda: [(moves.DEMove(), 0.8), (moves.DESnookerMove(), 0.2)])
    pt = PTSampler(T, N, D, BatchCallable(pt_view(fn, G, T)), log_prior=(lo, hi), betas=betas, nbatch=G, moves=mfac(),
                   seeds=[7, 8, 9], swap_every=0)
    p0 = start(rs, G, T, N, D, scale=0.3)
    pt.run_mcmc(p0, nsteps)
    bt = torch.as_tensor(np.tile(betas, G), device="cuda")[:, None]
    eb = EnsembleBatch(G * T, N, D, BatchCallable(lambda q: bt * fn(q) + prior(q)), moves=mfac(), seeds=pt.member_seeds.reshape(-1))
    eb.run_mcmc(p0.reshape(G * T, N, D), nsteps)
    last, ref = pt.get_last_sample(), eb.get_last_sample()
    assert np.array_equal(last.coords.reshape(G * T, N, D), ref.coords)
    assert np.array_equal(last.log_prob.reshape(G * T, N), ref.log_prob)
    assert np.array_equal(pt.get_chain().reshape(G * T, nsteps, N, D), eb.get_chain())
    assert np.array_equal(pt.get_log_prob().reshape(G * T, nsteps, N), eb.get_log_prob())
    assert np.array_equal(pt.acceptance_fraction.reshape(G * T, N), eb.acceptance_fraction)
    chain = pt.get_chain().reshape(G * T, nsteps * N, D)
    want = fn(torch.as_tensor(chain, device="cuda")).cpu().numpy().reshape(G, T, nsteps, N)
    assert np.array_equal(pt.get_log_likelihood(), want)
    assert np.all(pt.tswap_acceptance_fraction == 0)


# ---------------------------------------------------------------------------------------------------------------- swap pass
@pytest.mark.parametrize("T, N", [(2, 32), (5, 100), (16, 1024)])
def test_swap_pass_matches_the_numpy_oracle(T, N):
    G, D = 3, 2
    rs = np.random.RandomState(T * 1000 + N)
    lo, hi = -3.0 * np.ones(D), 3.0 * np.ones(D)
    betas = np.concatenate([np.geomspace(1.0, 0.05, T - 1), [0.0]])
    fn = gauss_fn(np.zeros((G * T, D)), np.ones((G * T, D)))
    s = PTSampler(T, N, D, BatchCallable(pt_view(fn, G, T)), log_prior=(lo, hi), betas=betas, nbatch=G, seeds=[1, 2, 3],
                  swap_every=0)
    s.run_mcmc(start(rs, G, T, N, D), 1, skip_initial_state_check=True)
    X = rs.uniform(-4, 4, size=(G, T, N, D))
    P = np.where(((X >= lo) & (X <= hi)).all(-1), 0.0, -np.inf)
    L = np.where(P == 0, -0.5 * (X * X).sum(-1) + rs.randn(G, T, N), -np.inf)
    L[:, :, ::7] = -np.inf                              # rows with L = -inf inside the box too
    s._set_pt_state(X.reshape(G * T, N, D), L.reshape(G * T, N), P.reshape(G * T, N))
    before = s._swap_counts()
    s._swap()
    wX, wL, wP, wlp, wacc = swap_oracle(X, L, P, betas, group_seeds(s), s._b._step - 1)
    got = s.get_last_sample()
    gL, gP = s._pt_state()
    assert np.array_equal(got.coords, wX)
    assert np.array_equal(gL, wL) and np.array_equal(gP, wP)
    assert np.array_equal(got.log_prob, wlp)
    att, acc = s._swap_counts()
    assert np.array_equal(att - before[0], np.full((G, T - 1), N, dtype=np.uint64))
    assert np.array_equal(acc - before[1], wacc)
    assert wacc.sum() > 0
    # the pass preserves each group's multiset of (x, L) rows
    for g in range(G):
        a = np.concatenate([X[g].reshape(-1, D), L[g].reshape(-1, 1)], axis=1)
        b = np.concatenate([got.coords[g].reshape(-1, D), gL[g].reshape(-1, 1)], axis=1)
        assert np.array_equal(a[np.lexsort(a.T[::-1])], b[np.lexsort(b.T[::-1])])


def test_equal_adjacent_betas_accept_every_swap():
    G, T, N, D = 2, 4, 64, 2
    rs = np.random.RandomState(3)
    fn = gauss_fn(np.zeros((G * T, D)), np.ones((G * T, D)))
    s = PTSampler(T, N, D, BatchCallable(pt_view(fn, G, T)), nbatch=G, seeds=[4, 5], swap_every=0)
    s.run_mcmc(start(rs, G, T, N, D), 1, store=False)
    lib = _lib.load()
    assert lib.emx_pt_set_tempering(s._h, T, np.full(T, 1.0), None, None) == 0
    X = rs.randn(G, T, N, D)
    s._set_pt_state(X.reshape(G * T, N, D), rs.randn(G * T, N) - 3.0, np.zeros((G * T, N)))
    s._swap()
    att, acc = s._swap_counts()
    assert np.array_equal(att, acc) and att.min() == N


# ---------------------------------------------------------------------------------------------------------------- composition
def _make(G, T, N, D, swap_every, seeds=(21, 22)):
    rs = np.random.RandomState(17)
    mu, ivar = 0.5 * rs.randn(G * T, D), 1.0 / (0.3 + rs.rand(G * T, D))
    fn = gauss_fn(mu, ivar)
    s = PTSampler(T, N, D, BatchCallable(pt_view(fn, G, T)), log_prior=(-5 * np.ones(D), 5 * np.ones(D)), Tmax=20.0, nbatch=G,
                  seeds=list(seeds), swap_every=swap_every)
    return s, start(np.random.RandomState(2), G, T, N, D, scale=0.5)


@pytest.mark.parametrize("thin_by, swap_every", [(1, 1), (2, 3)])
def test_runs_compose_step_by_step(thin_by, swap_every):
    G, T, N, D, n = 2, 5, 32, 3, 12
    a, p0 = _make(G, T, N, D, swap_every)
    a.run_mcmc(p0, n, thin_by=thin_by)
    # n thin_by single steps without swaps, each followed by emx_pt_swap on the cadence
    b, _ = _make(G, T, N, D, 0)
    for k in range(n * thin_by):
        b.run_mcmc(p0 if k == 0 else None, 1)
        if (k + 1) % swap_every == 0:
            b._swap()
    la, lb = a.get_last_sample(), b.get_last_sample()
    assert np.array_equal(la.coords, lb.coords) and np.array_equal(la.log_prob, lb.log_prob)
    assert all(np.array_equal(u, v) for u, v in zip(a._pt_state(), b._pt_state()))
    assert all(np.array_equal(u, v) for u, v in zip(a._swap_counts(), b._swap_counts()))
    assert a._swap_counts()[1].sum() > 0
    if thin_by == 1:
        assert np.array_equal(a.acceptance_fraction, b.acceptance_fraction)
    # stored rows are post-swap: one stored step at a time reproduces the chain row by row
    c, _ = _make(G, T, N, D, swap_every)
    rows = []
    for k in range(n):
        st = c.run_mcmc(p0 if k == 0 else None, 1, thin_by=thin_by)
        rows.append((st.coords, st.log_prob, c._pt_state()[0]))
    ch, lp, ll = a.get_chain(), a.get_log_prob(), a.get_log_likelihood()
    for k, (x, l, L) in enumerate(rows):
        assert np.array_equal(ch[:, :, k], x) and np.array_equal(lp[:, :, k], l) and np.array_equal(ll[:, :, k], L), k
    assert np.array_equal(c.get_chain(), ch) and np.array_equal(c.get_log_likelihood(), ll)


# ---------------------------------------------------------------------------------------------------------------- statistics
def mixture_fn():
    m = 4.0
    s2 = 0.3 ** 2
    lw1, lw2 = np.log(0.25), np.log(0.75)
    norm = -np.log(2 * np.pi * s2)

    def fn(q):
        d1 = ((q + m) ** 2).sum(-1)
        d2 = ((q - m) ** 2).sum(-1)
        return torch.logaddexp(lw1 - 0.5 * d1 / s2, lw2 - 0.5 * d2 / s2) + norm
    return fn


def test_mode_hopping():
    N, D, nsteps, burn = 64, 2, 2000, 500
    box = (-10 * np.ones(D), 10 * np.ones(D))
    fn = mixture_fn()
    rs = np.random.RandomState(8)
    cold = PTSampler(1, N, D, BatchCallable(fn), log_prior=box, nbatch=1, seeds=[1])
    cold.run_mcmc(-4.0 + 0.3 * rs.randn(1, 1, N, D), 1000)
    assert (cold.get_chain()[0, 0, :, :, 0] > 0).mean() < 0.01
    G, T = 8, 16
    pt = PTSampler(T, N, D, BatchCallable(fn), log_prior=box, Tmax=1e3, nbatch=G, seeds=list(range(100, 108)))
    pt.run_mcmc(-4.0 + 0.3 * rs.randn(G, T, N, D), nsteps)
    frac = (pt.get_chain(discard=burn)[:, 0, :, :, 0] > 0).mean(axis=(1, 2))
    assert np.all(np.abs(frac - 0.75) < 0.05), frac
    assert np.all(pt.tswap_acceptance_fraction > 0.05)


def exact_mean_loglike(beta, a=10.0, D=2):
    from math import erf
    if beta == 0:
        return -D / 2 * np.log(2 * np.pi) - 0.5 * D * a * a / 3
    s = 1 / np.sqrt(beta)
    z = a / s
    phi = np.exp(-z * z / 2) / np.sqrt(2 * np.pi)
    ex2 = s * s * (1 - 2 * z * phi / erf(z / np.sqrt(2)))
    return -D / 2 * np.log(2 * np.pi) - 0.5 * D * ex2


def test_evidence_of_a_box_truncated_gaussian():
    G, T, N, D, nsteps = 4, 40, 32, 2, 2000
    fn = lambda q: -0.5 * (q * q).sum(-1) - np.log(2 * np.pi)  # noqa: E731
    pt = PTSampler(T, N, D, BatchCallable(fn), log_prior=(-10 * np.ones(D), 10 * np.ones(D)), Tmax=1e4, nbatch=G,
                   seeds=[31, 32, 33, 34])
    rs = np.random.RandomState(9)
    pt.run_mcmc(rs.uniform(-1, 1, size=(G, T, N, D)), nsteps)
    logz, dlogz = pt.log_evidence_estimate()
    exact, _ = thermodynamic_integration_log_evidence(pt.betas, np.array([exact_mean_loglike(b) for b in pt.betas]))
    mc = np.std(logz)
    assert np.all(np.abs(logz - exact) < max(0.05, 4 * mc)), (logz, exact, mc)
    assert np.all(np.abs(logz - (-2 * np.log(20))) < 0.2), logz
    dev = pt.mean_log_likelihood(int(0.1 * pt.iteration))
    host = pt.get_log_likelihood(discard=int(0.1 * pt.iteration)).mean(axis=(2, 3))
    assert np.allclose(dev, host, rtol=1e-12, atol=0)


# ---------------------------------------------------------------------------------------------------------------- plumbing
@pytest.mark.parametrize("G, T", [(4, 4), (64, 16)])
def test_launches_per_step(G, T):
    N, D = 32, 5
    fn = lambda q: -0.5 * (q * q).sum(-1)  # noqa: E731
    s = PTSampler(T, N, D, BatchCallable(fn), nbatch=G, seeds=list(range(G)))
    s.run_mcmc(np.random.RandomState(0).randn(G, T, N, D), 1)
    n0 = s.launch_info()["launches"]
    s.run_mcmc(None, 10)
    smax = 2
    assert s.launch_info()["launches"] - n0 <= 10 * (smax + 2)
    s.swap_every = 0
    n1 = s.launch_info()["launches"]
    s.run_mcmc(None, 10)
    assert s.launch_info()["launches"] - n1 <= 10 * smax + 1


def test_prior_callable_matches_the_box():
    G, T, N, D = 2, 3, 32, 2
    lo, hi = -1.5 * np.ones(D), 1.5 * np.ones(D)
    fn = gauss_fn(np.zeros((G * T, D)), np.ones((G * T, D)))
    p0 = start(np.random.RandomState(4), G, T, N, D, scale=0.3)
    a = PTSampler(T, N, D, BatchCallable(pt_view(fn, G, T)), log_prior=(lo, hi), Tmax=10.0, nbatch=G, seeds=[1, 2])
    b = PTSampler(T, N, D, BatchCallable(pt_view(fn, G, T)), log_prior=BatchCallable(pt_view(box_fn(lo, hi), G, T)), Tmax=10.0,
                  nbatch=G, seeds=[1, 2])
    a.run_mcmc(p0, 30)
    b.run_mcmc(p0, 30)
    assert np.array_equal(a.get_chain(), b.get_chain()) and np.array_equal(a.get_log_prob(), b.get_log_prob())
    assert np.array_equal(a.get_log_likelihood(), b.get_log_likelihood())


def test_nan_likelihood_names_object_and_rung():
    G, T, N, D = 2, 3, 32, 2
    flag = {"on": False}
    base = gauss_fn(np.zeros((G * T, D)), np.ones((G * T, D)))

    def fn(q):
        out = pt_view(base, G, T)(q)
        if flag["on"]:
            out = out.clone()
            out[1, 2] = float("nan")
        return out
    s = PTSampler(T, N, D, BatchCallable(fn), nbatch=G, seeds=[1, 2])
    s.run_mcmc(start(np.random.RandomState(1), G, T, N, D), 2)
    flag["on"] = True
    with pytest.raises(ValueError, match=r"object 1, rung 2\): Probability function returned NaN"):
        s.run_mcmc(None, 1)


def test_nan_likelihood_outside_the_prior_is_ignored():
    G, T, N, D = 2, 3, 32, 2
    lo, hi = -0.5 * np.ones(D), 0.5 * np.ones(D)

    def fn(q):
        out = -0.5 * (q * q).sum(-1)
        return torch.where((q.abs() > 0.5).any(-1), torch.full_like(out, float("nan")), out)
    s = PTSampler(T, N, D, BatchCallable(fn), log_prior=(lo, hi), nbatch=G, seeds=[1, 2])
    s.run_mcmc(np.random.RandomState(1).uniform(-0.4, 0.4, size=(G, T, N, D)), 20)
    assert np.all(np.isfinite(s.get_log_likelihood()))
    assert np.all(np.abs(s.get_chain()) <= 0.5)


def test_an_exception_in_the_callable_comes_out():
    G, T, N, D = 1, 2, 16, 2
    calls = {"n": 0}

    def fn(q):
        calls["n"] += 1
        if calls["n"] > 3:
            raise RuntimeError("boom in the likelihood")
        return -0.5 * (q * q).sum(-1)
    s = PTSampler(T, N, D, BatchCallable(fn), nbatch=G, seeds=[1])
    with pytest.raises(RuntimeError, match="boom in the likelihood"):
        s.run_mcmc(np.random.RandomState(0).randn(G, T, N, D), 5)


def test_autocorr_time_shape():
    G, T, N, D = 2, 3, 32, 2
    s = PTSampler(T, N, D, BatchCallable(lambda q: -0.5 * (q * q).sum(-1)), nbatch=G, seeds=[1, 2])
    s.run_mcmc(np.random.RandomState(0).randn(G, T, N, D), 200)
    tau = s.get_autocorr_time(quiet=True)
    assert tau.shape == (G, T, D) and np.all(np.isfinite(tau))
    host = s.get_autocorr_time(quiet=True, on_device=False)
    assert np.allclose(tau, host, rtol=1e-6)


def test_pt_rate_against_the_batch():
    """loose: the swap pass and its extra launch cost at most about half the callback batch's rate"""
    import time
    G, T, N, D, n = 64, 16, 32, 5, 60
    fn = lambda q: -0.5 * (q * q).sum(-1)  # noqa: E731
    p0 = np.random.RandomState(0).randn(G, T, N, D)
    pt = PTSampler(T, N, D, BatchCallable(fn), nbatch=G, seeds=list(range(G)))
    eb = EnsembleBatch(G * T, N, D, BatchCallable(lambda q: 0.5 * fn(q)), seeds=list(range(G * T)))
    pt.run_mcmc(p0, 10)
    eb.run_mcmc(p0.reshape(G * T, N, D), 10)

    def rate(f):
        best = 0.0
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            best = max(best, n / (time.perf_counter() - t0))
        return best
    r_pt = rate(lambda: pt.run_mcmc(None, n, store=False))
    r_eb = rate(lambda: eb.run_mcmc(None, n, store=False))
    assert r_pt >= 0.5 * r_eb, (r_pt, r_eb)
