"""PTSampler's adaptive ladder on the GPU: one adaptive swap pass is bit for bit the swap oracle followed by the host twin of the
update; runs compose step by step and resume through emx_pt_get_ladder / emx_pt_set_ladder; a frozen ladder stays put and the
evidence refuses a window that adapted; adaptation evens out the swap acceptance of a poor ladder; launches do not change."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from emcee_amd import PTSampler, _lib  # noqa: E402
from emcee_amd.pt import thermodynamic_integration_log_evidence  # noqa: E402
from emcee_amd.targets import BatchCallable  # noqa: E402

pytestmark = pytest.mark.gpu


def gauss_fn(mu, ivar):
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


def pt_view(fn, G, T):
    return lambda q: fn(q.reshape(G * T, q.shape[2], q.shape[3])).reshape(G, T, q.shape[2])


def tempered(beta, L, P):
    with np.errstate(invalid="ignore"):
        out = beta * L + P
    out = np.where(beta == 0, P, out)
    return np.where(P == -np.inf, -np.inf, out)


def swap_oracle(X, L, P, ladder, seeds, step):
    """ptemcee's swap pass with each group's own ladder (G, T) and the library's draws -> (X, L, P, accepts (G, T - 1))"""
    X, L, P = X.copy(), L.copy(), P.copy()
    G, T, N = L.shape
    acc = np.zeros((G, T - 1), dtype=np.int64)
    lib = _lib.load()
    for g in range(G):
        perm = np.zeros((T - 1, N), dtype=np.int32)
        logu = np.zeros((T - 1, N))
        assert lib.emx_host_pt_swap_draws(int(seeds[g]), int(step), N, T, perm, logu) == 0
        b = ladder[g]
        for i in range(T - 1, 0, -1):
            j = perm[i - 1]
            with np.errstate(invalid="ignore"):
                ok = (b[i - 1] - b[i]) * (L[g, i] - L[g, i - 1, j]) > logu[i - 1]
            k = np.flatnonzero(ok)
            jk = j[k]
            for A in (X, L, P):
                hot, cold = A[g, i, k].copy(), A[g, i - 1, jk].copy()
                A[g, i, k], A[g, i - 1, jk] = cold, hot
            acc[g, i - 1] = len(k)
    return X, L, P, acc


def host_adapt(b, acc, N, lag, time, t):
    out = np.empty_like(b)
    a = np.ascontiguousarray(acc, dtype=np.int64) if len(acc) else np.zeros(1, dtype=np.int64)
    assert _lib.load().emx_host_pt_adapt_ladder(np.ascontiguousarray(b), a, len(b), N, lag, time, int(t), out) == 0
    return out


def set_ladder(s, lad, updates):
    u = C.c_int64(int(updates))
    s._ck(_lib.load().emx_pt_set_ladder(s._h, np.ascontiguousarray(lad, dtype=np.float64), C.byref(u)))


def group_seeds(s):
    return [int(s._b._philox[g * s.ntemps]) for g in range(s.nbatch)]


# ---------------------------------------------------------------------------------------------------------------- oracle
@pytest.mark.parametrize("T, N, last", [(3, 32, 0.0), (5, 100, 0.0), (16, 1024, 0.0), (5, 100, 0.02)])
def test_adaptive_swap_pass_matches_the_oracle_and_the_host_twin(T, N, last):
    G, D = 3, 2
    lag, time, t0 = 7.0, 3.0, 11
    rs = np.random.RandomState(T * 1000 + N)
    lo, hi = -3.0 * np.ones(D), 3.0 * np.ones(D)
    betas = np.concatenate([np.geomspace(1.0, 0.05, T - 1), [last]])
    fn = gauss_fn(np.zeros((G * T, D)), np.ones((G * T, D)))
    s = PTSampler(T, N, D, BatchCallable(pt_view(fn, G, T)), log_prior=(lo, hi), betas=betas, nbatch=G, seeds=[1, 2, 3],
                  swap_every=0, adaptive=True, adaptation_lag=lag, adaptation_time=time)
    s.run_mcmc(rs.randn(G, T, N, D), 1, skip_initial_state_check=True)
    assert s.adaptation_updates == 0 and np.array_equal(s.ladder, np.tile(betas, (G, 1)))
    # every group on a ladder of its own, the counter at t0
    lad = np.tile(betas, (G, 1))
    for g in range(G):
        lad[g, 1:-1] = np.sort(rs.uniform(max(last, 1e-3), 1.0, size=T - 2))[::-1]
    set_ladder(s, lad, t0)
    assert np.array_equal(s.ladder, lad) and s.adaptation_updates == t0
    X = rs.uniform(-4, 4, size=(G, T, N, D))
    P = np.where(((X >= lo) & (X <= hi)).all(-1), 0.0, -np.inf)
    L = np.where(P == 0, -0.5 * (X * X).sum(-1) + rs.randn(G, T, N), -np.inf)
    L[:, :, ::7] = -np.inf
    s._set_pt_state(X.reshape(G * T, N, D), L.reshape(G * T, N), P.reshape(G * T, N))
    # emx_pt_set_state takes each member's current beta
    assert np.array_equal(s.get_last_sample().log_prob, tempered(lad[:, :, None], L, P))
    s._swap()
    wX, wL, wP, wacc = swap_oracle(X, L, P, lad, group_seeds(s), s._b._step - 1)
    wlad = np.stack([host_adapt(lad[g], wacc[g], N, lag, time, t0) for g in range(G)])
    got = s.get_last_sample()
    gL, gP = s._pt_state()
    assert np.array_equal(got.coords, wX)
    assert np.array_equal(gL, wL) and np.array_equal(gP, wP)
    assert np.array_equal(s.ladder, wlad)
    assert np.array_equal(got.log_prob, tempered(wlad[:, :, None], wL, wP))
    assert s.adaptation_updates == t0 + 1
    assert wacc.sum() > 0 and not np.array_equal(wlad, lad)
    assert np.array_equal(s.ladder[:, 0], lad[:, 0]) and np.array_equal(s.ladder[:, -1], lad[:, -1])


# ---------------------------------------------------------------------------------------------------------------- composition
def _make(G, T, N, D, swap_every, adaptive=True, seeds=(21, 22)):
    rs = np.random.RandomState(17)
    mu, ivar = 0.5 * rs.randn(G * T, D), 1.0 / (0.3 + rs.rand(G * T, D))
    fn = gauss_fn(mu, ivar)
    s = PTSampler(T, N, D, BatchCallable(pt_view(fn, G, T)), log_prior=(-5 * np.ones(D), 5 * np.ones(D)), Tmax=20.0, nbatch=G,
                  seeds=list(seeds), swap_every=swap_every, adaptive=adaptive, adaptation_lag=5, adaptation_time=2)
    return s, np.random.RandomState(2).randn(G, T, N, D) * 0.5


@pytest.mark.parametrize("thin_by, swap_every", [(1, 1), (2, 3)])
def test_adaptive_runs_compose_step_by_step(thin_by, swap_every):
    G, T, N, D, n = 2, 5, 32, 3, 12
    a, p0 = _make(G, T, N, D, swap_every)
    a.run_mcmc(p0, n, thin_by=thin_by)
    passes = (n * thin_by) // swap_every
    assert a.adaptation_updates == passes and not np.array_equal(a.ladder, np.tile(a.betas, (G, 1)))
    b, _ = _make(G, T, N, D, 0)
    for k in range(n * thin_by):
        b.run_mcmc(p0 if k == 0 else None, 1)
        if (k + 1) % swap_every == 0:
            b._swap()
    la, lb = a.get_last_sample(), b.get_last_sample()
    assert np.array_equal(la.coords, lb.coords) and np.array_equal(la.log_prob, lb.log_prob)
    assert all(np.array_equal(u, v) for u, v in zip(a._pt_state(), b._pt_state()))
    assert np.array_equal(a.ladder, b.ladder) and a.adaptation_updates == b.adaptation_updates
    assert all(np.array_equal(u, v) for u, v in zip(a._swap_counts(), b._swap_counts()))
    # one stored step at a time: the chain planes row by row, each row after the step's pass and update
    c, _ = _make(G, T, N, D, swap_every)
    rows = []
    for k in range(n):
        st = c.run_mcmc(p0 if k == 0 else None, 1, thin_by=thin_by)
        rows.append((st.coords, st.log_prob, c._pt_state()[0], c.ladder))
    ch, lp, ll, bt = a.get_chain(), a.get_log_prob(), a.get_log_likelihood(), a.get_betas()
    assert bt.shape == (G, n, T)
    for k, (x, l, L, lad) in enumerate(rows):
        assert np.array_equal(ch[:, :, k], x) and np.array_equal(lp[:, :, k], l) and np.array_equal(ll[:, :, k], L), k
        assert np.array_equal(bt[:, k], lad), k
    assert np.array_equal(c.get_chain(), ch) and np.array_equal(c.get_betas(), bt)
    assert np.array_equal(a.get_betas(discard=3, thin=2), bt[:, 4::2])
    # stop, disturb the ladder, put it back through emx_pt_set_ladder and resume: the same bits as one run
    d, _ = _make(G, T, N, D, swap_every)
    d.run_mcmc(p0, n // 2, thin_by=thin_by)
    saved, t = d.ladder, d.adaptation_updates
    set_ladder(d, np.tile(d.betas, (G, 1)), 0)
    set_ladder(d, saved, t)
    d.run_mcmc(None, n - n // 2, thin_by=thin_by)
    ld = d.get_last_sample()
    assert np.array_equal(ld.coords, la.coords) and np.array_equal(ld.log_prob, la.log_prob)
    assert np.array_equal(d.ladder, a.ladder) and d.adaptation_updates == a.adaptation_updates
    assert np.array_equal(d.get_betas(), bt) and np.array_equal(d.get_log_prob(), lp)


# ---------------------------------------------------------------------------------------------------------------- freeze
def test_freezing_keeps_the_ladder_and_the_evidence_needs_a_frozen_window():
    G, T, N, D = 2, 4, 32, 2
    fn = lambda q: -0.5 * (q * q).sum(-1) - np.log(2 * np.pi)  # noqa: E731
    s = PTSampler(T, N, D, BatchCallable(fn), log_prior=(-10 * np.ones(D), 10 * np.ones(D)), Tmax=100.0, nbatch=G,
                  seeds=[3, 4], adaptive=True, adaptation_lag=10, adaptation_time=5)
    s.run_mcmc(np.random.RandomState(0).uniform(-1, 1, size=(G, T, N, D)), 20)
    frozen, t = s.ladder, s.adaptation_updates
    assert t == 20 and not np.array_equal(frozen, np.tile(s.betas, (G, 1)))
    s.adaptive = False
    s.run_mcmc(None, 30)
    assert np.array_equal(s.ladder, frozen) and s.adaptation_updates == t
    bt = s.get_betas()
    assert np.array_equal(bt[:, 20:], np.broadcast_to(frozen[:, None], (G, 30, T)))
    assert np.array_equal(bt[:, 19], frozen) and not np.array_equal(bt[:, 0], frozen)
    with pytest.raises(ValueError, match="Freeze adaptation"):
        s.log_evidence_estimate(fburnin=0.1)
    logz, dlogz = s.log_evidence_estimate(fburnin=0.4)
    means = s.mean_log_likelihood(20)
    want = thermodynamic_integration_log_evidence(frozen, means)
    assert np.array_equal(logz, want[0]) and np.array_equal(dlogz, want[1])


# ---------------------------------------------------------------------------------------------------------------- statistics
def _pair_acceptance(s, steps):
    att0, acc0 = s._swap_counts()
    s.run_mcmc(None, steps)
    att, acc = s._swap_counts()
    return (acc - acc0) / (att - att0).astype(np.float64)


def exact_mean_loglike(beta, a=10.0, D=2):
    from math import erf
    if beta == 0:
        return -D / 2 * np.log(2 * np.pi) - 0.5 * D * a * a / 3
    s = 1 / np.sqrt(beta)
    z = a / s
    phi = np.exp(-z * z / 2) / np.sqrt(2 * np.pi)
    ex2 = s * s * (1 - 2 * z * phi / erf(z / np.sqrt(2)))
    return -D / 2 * np.log(2 * np.pi) - 0.5 * D * ex2


def test_adaptation_evens_out_swap_acceptance():
    G, T, N, D = 4, 8, 32, 2
    n_adapt, n_frozen = 1500, 1500
    fn = lambda q: -0.5 * (q * q).sum(-1) - np.log(2 * np.pi)  # noqa: E731
    box = (-10 * np.ones(D), 10 * np.ones(D))
    p0 = np.random.RandomState(9).uniform(-1, 1, size=(G, T, N, D))
    fixed = PTSampler(T, N, D, BatchCallable(fn), log_prior=box, Tmax=1e4, nbatch=G, seeds=[41, 42, 43, 44])
    fixed.run_mcmc(p0, n_adapt)
    before = _pair_acceptance(fixed, n_frozen)
    s = PTSampler(T, N, D, BatchCallable(fn), log_prior=box, Tmax=1e4, nbatch=G, seeds=[41, 42, 43, 44], adaptive=True,
                  adaptation_lag=1000, adaptation_time=10)
    s.run_mcmc(p0, n_adapt)
    s.adaptive = False
    after = _pair_acceptance(s, n_frozen)
    spread_before, spread_after = before.std(axis=1), after.std(axis=1)
    print("pair acceptance std before", spread_before, "after", spread_after)
    print("ladders", s.ladder)
    # first measured run (profiles/pt.md): std 0.240 ... 0.242 on the initial ladder, 0.0066 ... 0.0108 after adaptation
    assert np.all(spread_after < 0.2 * spread_before) and np.all(spread_after < 0.05), (spread_before, spread_after)
    lad = s.ladder
    assert len({tuple(r) for r in lad}) == G                        # each object ends on a ladder of its own
    assert np.all(lad[:, 0] == 1.0) and np.all(lad[:, -1] == s.betas[-1])
    # the evidence over the frozen, adapted ladder: the existing test's tolerance around each ladder's exact trapezoid value
    logz, _ = s.log_evidence_estimate(fburnin=(n_adapt + 100) / float(s.iteration))
    exact = np.array([thermodynamic_integration_log_evidence(r, np.array([exact_mean_loglike(b) for b in r]))[0] for r in lad])
    mc = np.std(logz - exact)
    print("logZ", logz, "exact trapezoid", exact, "analytic", -2 * np.log(20))
    assert np.all(np.abs(logz - exact) < max(0.05, 4 * mc)), (logz, exact, mc)


# ---------------------------------------------------------------------------------------------------------------- plumbing
@pytest.mark.parametrize("G, T", [(4, 4), (64, 16)])
def test_launches_per_step_do_not_change_with_adaptation(G, T):
    N, D = 32, 5
    fn = lambda q: -0.5 * (q * q).sum(-1)  # noqa: E731
    per = []
    for adaptive in (False, True):
        s = PTSampler(T, N, D, BatchCallable(fn), nbatch=G, seeds=list(range(G)), adaptive=adaptive)
        s.run_mcmc(np.random.RandomState(0).randn(G, T, N, D), 1)
        n0 = s.launch_info()["launches"]
        s.run_mcmc(None, 10)
        per.append(s.launch_info()["launches"] - n0)
        s.close()
    assert per[0] == per[1], per


def test_one_and_two_rungs_count_updates_without_moving():
    for T in (1, 2):
        s = PTSampler(T, 16, 2, BatchCallable(lambda q: -0.5 * (q * q).sum(-1)), nbatch=2, seeds=[1, 2], Tmax=10.0,
                      adaptive=True)
        s.run_mcmc(np.random.RandomState(0).randn(2, T, 16, 2), 5)
        assert s.adaptation_updates == 5
        assert np.array_equal(s.ladder, np.tile(s.betas, (2, 1)))
        assert np.array_equal(s.get_betas(), np.broadcast_to(s.betas, (2, 5, T)))
