"""WalkMove and KDEMove on the device in the Philox mode (csrc/emx_walkkde.hip): the host get_proposal is never called, the
proposal arithmetic equals NumPy / scipy's from the host twin's draws, the chains sample the target, and everything outside
the device scope keeps the host path."""
import ctypes as C

import numpy as np
import pytest
from scipy import stats
from scipy.stats import gaussian_kde

import emcee_amd
from emcee_amd import _lib, moves, targets
from emcee_amd.device import DeviceEnsemble

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE


def walk(s, nsplits=2):
    return _lib.MoveDesc(_lib.MOVE_WALK, nsplits, 1, 0 if s is None else s, 0.0, 0.0, 0.0, 0.0)


def kde(rule=0, a=0.0):
    return _lib.MoveDesc(_lib.MOVE_KDE, 2, 1, rule, a, 0.0, 0.0, 0.0)


def host_draws(md, N, D, split, step):
    S = md.nsplits
    ns = (N - split + S - 1) // S
    s = md.reserved if md.kind == _lib.MOVE_WALK else 0
    nh = s if s >= 2 else (1 if md.kind == _lib.MOVE_KDE else 0)
    nz = s if s >= 2 else D
    h = np.zeros(max(ns * nh, 1), dtype=np.int32)
    z = np.empty(ns * nz)
    assert _lib.load().emx_host_walk_kde_draws(SEED, step, N, D, C.byref(md), split, h.ctypes.data_as(C.c_void_p), z) == ns
    return h[:ns * nh].reshape(ns, nh), z.reshape(ns, nz)


def raising(monkeypatch):
    def boom(self, *a, **k):
        raise AssertionError("host get_proposal called")
    monkeypatch.setattr(moves.WalkMove, "get_proposal", boom)
    monkeypatch.setattr(moves.KDEMove, "get_proposal", boom)


MOVE_SETS = [lambda: moves.WalkMove(s=3), lambda: moves.WalkMove(), lambda: moves.KDEMove(),
             lambda: [(moves.WalkMove(s=3), 0.5), (moves.StretchMove(), 0.5)],
             lambda: [(moves.KDEMove(), 0.5), (moves.StretchMove(), 0.5)]]


@pytest.mark.parametrize("mv", MOVE_SETS)
def test_host_get_proposal_is_never_called_in_philox_mode(mv, monkeypatch):
    raising(monkeypatch)
    rs = np.random.RandomState(1)
    s = emcee_amd.EnsembleSampler(64, 4, targets.IsoGaussian(), moves=mv(), rng="philox")
    s.random_state = rs.get_state()
    s.run_mcmc(rs.randn(64, 4), 30)
    assert s.get_chain().shape == (30, 64, 4)
    assert np.all(np.isfinite(s.get_chain()))
    assert 0.05 < np.mean(s.acceptance_fraction) < 0.99


def _propose_once(N, D, md, step, x):
    ens = DeviceEnsemble(N, D)
    try:
        ens.set_target(_lib.TARGET_HOST)
        ens.set_moves([md], np.array([1.0]))
        ens.set_rng_mode(_lib.RNG_PHILOX)
        ens.set_philox(SEED, step)
        ens.set_state(x, np.zeros(N))
        _, nsplits = ens.step_begin(False)
        plan = ens.plan_get(nsplits)
        out = []
        for split in range(nsplits):
            q, f = ens.propose(split, with_factors=True)
            out.append((q.copy(), f.copy()))
            ens.accept(split, np.full(len(q), -np.inf))          # nothing moves: both splits see x
        ens.step_end()
        ens.raise_on_status()
        return plan, out
    finally:
        ens.close()


def _comp(plan, split):
    off, order = plan["off"], plan["order"]
    return np.concatenate([order[off[j]:off[j + 1]] for j in range(len(off) - 1) if j != split])


@pytest.mark.parametrize("N,D", [(512, 8), (4096, 64)])
@pytest.mark.parametrize("s", [2, 3, 8])
def test_walk_helpers_proposal_arithmetic(N, D, s):
    rs = np.random.RandomState(N + s)
    x = rs.randn(N, D) * (1 + np.arange(D))
    step = 3
    plan, out = _propose_once(N, D, walk(s), step, x)
    for split, (q, f) in enumerate(out):
        h, z = host_draws(walk(s), N, D, split, step)
        w = (z - z.mean(1, keepdims=True)) / np.sqrt(s - 1)
        members = plan["order"][plan["off"][split]:plan["off"][split + 1]]
        want = x[members] + np.einsum("tk,tkd->td", w, x[h])
        np.testing.assert_allclose(q, want, rtol=1e-12, atol=1e-12 * np.abs(x).max())
        assert np.all(f == 0)


@pytest.mark.parametrize("N,D", [(512, 8), (4096, 64)])
def test_walk_whole_complement_proposal_arithmetic(N, D):
    rs = np.random.RandomState(5)
    A = rs.randn(D, D) / np.sqrt(D) + np.eye(D)
    x = rs.randn(N, D) @ A.T
    step = 11
    plan, out = _propose_once(N, D, walk(None), step, x)
    for split, (q, f) in enumerate(out):
        _, z = host_draws(walk(None), N, D, split, step)
        L = np.linalg.cholesky(np.cov(x[_comp(plan, split)], rowvar=False))
        members = plan["order"][plan["off"][split]:plan["off"][split + 1]]
        np.testing.assert_allclose(q, x[members] + z @ L.T, rtol=1e-10, atol=1e-10)
        assert np.all(f == 0)


@pytest.mark.parametrize("N,D", [(512, 8), (4096, 64)])
@pytest.mark.parametrize("bw", [None, "silverman", 0.5])
def test_kde_proposal_and_factor_equal_scipy(N, D, bw):
    rs = np.random.RandomState(7)
    A = rs.randn(D, D) / np.sqrt(D) + np.eye(D)
    x = rs.randn(N, D) @ A.T + 0.3
    md = moves.KDEMove(bw_method=bw)._philox_desc(D)
    step = 2
    plan, out = _propose_once(N, D, md, step, x)
    for split, (q, f) in enumerate(out):
        h, z = host_draws(md, N, D, split, step)
        C_ = x[_comp(plan, split)]
        dens = gaussian_kde(C_.T, bw_method=bw)
        Lh = np.linalg.cholesky(dens.covariance)
        members = plan["order"][plan["off"][split]:plan["off"][split + 1]]
        np.testing.assert_allclose(q, x[h[:, 0]] + z @ Lh.T, rtol=1e-10, atol=1e-10)
        want = dens.logpdf(x[members].T) - dens.logpdf(q.T)
        np.testing.assert_allclose(f, want, rtol=0, atol=1e-8)


@pytest.mark.parametrize("mv,nsteps", [(lambda: moves.WalkMove(s=3), 1500), (lambda: moves.WalkMove(), 600),
                                       (lambda: moves.KDEMove(), 1500)])
def test_normal_target_statistics_philox(mv, nsteps):
    """test_normal_target_statistics_host_proposal_moves's bounds, device proposals."""
    np.random.seed(1234)
    nwalkers, ndim = 32, 2
    coords = np.random.randn(nwalkers, ndim)
    s = emcee_amd.EnsembleSampler(nwalkers, ndim, targets.IsoGaussian(), moves=mv(), rng="philox")
    s.run_mcmc(coords, nsteps)
    acc = s.acceptance_fraction
    assert np.all((acc < 0.95) * (acc > 0.1)), acc
    samps = s.get_chain(flat=True, discard=100)
    mu, sig = np.mean(samps, axis=0), np.std(samps, axis=0)
    assert np.all(np.abs(mu) < 0.08), mu
    assert np.all(np.abs(sig - 1) < 0.05), sig


def _dense8():
    rs = np.random.RandomState(3)
    A = rs.randn(8, 8)
    cov = A @ A.T / 8 + 0.5 * np.eye(8)
    mu = rs.randn(8)
    return mu, cov


@pytest.mark.parametrize("mv", [lambda: moves.WalkMove(s=8), lambda: moves.WalkMove(), lambda: moves.KDEMove()])
def test_dense_gaussian_moments_and_acceptance_match_the_host_path(mv):
    mu, cov = _dense8()
    N, D, nsteps = 4096, 8, 200
    rs = np.random.RandomState(9)
    p0 = mu + rs.randn(N, D) @ np.linalg.cholesky(cov).T
    s = emcee_amd.EnsembleSampler(N, D, targets.DenseGaussian(mu, np.linalg.inv(cov)), moves=mv(), rng="philox")
    s.run_mcmc(p0, nsteps)
    samps = s.get_chain(flat=True, discard=50)
    np.testing.assert_allclose(samps.mean(0), mu, atol=0.05)
    np.testing.assert_allclose(np.cov(samps, rowvar=False), cov, atol=0.08 * np.abs(cov).max())
    # the exact mode's host get_proposal from the same (stationary) start: a few steps of 4 096 walkers pin its acceptance
    h = emcee_amd.EnsembleSampler(N, D, targets.DenseGaussian(mu, np.linalg.inv(cov)), moves=mv())
    h.random_state = np.random.RandomState(2).get_state()
    h.run_mcmc(p0, 6)
    a_dev, a_host = np.mean(s.acceptance_fraction), np.mean(h.acceptance_fraction)
    assert abs(a_dev - a_host) < 0.02, (a_dev, a_host)


def _run(mv, p0, n, **kw):
    N, D = p0.shape
    s = emcee_amd.EnsembleSampler(N, D, targets.IsoGaussian(), moves=mv(), rng="philox")
    s.random_state = np.random.RandomState(8).get_state()
    st = s.run_mcmc(p0, n, **kw)
    return s, np.array(st.coords)


@pytest.mark.parametrize("mv", [lambda: moves.WalkMove(s=4), lambda: moves.WalkMove(), lambda: moves.KDEMove(),
                                lambda: [(moves.KDEMove(), 0.5), (moves.StretchMove(), 0.5)]])
def test_bit_identical_reruns_and_the_paths_agree(mv):
    N, D, n = 256, 5, 20
    p0 = np.random.RandomState(4).randn(N, D)
    a, ca = _run(mv, p0, n)
    b, cb = _run(mv, p0, n)
    assert np.array_equal(a.get_chain(), b.get_chain()) and np.array_equal(ca, cb)
    s = emcee_amd.EnsembleSampler(N, D, targets.IsoGaussian(), moves=mv(), rng="philox")
    s.random_state = np.random.RandomState(8).get_state()
    for _ in s.sample(p0, iterations=n):
        pass
    assert np.array_equal(s.get_chain(), a.get_chain())
    t, _ = _run(mv, p0, n // 2, thin_by=2)
    assert np.array_equal(t.get_chain(), a.get_chain()[1::2])
    _, cn = _run(mv, p0, n, store=False)
    assert np.array_equal(cn, ca)


@pytest.mark.parametrize("mv", [lambda: moves.WalkMove(s=4), lambda: moves.KDEMove()])
def test_python_log_prob_and_device_callable(mv):
    N, D, n = 512, 3, 300
    p0 = np.random.RandomState(6).randn(N, D)
    s = emcee_amd.EnsembleSampler(N, D, lambda x: -0.5 * np.sum(x ** 2), moves=mv(), rng="philox")
    s.run_mcmc(p0, n)
    samps = s.get_chain(flat=True, discard=50)
    assert np.all(np.abs(samps.mean(0)) < 0.08) and np.all(np.abs(samps.std(0) - 1) < 0.06)

    def lp(q):
        return -0.5 * (q * q).sum(1)
    c = emcee_amd.EnsembleSampler(N, D, targets.DeviceCallable(lp), moves=mv(), rng="philox")
    c.run_mcmc(p0, n)
    samps = c.get_chain(flat=True, discard=50)
    assert np.all(np.abs(samps.mean(0)) < 0.08) and np.all(np.abs(samps.std(0) - 1) < 0.06)


def test_kde_singular_complement_raises_linalg_error():
    N, D = 64, 3
    p0 = np.random.RandomState(2).randn(N, D)
    p0[:, 1] = 0.0
    s = emcee_amd.EnsembleSampler(N, D, targets.IsoGaussian(), moves=moves.KDEMove(), rng="philox")
    with pytest.raises(np.linalg.LinAlgError):
        s.run_mcmc(p0, 2, skip_initial_state_check=True)
    h = emcee_amd.EnsembleSampler(N, D, targets.IsoGaussian(), moves=moves.KDEMove())
    with pytest.raises(np.linalg.LinAlgError):
        h.run_mcmc(p0, 2, skip_initial_state_check=True)


class Called(Exception):
    pass


@pytest.mark.parametrize("case", ["mt19937", "callable_bw", "ndim130"])
def test_out_of_scope_inputs_keep_the_host_proposal(case, monkeypatch):
    def boom(self, *a, **k):
        raise Called()
    monkeypatch.setattr(moves.WalkMove, "get_proposal", boom)
    monkeypatch.setattr(moves.KDEMove, "get_proposal", boom)
    D = 130 if case == "ndim130" else 3
    N = 2 * D + 2
    mv = moves.KDEMove(bw_method=lambda k: 0.4) if case == "callable_bw" else moves.WalkMove(s=3)
    s = emcee_amd.EnsembleSampler(N, D, targets.IsoGaussian(), moves=mv, rng="mt19937" if case == "mt19937" else "philox")
    with pytest.raises(Called):
        s.run_mcmc(np.random.RandomState(1).randn(N, D), 2, skip_initial_state_check=True)


def test_c_abi_refusals():
    N, D = 64, 3
    ens = DeviceEnsemble(N, D)
    try:
        ens.set_target(_lib.TARGET_ISO)
        for bad in (walk(1), walk(N // 2 + 1)):
            with pytest.raises(Exception, match="s must be|larger sample"):
                ens.set_moves([bad], np.array([1.0]))
        ens.set_moves([walk(3)], np.array([1.0]))
        ens.set_state(np.random.RandomState(0).randn(N, D))
        ens.eval_state_log_prob()
        ens.set_rng_mode(_lib.RNG_MT19937)
        ens.set_mt19937(np.random.RandomState(0).get_state())
        ens.chain_config(2)
        with pytest.raises(Exception, match="Philox"):
            ens.run(1, 1, False)
        ens.set_moves([kde()], np.array([1.0]))
        with pytest.raises(Exception, match="Philox"):
            ens.step_begin(False)
        ens.set_rng_mode(_lib.RNG_INPUTS)
        ens.step_begin(False)
        with pytest.raises(Exception, match="Philox"):
            ens.plan_set(0, dict(off=np.array([0, 32, 64], np.int32), order=np.arange(N, dtype=np.int32),
                                 p0=np.arange(N, dtype=np.int32), p1=np.arange(N, dtype=np.int32),
                                 p2=np.arange(N, dtype=np.int32), s0=np.zeros(N), uacc=np.ones(N)))
    finally:
        ens.close()
