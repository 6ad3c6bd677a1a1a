"""The adaptive ladder without a GPU: the host twin of the update (emx_host_pt_adapt_ladder) against a NumPy transcription of
ptemcee's rule, the argument checks, and thermodynamic integration over one ladder per object."""
import numpy as np
import pytest

from emcee_amd import PTSampler, _lib, targets
from emcee_amd.pt import thermodynamic_integration_log_evidence

LIKE = targets.BatchCallable(lambda q: -0.5 * (q * q).sum(-1))


def ptemcee_adjustment(time, betas0, ratios, adaptation_lag, adaptation_time):
    """ptemcee 1.0's Sampler._get_ladder_adjustment, transcribed: -> the change of the ladder"""
    betas = betas0.copy()
    decay = adaptation_lag / (time + adaptation_lag)
    kappa = decay / adaptation_time
    dSs = kappa * (ratios[:-1] - ratios[1:])
    deltaTs = np.diff(1 / betas[:-1])
    deltaTs *= np.exp(dSs)
    betas[1:-1] = 1 / (np.cumsum(deltaTs) + 1 / betas[0])
    return betas - betas0


def host_adapt(betas, accepts, N, lag, time, t):
    betas = np.ascontiguousarray(betas, dtype=np.float64)
    out = np.full_like(betas, np.nan)
    acc = np.ascontiguousarray(accepts, dtype=np.int64)
    if acc.size == 0:
        acc = np.zeros(1, dtype=np.int64)
    assert _lib.load().emx_host_pt_adapt_ladder(betas, acc, len(betas), N, lag, time, t, out) == 0
    return out


def random_ladder(rs, T, last0):
    b = np.sort(rs.uniform(1e-4, 1.0, size=T - 1))[::-1]
    b = np.concatenate([[1.0], b[:T - 2], [0.0] if last0 else b[T - 2:]])
    return b


@pytest.mark.parametrize("T", [3, 4, 5, 8, 16, 40, 256])
@pytest.mark.parametrize("last0", [False, True])
def test_host_twin_matches_ptemcee(T, last0):
    rs = np.random.RandomState(T * 2 + last0)
    for _ in range(40):
        N = int(rs.randint(2, 2000))
        b = random_ladder(rs, T, last0)
        acc = rs.randint(0, N + 1, size=T - 1)
        lag = float(rs.choice([1.0, 10.0, 1e4])) * rs.uniform(0.5, 2.0)
        time = rs.uniform(1.0, 300.0)
        t = int(rs.randint(0, 10 ** 6))
        out = host_adapt(b, acc, N, lag, time, t)
        want = b + ptemcee_adjustment(t, b, acc / float(N), lag, time)
        np.testing.assert_allclose(out, want, rtol=1e-14, atol=0)
        assert out[0] == b[0] and out[-1] == b[-1]                  # the ends never move
        assert np.all(np.diff(out) < 0) and np.all(out[:-1] > 0)


def test_few_rungs_do_not_move():
    rs = np.random.RandomState(1)
    for T, b in ((1, np.ones(1)), (2, np.array([1.0, 0.3])), (2, np.array([1.0, 0.0]))):
        out = host_adapt(b, rs.randint(0, 10, size=T - 1), 10, 5.0, 2.0, 3)
        assert np.array_equal(out, b)


def test_rates_move_the_ladder_the_documented_way():
    # a pair that accepts more than its hotter neighbour widens in temperature; equal rates leave the ladder as it is
    b = np.array([1.0, 0.5, 0.25, 0.125, 0.0])
    assert np.array_equal(host_adapt(b, [8, 8, 8, 8], 10, 10.0, 1.0, 0), b)
    out = host_adapt(b, [10, 0, 5, 5], 10, 10.0, 1.0, 0)
    assert 1 / out[1] - 1 / out[0] > 1 / b[1] - 1 / b[0]
    assert 1 / out[2] - 1 / out[1] < 1 / b[2] - 1 / b[1]


def test_large_rate_differences_stay_finite():
    # kappa far above ptemcee's: exp of +-100 and +-1000 (no libm on either side; host == device by construction).  The new
    # betas are stored as computed, so a rung far below its old value keeps its digits where ptemcee's b + (b' - b) rounds to 0.
    b = np.array([1.0, 0.5, 0.25, 1e-3])
    for time in (1e-2, 1e-3):
        out = host_adapt(b, [100, 0, 100], 100, 1.0, time, 0)
        dS = (1.0 / time) * np.array([1.0, -1.0])
        with np.errstate(over="ignore"):
            want = 1 / (np.cumsum(np.diff(1 / b[:-1]) * np.exp(dS)) + 1.0)      # exp(1000) overflows to inf: beta 0
        np.testing.assert_allclose(out[1:-1], want, rtol=1e-13, atol=0)
        assert out[0] == 1.0 and out[-1] == 1e-3
    assert out[1] == 0.0 and out[2] == 0.0


def test_host_twin_refuses_bad_arguments():
    lib = _lib.load()
    b, acc, out = np.array([1.0, 0.5, 0.1]), np.array([1, 2], dtype=np.int64), np.zeros(3)
    for lag, time in ((0.0, 1.0), (-1.0, 1.0), (1.0, 0.0), (1.0, -2.0), (np.inf, 1.0), (1.0, np.nan), (np.nan, 1.0)):
        assert lib.emx_host_pt_adapt_ladder(b, acc, 3, 10, lag, time, 0, out) == -1
    assert lib.emx_host_pt_adapt_ladder(b, acc, 3, 0, 1.0, 1.0, 0, out) == -1
    assert lib.emx_host_pt_adapt_ladder(b, acc, 3, 10, 1.0, 1.0, -1, out) == -1


# ---------------------------------------------------------------------------------------------------------------- arguments
@pytest.mark.parametrize("kw, match", [
    (dict(adaptation_lag=0), "adaptation_lag"),
    (dict(adaptation_lag=-5), "adaptation_lag"),
    (dict(adaptation_lag=np.inf), "adaptation_lag"),
    (dict(adaptation_time=0), "adaptation_time"),
    (dict(adaptation_time=-1.0), "adaptation_time"),
    (dict(adaptation_time=np.nan), "adaptation_time"),
])
def test_adaptation_constants_are_checked(kw, match):
    with pytest.raises(ValueError, match=match):
        PTSampler(3, 16, 2, LIKE, adaptive=True, **kw)


def test_too_many_rungs_for_an_adaptive_ladder():
    with pytest.raises(ValueError, match="at most 256"):
        PTSampler(257, 16, 2, LIKE, adaptive=True)
    s = PTSampler(257, 16, 2, LIKE)          # a fixed ladder has no such limit
    assert s.ntemps == 257 and not s.adaptive
    PTSampler(256, 16, 2, LIKE, adaptive=True)


def test_defaults_and_the_ladder_before_a_run():
    s = PTSampler(4, 16, 2, LIKE, nbatch=3, Tmax=50.0, adaptive=True)
    assert (s.adaptation_lag, s.adaptation_time) == (10000.0, 100.0)
    assert s.adaptation_updates == 0
    assert s.ladder.shape == (3, 4) and np.array_equal(s.ladder, np.tile(s.betas, (3, 1)))
    assert not PTSampler(4, 16, 2, LIKE).adaptive


# ---------------------------------------------------------------------------------------------------------------- integration
def test_one_ladder_per_row_broadcasts():
    rs = np.random.RandomState(3)
    G, T = 5, 6
    lad = np.stack([random_ladder(rs, T, g % 2 == 0) for g in range(G)])     # rows ending at 0 and above 0
    logls = rs.randn(G, T) - 3.0
    logz, dlogz = thermodynamic_integration_log_evidence(lad, logls)
    assert logz.shape == (G,) and dlogz.shape == (G,)
    for g in range(G):
        z1, d1 = thermodynamic_integration_log_evidence(lad[g], logls[g])
        assert logz[g] == z1 and dlogz[g] == d1
    # one shared ladder as a 1-D array or repeated per row: the same bits
    b = random_ladder(rs, T, False)
    one = thermodynamic_integration_log_evidence(b, logls)
    rows = thermodynamic_integration_log_evidence(np.tile(b, (G, 1)), logls)
    assert np.array_equal(one[0], rows[0]) and np.array_equal(one[1], rows[1])
    # (G, 1, T) ladders against (G, K, T) means; (G, T) ladders against (T,) means
    many = rs.randn(G, 3, T)
    z3, _ = thermodynamic_integration_log_evidence(lad[:, None, :], many)
    assert z3.shape == (G, 3)
    for g in range(G):
        for k in range(3):
            assert z3[g, k] == thermodynamic_integration_log_evidence(lad[g], many[g, k])[0]
    zs, _ = thermodynamic_integration_log_evidence(lad, logls[0])
    assert zs.shape == (G,) and zs[1] == thermodynamic_integration_log_evidence(lad[1], logls[0])[0]
