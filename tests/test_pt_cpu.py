"""PTSampler without a GPU: argument checks, the default ladders, the host twin of the swap draws and the NumPy thermodynamic
integration."""
import ctypes as C

import numpy as np
import pytest

from emcee_amd import PTSampler, _lib, moves, targets
from emcee_amd.pt import default_betas, thermodynamic_integration_log_evidence

LIKE = targets.BatchCallable(lambda q: -0.5 * (q * q).sum(-1))


# ---------------------------------------------------------------------------------------------------------------- arguments
@pytest.mark.parametrize("betas, match", [
    ([1.0, 0.5, 0.7], "decreasing"),
    ([1.0, 0.5, 0.5], "decreasing"),
    ([0.9, 0.5, 0.1], "betas\\[0\\]"),
    ([1.0, 0.5, -0.1], ">= 0"),
])
def test_bad_ladders_are_refused(betas, match):
    with pytest.raises(ValueError, match=match):
        PTSampler(3, 16, 2, LIKE, betas=betas)


def test_ladder_length_must_match_ntemps():
    with pytest.raises(ValueError, match="ntemps"):
        PTSampler(4, 16, 2, LIKE, betas=[1.0, 0.5, 0.25])


def test_shapes_and_rng_are_checked():
    with pytest.raises(ValueError, match="philox"):
        PTSampler(2, 16, 2, LIKE, rng="mt19937")
    with pytest.raises(ValueError, match="positive"):
        PTSampler(0, 16, 2, LIKE)
    with pytest.raises(ValueError, match="seeds"):
        PTSampler(2, 16, 2, LIKE, nbatch=3, seeds=[1, 2])
    with pytest.raises(ValueError, match="box"):
        PTSampler(2, 16, 2, LIKE, log_prior=(np.zeros(3), np.ones(3)))
    with pytest.raises(ValueError, match="swap_every"):
        PTSampler(2, 16, 2, LIKE, swap_every=-1)
    with pytest.raises(ValueError):
        PTSampler(2, 16, 2, LIKE, moves=moves.WalkMove())


def test_run_mcmc_checks_the_state_shape_before_any_device():
    s = PTSampler(2, 16, 2, LIKE, nbatch=2, seeds=[1, 2])
    with pytest.raises(ValueError, match="nbatch, ntemps, nwalkers, ndim"):
        s.run_mcmc(np.zeros((2, 16, 2)), 1)
    p0 = np.random.RandomState(0).randn(2, 2, 16, 2)
    p0[1, 1, 3, 0] = np.nan
    with pytest.raises(ValueError, match="object 1, rung 1"):
        s.run_mcmc(p0, 1)
    with pytest.raises(ValueError, match="never been called"):
        s.run_mcmc(None, 1)


def test_a_fused_target_is_refused_as_the_likelihood():
    with pytest.raises(TypeError, match="BatchCallable"):
        PTSampler(2, 16, 2, targets.IsoGaussian())
    with pytest.raises(TypeError, match="BatchCallable"):
        PTSampler(2, 16, 2, lambda x: -0.5 * np.sum(x * x))


def test_the_evidence_needs_a_normalised_prior():
    s = PTSampler(2, 16, 2, LIKE)
    with pytest.raises(ValueError, match="improper"):
        s.log_evidence_estimate()


def test_member_seeds_follow_the_documented_rule():
    s = PTSampler(3, 16, 2, LIKE, nbatch=2, seeds=[11, 12])
    for g, seed in enumerate([11, 12]):
        want = np.random.RandomState(seed).randint(0, 2 ** 32, size=3, dtype=np.uint64)
        assert np.array_equal(s.member_seeds[g], want)
    assert [int(v) for v in s._b.seeds] == [int(v) for v in s.member_seeds.reshape(-1)]


# ---------------------------------------------------------------------------------------------------------------- ladders
def test_default_ladders():
    ratio = 1.0 + np.sqrt(2.0 / 5)
    b = default_betas(6, 5)
    assert np.allclose(b, ratio ** -np.arange(6)) and b[0] == 1.0
    b = default_betas(6, 5, Tmax=1e3)
    assert np.allclose(b, np.geomspace(1, 1e-3, 6)) and b[0] == 1.0
    b = default_betas(6, 5, Tmax=np.inf)
    assert b[-1] == 0.0 and np.allclose(b[:-1], ratio ** -np.arange(5))
    assert np.array_equal(default_betas(1, 5), [1.0])
    s = PTSampler(4, 16, 2, LIKE, Tmax=10.0)
    assert np.allclose(s.betas, np.geomspace(1, 0.1, 4))
    with pytest.raises(ValueError, match="Tmax"):
        default_betas(4, 2, Tmax=0.5)


# ---------------------------------------------------------------------------------------------------------------- swap draws
def swap_draws(seed, step, N, T):
    perm = np.zeros((T - 1, N), dtype=np.int32)
    logu = np.zeros((T - 1, N))
    assert _lib.load().emx_host_pt_swap_draws(seed, step, N, T, perm, logu) == 0
    return perm, logu


def test_swap_draws_are_deterministic_and_bijective():
    for N in (2, 33, 100, 4096):
        p, u = swap_draws(0x1234567890ABCDEF, 7, N, 5)
        p2, u2 = swap_draws(0x1234567890ABCDEF, 7, N, 5)
        assert np.array_equal(p, p2) and np.array_equal(u, u2)
        for row in p:
            assert np.array_equal(np.sort(row), np.arange(N))
        assert np.all(u <= 0) and np.all(np.isfinite(u) | (u == -np.inf))
    p3, u3 = swap_draws(0x1234567890ABCDEF, 8, 100, 5)
    p4, _ = swap_draws(0x1234567890ABCDEF, 7, 100, 5)
    assert not np.array_equal(p3, p4) and not np.array_equal(u3, swap_draws(0x1234567890ABCDEF, 7, 100, 5)[1])
    assert not np.array_equal(p4[0], p4[1])             # every pair its own pairing


def test_swap_draws_match_plan_log_of_u53():
    """log u is the plan logarithm of a uniform: the distribution of exp(logu) is U[0, 1)"""
    _, u = swap_draws(99, 3, 4096, 3)
    e = np.exp(u.reshape(-1))
    assert 0.45 < e.mean() < 0.55 and e.min() >= 0 and e.max() < 1


def test_swap_pairing_is_not_the_split_permutation():
    lib = _lib.load()
    desc = _lib.MoveDesc(_lib.MOVE_STRETCH, 1, 0, 0, 2.0, 0.0, 0.0, 0.0)
    for N in (33, 100, 4096):
        off = np.zeros(2, dtype=np.int32)
        order = np.zeros(N, dtype=np.int32)
        p0, p1, p2 = (np.zeros(N, dtype=np.int32) for _ in range(3))
        s0, ua = np.zeros(N), np.zeros(N)
        seed, step = 0xDEADBEEF12345, 11
        assert lib.emx_host_plan_philox(seed, step, N, C.byref(desc), off, order, p0, p1, p2, s0, ua) == 0
        assert np.array_equal(np.sort(order), np.arange(N))
        perm, _ = swap_draws(seed, step, N, 2)
        assert not np.array_equal(perm[0], order)
        assert not np.array_equal(perm[0], np.argsort(order))


def test_swap_draws_refuse_bad_arguments():
    lib = _lib.load()
    assert lib.emx_host_pt_swap_draws(1, 0, 0, 2, np.zeros(1, dtype=np.int32), np.zeros(1)) == -1


# ---------------------------------------------------------------------------------------------------------------- evidence
def test_thermodynamic_integration_by_hand():
    betas = np.array([1.0, 0.5, 0.25, 0.0])
    logls = np.array([-1.0, -2.0, -4.0, -10.0])
    # trapezoids over [0, 0.25], [0.25, 0.5], [0.5, 1]
    want = 0.25 * (-10 - 4) / 2 + 0.25 * (-4 - 2) / 2 + 0.5 * (-2 - 1) / 2
    # every other rung: betas (1, 0.25, 0) with the beta-0 mean
    want2 = 0.25 * (-10 - 4) / 2 + 0.75 * (-4 - 1) / 2
    z, dz = thermodynamic_integration_log_evidence(betas, logls)
    assert np.isclose(z, want) and np.isclose(dz, abs(want - want2))


def test_thermodynamic_integration_appends_beta_zero():
    betas = np.array([1.0, 0.5, 0.2])
    logls = np.array([[-1.0, -3.0, -5.0], [0.0, 0.0, 0.0]])
    # appended rung: beta 0 with the hottest mean
    want = 0.2 * (-5 - 5) / 2 + 0.3 * (-5 - 3) / 2 + 0.5 * (-3 - 1) / 2
    want2 = 0.2 * (-5 - 5) / 2 + 0.8 * (-5 - 1) / 2       # betas (1, 0.2, 0)
    z, dz = thermodynamic_integration_log_evidence(betas, logls)
    assert z.shape == (2,) and np.isclose(z[0], want) and np.isclose(dz[0], abs(want - want2))
    assert z[1] == 0 and dz[1] == 0
