"""EnsembleBatch without a GPU: the seed contract, the argument checks that must fire before any device is touched, and the
C ABI names of the batch handle."""
import os
import re

import numpy as np
import pytest

import emcee_amd
from emcee_amd import EnsembleBatch, EnsembleSampler, _lib, moves, targets
from emcee_amd.ensemble import philox_seed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    """any attempt to create the device handle fails the test"""
    def refuse(self):
        raise AssertionError("a device was touched before the arguments were checked")
    monkeypatch.setattr(EnsembleBatch, "_handle", refuse)


@pytest.mark.parametrize("seed", [0, 1, 42, 2 ** 31 - 1, 2 ** 32 - 1, 123456789])
def test_seed_helper_is_the_samplers(seed):
    s = EnsembleSampler(8, 2, targets.IsoGaussian(), rng="philox")
    s.random_state = np.random.RandomState(seed).get_state()
    assert philox_seed(np.random.RandomState(seed)) == s._philox_seed()
    assert philox_seed(np.random.RandomState(seed).get_state()) == s._philox_seed()


def test_member_seeds_follow_the_contract():
    b = EnsembleBatch(3, 16, 2, targets.IsoGaussian(), seeds=[7, 8, 9])
    assert [int(x) for x in b._philox] == [philox_seed(np.random.RandomState(s)) for s in (7, 8, 9)]
    np.random.seed(5)
    a = EnsembleBatch(4, 16, 2, targets.IsoGaussian())
    np.random.seed(5)
    c = EnsembleBatch(4, 16, 2, targets.IsoGaussian())
    assert a.seeds == c.seeds and len(set(a.seeds)) == 4


def test_exported_from_the_package():
    assert emcee_amd.EnsembleBatch is EnsembleBatch and "EnsembleBatch" in emcee_amd.__all__


def test_wrong_p0_shape(no_device):
    b = EnsembleBatch(3, 16, 2, targets.IsoGaussian(), seeds=[1, 2, 3])
    with pytest.raises(ValueError, match="incompatible input dimensions"):
        b.run_mcmc(np.zeros((2, 16, 2)), 10)
    with pytest.raises(ValueError, match="incompatible input dimensions"):
        b.run_mcmc(np.zeros((16, 2)), 10)
    with pytest.raises(ValueError, match="initial_state=None"):
        b.run_mcmc(None, 10)


def test_nan_member_named(no_device):
    b = EnsembleBatch(3, 16, 2, targets.IsoGaussian(), seeds=[1, 2, 3])
    p0 = np.random.RandomState(0).randn(3, 16, 2)
    p0[2, 3, 1] = np.nan
    with pytest.raises(ValueError, match="member 2: At least one parameter value was NaN"):
        b.run_mcmc(p0, 10)
    p0[2, 3, 1] = 0.0
    p0[1, :, 0] = 1.0       # degenerate walkers
    with pytest.raises(ValueError, match="member 1: Initial state has a large condition number"):
        b.run_mcmc(p0, 10)
    if np.dtype(np.longdouble).itemsize > 8:
        p0[1] = np.random.RandomState(1).randn(16, 2)
        with pytest.raises(TypeError, match="float64"):
            b.run_mcmc(p0.astype(np.longdouble), 10)


def test_mixed_targets(no_device):
    with pytest.raises(ValueError, match="one class"):
        EnsembleBatch(2, 16, 2, [targets.IsoGaussian(), targets.Rosenbrock()])
    with pytest.raises(ValueError, match="member 1"):
        EnsembleBatch(2, 16, 2, [targets.DiagGaussian(np.zeros(2), np.ones(2)), targets.DiagGaussian(np.zeros(3), np.ones(3))])
    with pytest.raises(ValueError, match="nbatch"):
        EnsembleBatch(3, 16, 2, [targets.IsoGaussian(), targets.IsoGaussian()])


def test_unsupported_targets(no_device):
    for t in (lambda x: -0.5 * np.sum(x ** 2), targets.DeviceCallable(lambda q: q), targets.DeviceKernel(0)):
        with pytest.raises(TypeError, match="EnsembleSampler"):
            EnsembleBatch(2, 16, 2, t)


def test_unsupported_moves_and_rng(no_device):
    for mv in (moves.WalkMove(), moves.KDEMove(), moves.GaussianMove(np.eye(2)),
               [moves.GaussianMove(0.5, mode="sequential"), moves.StretchMove()]):
        with pytest.raises(ValueError):
            EnsembleBatch(2, 16, 2, targets.IsoGaussian(), moves=mv)
    with pytest.raises(ValueError, match="philox"):
        EnsembleBatch(2, 16, 2, targets.IsoGaussian(), rng="mt19937")


def test_shapes_outside_one_workgroup(no_device):
    with pytest.raises(ValueError, match="one-workgroup"):
        EnsembleBatch(2, 8192, 2, targets.IsoGaussian())
    with pytest.raises(ValueError, match="one-workgroup"):
        EnsembleBatch(2, 16, 300, targets.IsoGaussian())
    with pytest.raises(ValueError, match="LDS"):
        EnsembleBatch(2, 2048, 16, targets.IsoGaussian())
    A = np.eye(64)
    with pytest.raises(ValueError, match="dense"):
        EnsembleBatch(2, 256, 64, targets.DenseGaussian(np.zeros(64), A))
    with pytest.raises(ValueError, match="complement"):
        EnsembleBatch(2, 3, 1, targets.IsoGaussian(), moves=moves.DEMove())


def test_header_declares_the_batch_abi():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "emx.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(emx_batch_[a-z0-9_]+)\s*\(", txt))
    want = {"emx_batch_check", "emx_batch_create", "emx_batch_destroy", "emx_batch_last_error", "emx_batch_set_tuning",
            "emx_batch_set_target", "emx_batch_set_moves", "emx_batch_set_move_scale", "emx_batch_get_move",
            "emx_batch_set_philox", "emx_batch_get_philox", "emx_batch_set_state", "emx_batch_get_state",
            "emx_batch_eval_state_log_prob", "emx_batch_chain_config", "emx_batch_run", "emx_batch_iteration",
            "emx_batch_chain_read", "emx_batch_accepted_counts", "emx_batch_status", "emx_batch_launch_info"}
    assert names == want, names ^ want
    lib = _lib.load()
    for n in want:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert '"batch_threads"' in open(os.path.join(ROOT, "include", "emx.h")).read()
