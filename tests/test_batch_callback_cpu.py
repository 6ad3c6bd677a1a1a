"""EnsembleBatch with the user's batched log-probability (targets.BatchCallable / BatchKernel) without a GPU: the argument checks
that must fire before any device is touched, the refusals, and the C ABI entry point."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from emcee_amd import EnsembleBatch, EnsembleSampler, _lib, moves, targets
from emcee_amd.targets import BatchCallable, BatchKernel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    """any attempt to create the device handle fails the test"""
    def refuse(self):
        raise AssertionError("a device was touched before the arguments were checked")
    monkeypatch.setattr(EnsembleBatch, "_handle", refuse)


def lp(q):
    return -0.5 * (q * q).sum(-1)


def test_exported_from_targets():
    assert "BatchCallable" in targets.__all__ and "BatchKernel" in targets.__all__


def test_construction_checks_arguments(no_device):
    b = EnsembleBatch(3, 16, 2, BatchCallable(lp), moves=[moves.DEMove(), moves.DESnookerMove()], seeds=[1, 2, 3])
    assert b.nbatch == 3 and b._targets[0].fn is lp
    EnsembleBatch(3, 16, 2, BatchKernel(0x1234), seeds=[1, 2, 3])
    EnsembleBatch(3, 16, 2, BatchKernel(C.c_void_p(0x1234), 7), seeds=[1, 2, 3])
    EnsembleBatch(2, 16, 2, BatchCallable(lp), moves=moves.GaussianMove(0.5))         # a Gaussian move as the only move
    with pytest.raises(TypeError, match="callable"):
        BatchCallable(3)
    for bad in (0, None, "f", True, C.c_void_p(0)):
        with pytest.raises(TypeError, match="BatchKernel"):
            BatchKernel(bad)
    with pytest.raises(ValueError, match="seeds"):
        EnsembleBatch(3, 16, 2, BatchCallable(lp), seeds=[1, 2])
    b = EnsembleBatch(3, 16, 2, BatchCallable(lp), seeds=[1, 2, 3])
    with pytest.raises(ValueError, match="incompatible input dimensions"):
        b.run_mcmc(np.zeros((2, 16, 2)), 10)
    p0 = np.random.RandomState(0).randn(3, 16, 2)
    p0[1, 4, 0] = np.inf
    with pytest.raises(ValueError, match="member 1: At least one parameter value was infinite"):
        b.run_mcmc(p0, 10)


def test_gaussian_move_mixed_with_red_blue_moves_is_refused(no_device):
    for mv in ([moves.GaussianMove(0.5), moves.StretchMove()], [(moves.DEMove(), 0.5), (moves.GaussianMove([0.1, 0.2]), 0.5)]):
        with pytest.raises(ValueError, match="GaussianMove runs only as the one move"):
            EnsembleBatch(2, 16, 2, BatchCallable(lp), moves=mv)


def test_refusals(no_device):
    with pytest.raises(ValueError, match="one-workgroup"):
        EnsembleBatch(2, 8192, 2, BatchCallable(lp))
    with pytest.raises(ValueError, match="one-workgroup"):
        EnsembleBatch(2, 16, 300, BatchKernel(0x1234))
    with pytest.raises(ValueError, match="philox"):
        EnsembleBatch(2, 16, 2, BatchCallable(lp), rng="mt19937")
    for mv in (moves.WalkMove(), moves.KDEMove(), moves.GaussianMove(np.eye(2))):
        with pytest.raises(ValueError):
            EnsembleBatch(2, 16, 2, BatchCallable(lp), moves=mv)
    with pytest.raises(TypeError, match="ONE BatchCallable"):
        EnsembleBatch(2, 16, 2, [BatchCallable(lp), BatchCallable(lp)])
    with pytest.raises(TypeError, match="ONE BatchCallable"):
        EnsembleBatch(2, 16, 2, [BatchKernel(0x1234), BatchKernel(0x1234)])
    # the single-ensemble callables keep pointing at EnsembleSampler
    for t in (targets.DeviceCallable(lambda q: q), targets.DeviceKernel(0)):
        with pytest.raises(TypeError, match="EnsembleSampler"):
            EnsembleBatch(2, 16, 2, t)


def test_larger_shapes_than_the_fused_lds_bound(no_device):
    """no member lives in LDS on this path: the fused kernel's LDS bound does not apply (the shape limits do)"""
    with pytest.raises(ValueError, match="LDS"):
        EnsembleBatch(2, 2048, 16, targets.IsoGaussian())
    EnsembleBatch(2, 2048, 16, BatchCallable(lp))
    EnsembleBatch(2, 4096, 256, BatchCallable(lp))


def test_ensemble_sampler_refuses_batch_targets():
    for t in (BatchCallable(lp), BatchKernel(0x1234)):
        with pytest.raises(TypeError, match="EnsembleBatch"):
            EnsembleSampler(16, 2, t, rng="philox")


def test_header_declares_and_library_exports_the_entry_point():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "emx.h")).read(), flags=re.S)
    assert re.search(r"\bemx_set_batch_target_callback\s*\(", txt)
    assert re.search(r"typedef\s+int\s*\(\s*\*\s*emx_batch_log_prob_fn\s*\)", txt)
    assert "emx_set_batch_target_callback" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["emx_set_batch_target_callback"]
    assert args[1] is _lib.BATCH_LOG_PROB_FN
    assert _lib.BATCH_LOG_PROB_FN._argtypes_ == (C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p)
    lib = _lib.load()
    assert hasattr(lib, "emx_set_batch_target_callback")


def _check(N, D, descs):
    lib = _lib.load()
    msg = C.create_string_buffer(256)
    arr = (_lib.MoveDesc * len(descs))(*descs)
    return lib.emx_batch_check(N, D, _lib.TARGET_CALLBACK, len(descs), arr, msg, 256), msg.value.decode()


def test_batch_check_takes_the_callback_kind():
    from emcee_amd.ensemble import _native_desc
    stretch = _native_desc(moves.StretchMove(), 5, True, False)
    snooker = _native_desc(moves.DESnookerMove(), 5, True, False)
    gauss = _native_desc(moves.GaussianMove(0.5), 5, True, False)
    assert _check(32, 5, [stretch]) == (0, "")
    assert _check(100, 10, [stretch, snooker]) == (0, "")
    assert _check(4096, 256, [gauss]) == (0, "")
    rc, why = _check(8192, 5, [stretch])
    assert rc == -1 and "nwalkers <= 4096" in why
    rc, why = _check(32, 5, [stretch, gauss])
    assert rc == -1 and "GaussianMove" in why
    rc, why = _check(32, 5, [_native_desc(moves.WalkMove(), 5, True, True)])
    assert rc == -1 and "StretchMove" in why
