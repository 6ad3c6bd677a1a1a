"""EnsembleSampler.get_summary / Backend.get_summary without a GPU: the C ABI of emx_summary, the host path (a Backend filled
with save_step reduces with NumPy into the same BatchSummary the device path returns) and the argument checks that must fire
before any device is touched."""
import os
import re

import numpy as np
import pytest

from emcee_amd import EnsembleSampler, State, _lib, device, summary
from emcee_amd.backends import Backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, STEPS = 24, 3, 41


def declared_types(name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "emx.h")).read(), flags=re.S)
    m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, txt)
    assert m, "include/emx.h does not declare %s" % name
    return [p.strip().rsplit(None, 1)[0].replace(" *", "*") for p in m.group(1).split(",")]


def test_header_declares_and_library_exports_emx_summary():
    assert declared_types("emx_summary") == [
        "emx_ctx*", "int32_t", "int64_t", "int64_t", "int64_t", "double*", "double*", "int32_t", "const int64_t*", "double*", "double*",
        "double*", "int64_t*"]
    lib = _lib.load()
    assert hasattr(lib, "emx_summary")
    res, args = _lib.SIGNATURES["emx_summary"]
    assert res is _lib.C.c_int and len(args) == 13
    from emcee_amd import _build
    assert len(_build.SRCS) == 17
    assert hasattr(device.DeviceEnsemble, "summary")


def filled_backend(blobs=None, seed=0):
    """a host Backend of STEPS steps; the largest log-prob is planted twice: at (step 7, walker 5) and at (step 7, walker 9)"""
    rs = np.random.RandomState(seed)
    b = Backend()
    b.reset(N, D)
    first = None if blobs is None else blobs(rs, 0)
    b.grow(STEPS, first)
    for t in range(STEPS):
        lp = rs.randn(N)
        if t == 7:
            lp[5] = lp[9] = 50.0
        if t == 30:
            lp[2] = 50.0
        x = np.round(rs.randn(N, D), 1)                   # ties
        b.save_step(State(x, log_prob=lp, blobs=None if blobs is None else blobs(rs, t)), np.ones(N, dtype=bool))
    return b


def check_host(b, discard, thin, get, value):
    x = value(flat=True, discard=discard, thin=thin)
    x = x.reshape(len(x), -1)
    lp = b.get_log_prob(flat=True, discard=discard, thin=thin)
    q = (0.16, 0.5, 0.84)
    s = get(discard=discard, thin=thin, quantiles=q)
    assert isinstance(s, summary.BatchSummary) and s.nsamples == len(x)
    np.testing.assert_allclose(s.mean, x.mean(axis=0), rtol=1e-13, atol=0)
    np.testing.assert_allclose(s.cov, np.atleast_2d(np.cov(x.T)), rtol=1e-13, atol=0)
    assert s.cov.shape == (x.shape[1], x.shape[1])
    assert np.array_equal(s.quantiles, np.quantile(x, q, axis=0)) and s.quantiles.shape == (3, x.shape[1])
    at = int(np.argmax(lp))
    assert s.map_log_prob == lp[at] and np.array_equal(s.map_coords, x[at])
    nocov = get(discard=discard, thin=thin, cov=False)
    assert nocov.cov is None and np.array_equal(nocov.mean, s.mean) and np.array_equal(nocov.quantiles, s.quantiles)
    noq = get(discard=discard, thin=thin, quantiles=())
    assert noq.quantiles.shape == (0, x.shape[1]) and np.array_equal(noq.cov, s.cov) and np.array_equal(noq.map_coords, s.map_coords)
    return s, at


@pytest.mark.parametrize("discard,thin", [(0, 1), (5, 3), (40, 1)])
def test_host_backend_summary_equals_numpy(discard, thin):
    b = filled_backend()
    s, at = check_host(b, discard, thin, b.get_summary, b.get_chain)
    if (discard, thin) == (0, 1):
        assert at == 7 * N + 5                            # the first of the three planted maxima
        assert s.map_log_prob == 50.0
    if (discard, thin) == (5, 3):
        assert at == 0 * N + 5                            # rows 7, 10, ...: step 7 is the selection's first row
    assert s.nsamples == len(range(discard + thin - 1, STEPS, thin)) * N


def test_host_blob_summary():
    for blobs, K in ((lambda rs, t: rs.randn(N), 1), (lambda rs, t: rs.randn(N, 2), 2)):
        b = filled_backend(blobs)
        s, _ = check_host(b, 5, 3, b.get_blob_summary, b.get_blobs)
        assert s.mean.shape == (K,) and s.map_coords.shape == (K,)
    dt = np.dtype([("a", float), ("b", int)])
    b = filled_backend(lambda rs, t: np.zeros(N, dtype=dt))
    with pytest.raises(TypeError, match="plain float blobs"):
        b.get_blob_summary()
    b = filled_backend(lambda rs, t: np.array([{"t": t}] * N, dtype=object))
    with pytest.raises(TypeError, match="plain float blobs"):
        b.get_blob_summary()
    with pytest.raises(ValueError, match="no blobs"):
        filled_backend().get_blob_summary()


@pytest.fixture
def no_device(monkeypatch):
    """any attempt to load the library or to create a context fails the test"""
    def refuse(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(device.DeviceEnsemble, "__init__", refuse)
    monkeypatch.setattr(device.DeviceEnsemble, "summary", refuse)


def bad_argument_cases(get, stored):
    if not stored:
        with pytest.raises(AttributeError, match="run the sampler"):
            get()
    for thin in (0, -1, 1.5):
        with pytest.raises(ValueError, match="thin"):
            get(thin=thin)
    for discard in (-1, 0.5):
        with pytest.raises(ValueError, match="discard"):
            get(discard=discard)
    for q in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match="quantile"):
            get(quantiles=(0.5, q))
    with pytest.raises(ValueError, match="at most 16"):
        get(quantiles=np.linspace(0, 1, 17))
    if stored:
        for discard in (stored, stored + 3):
            with pytest.raises(ValueError, match="select none"):
                get(discard=discard)
        with pytest.raises(ValueError, match="select none"):
            get(discard=stored - 2, thin=3)


def test_bad_arguments_before_any_device(no_device):
    from emcee_amd import targets
    s = EnsembleSampler(16, 2, targets.IsoGaussian())
    bad_argument_cases(s.get_summary, 0)
    bad_argument_cases(s.get_blob_summary, 0)
    empty = Backend()
    bad_argument_cases(empty.get_summary, 0)
    empty.reset(N, D)
    bad_argument_cases(empty.get_summary, 0)
    b = filled_backend()
    bad_argument_cases(b.get_summary, STEPS)
