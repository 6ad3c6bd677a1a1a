"""EnsembleSampler.get_histograms / Backend.get_histograms without a GPU: the C ABI of emx_chain_minmax / emx_histograms, the host
path (a Backend filled with save_step is counted with NumPy into the same Histograms tuple the device path returns) against
np.histogram / np.histogram2d, count for count, and the argument checks that must fire before any device is touched."""
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


def test_header_declares_and_library_exports_the_two_calls():
    assert declared_types("emx_chain_minmax") == ["emx_ctx*", "int32_t", "int64_t", "int64_t", "int64_t", "double*", "double*", "int64_t*"]
    assert declared_types("emx_histograms") == [
        "emx_ctx*", "int32_t", "int64_t", "int64_t", "int64_t", "const int64_t*", "const double*", "int64_t*", "const int64_t*",
        "const double*", "int64_t", "const int32_t*", "const int64_t*", "int64_t*", "int64_t*"]
    lib = _lib.load()
    for name, nargs in (("emx_chain_minmax", 8), ("emx_histograms", 15)):
        assert hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.C.c_int and len(args) == nargs
    assert hasattr(device.DeviceEnsemble, "chain_minmax") and hasattr(device.DeviceEnsemble, "histograms")
    assert os.path.exists(os.path.join(ROOT, "emcee_amd", "csrc", "emx_hist.hpp"))
    from emcee_amd import _build
    assert os.path.join(ROOT, "emcee_amd", "csrc", "emx_hist.hpp") in _build.DEPS


def filled_backend(blobs=None, seed=0, plant=None):
    """a host Backend of STEPS steps of values rounded to one decimal (ties); plant(t, x) may edit a step's coordinates"""
    rs = np.random.RandomState(seed)
    b = Backend()
    b.reset(N, D)
    first = None if blobs is None else blobs(rs, 0)
    b.grow(STEPS, first)
    for t in range(STEPS):
        lp = rs.randn(N)
        x = np.round(rs.randn(N, D), 1)
        if plant:
            plant(t, x)
        b.save_step(State(x, log_prob=lp, blobs=None if blobs is None else blobs(rs, t)), np.ones(N, dtype=bool))
    return b


def check_host(x, h, bins=None, rng=None, pairs="all", pair_bins=None):
    """h against np.histogram / np.histogram2d on the (n, W) samples x.  bins / pair_bins: what NumPy is given per column -- an
    int (with the ranges `rng` (W, 2) or None) or a list of W edge arrays."""
    n, W = x.shape
    assert isinstance(h, summary.Histograms) and h.nsamples == n
    assert len(h.edges) == len(h.counts) == len(h.pair_edges) == W
    for d in range(W):
        b = bins if isinstance(bins, int) else bins[d]
        r = None if rng is None or not isinstance(bins, int) else tuple(rng[d])
        c, e = np.histogram(x[:, d], bins=b, range=r)
        assert h.counts[d].dtype == np.int64 and h.edges[d].dtype == np.float64
        assert np.array_equal(h.edges[d], e), d
        assert np.array_equal(h.counts[d], c), d
    want = [(i, j) for i in np.arange(W) for j in np.arange(i + 1, W)] if isinstance(pairs, str) else list(pairs or ())
    assert h.pairs.shape == (len(want), 2) and h.pairs.tolist() == [list(map(int, p)) for p in want]
    assert len(h.pair_counts) == len(want)
    for d in range(W):
        if isinstance(pair_bins, int):
            r = None if rng is None else tuple(rng[d])
            assert np.array_equal(h.pair_edges[d], np.histogram_bin_edges(x[:, d], bins=pair_bins, range=r)), d
        else:
            assert np.array_equal(h.pair_edges[d], pair_bins[d]), d
    for (i, j), pc in zip(want, h.pair_counts):
        c, ex, ey = np.histogram2d(x[:, i], x[:, j], bins=[h.pair_edges[i], h.pair_edges[j]])
        assert pc.dtype == np.int64 and pc.shape == c.shape
        assert np.array_equal(pc, c), (i, j)


@pytest.mark.parametrize("discard,thin", [(0, 1), (5, 3), (40, 1)])
def test_host_backend_histograms_equal_numpy(discard, thin):
    b = filled_backend()
    x = b.get_chain(flat=True, discard=discard, thin=thin)
    assert len(x) == len(range(discard + thin - 1, STEPS, thin)) * N
    kw = dict(discard=discard, thin=thin)
    # integer bins, the range from the data: the max lands in the closed last bin
    for bins in (1, 7, 64):
        h = b.get_histograms(bins=bins, **kw)
        check_host(x, h, bins=bins, pair_bins=min(bins, 64))
        assert all(c.sum() == len(x) for c in h.counts) and all(c.sum() == len(x) for c in h.pair_counts)
    check_host(x, b.get_histograms(bins=200, pair_bins=5, **kw), bins=200, pair_bins=5)
    # an explicit range that leaves samples outside: one for all columns, and one a column
    r = np.array([[-1.0, 0.5]] * D)
    h = b.get_histograms(bins=10, range=(-1.0, 0.5), **kw)
    check_host(x, h, bins=10, rng=r, pair_bins=10)
    assert all(c.sum() < len(x) for c in h.counts)
    r = np.array([[-1.0, 0.5], [0.0, 3.0], [-0.3, 0.3]])
    check_host(x, b.get_histograms(bins=9, range=r, pair_bins=4, **kw), bins=9, rng=r, pair_bins=4)
    # non-uniform edges whose interior edges are stored values: one array for all columns, one a column, and for the panels
    vals = np.unique(x)
    e = np.concatenate([[vals[0] - 1.0], vals[::3][:12], [vals[-1] + 0.25]])
    e = np.unique(e)
    check_host(x, b.get_histograms(bins=e, **kw), bins=[e] * D, pair_bins=[e] * D)
    per = [np.unique(x[:, d])[::(2 + d)] for d in range(D)]
    per = [p if len(p) > 1 else np.array([p[0], p[0] + 1.0]) for p in per]
    check_host(x, b.get_histograms(bins=per, **kw), bins=per, pair_bins=per)
    check_host(x, b.get_histograms(bins=16, pair_bins=per, **kw), bins=16, pair_bins=per)
    # pairs: all, none, a list (both orders of a pair are panels of their own)
    h = b.get_histograms(bins=8, pairs=None, **kw)
    check_host(x, h, bins=8, pairs=None, pair_bins=8)
    assert h.pairs.shape == (0, 2) and h.pair_counts == []
    check_host(x, b.get_histograms(bins=8, pairs=(), **kw), bins=8, pairs=None, pair_bins=8)
    lst = [(2, 0), (0, 2), (1, 2)]
    h = b.get_histograms(bins=8, pairs=lst, pair_bins=6, **kw)
    check_host(x, h, bins=8, pairs=lst, pair_bins=6)
    assert np.array_equal(h.pair_counts[0], h.pair_counts[1].T)


def test_a_constant_column_widens_by_a_half():
    def plant(t, x):
        x[:, 1] = 2.5
    b = filled_backend(plant=plant)
    x = b.get_chain(flat=True)
    h = b.get_histograms(bins=4)
    assert np.array_equal(h.edges[1], np.linspace(2.0, 3.0, 5)) and h.counts[1].tolist() == [0, 0, len(x), 0]
    check_host(x, h, bins=4, pair_bins=4)
    h = b.get_histograms(bins=4, range=(2.5, 2.5), pairs=None)
    assert all(np.array_equal(e, np.linspace(2.0, 3.0, 5)) for e in h.edges)
    check_host(x, h, bins=4, rng=[(2.5, 2.5)] * D, pairs=None, pair_bins=4)


def test_nan_raises_with_the_range_from_the_data_and_is_not_counted_with_a_range():
    def plant(t, x):
        if t == 11:
            x[3, 2] = np.nan
        if t == 12:
            x[4, 2] = np.inf
    b = filled_backend(plant=plant)
    with pytest.raises(ValueError, match=r"column\(s\) \[2\] is not finite"):
        b.get_histograms(bins=8)
    x = b.get_chain(flat=True)
    r = [(-4.0, 4.0)] * D
    h = b.get_histograms(bins=8, range=(-4.0, 4.0))
    check_host(x, h, bins=8, rng=r, pair_bins=8)
    assert h.counts[2].sum() == len(x) - 2 and h.counts[0].sum() == len(x)
    assert h.pair_counts[1].sum() == len(x) - 2          # the pair (0, 2)
    e = np.array([-5.0, -1.0, 0.0, 0.1, 2.0, 6.0])
    check_host(x, b.get_histograms(bins=e), bins=[e] * D, pair_bins=[e] * D)


def test_host_blob_histograms():
    for blobs, K in ((lambda rs, t: np.round(rs.randn(N), 1), 1), (lambda rs, t: np.round(rs.randn(N, 2), 1), 2)):
        b = filled_backend(blobs)
        x = b.get_blobs(flat=True, discard=5, thin=3)
        x = x.reshape(len(x), -1)
        h = b.get_blob_histograms(bins=12, discard=5, thin=3)
        check_host(x, h, bins=12, pair_bins=12)
        assert len(h.counts) == K and len(h.pair_counts) == K * (K - 1) // 2
    dt = np.dtype([("a", float), ("b", int)])
    with pytest.raises(TypeError, match="plain float blobs"):
        filled_backend(lambda rs, t: np.zeros(N, dtype=dt)).get_blob_histograms()
    with pytest.raises(ValueError, match="no blobs"):
        filled_backend().get_blob_histograms()


@pytest.fixture
def no_device(monkeypatch):
    """any attempt to load the library or to create a context fails the test"""
    def refuse(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(device.DeviceEnsemble, "__init__", refuse)
    monkeypatch.setattr(device.DeviceEnsemble, "histograms", refuse)
    monkeypatch.setattr(device.DeviceEnsemble, "chain_minmax", refuse)


def bad_argument_cases(get, W):
    for bins in (0, 1025, -3):
        with pytest.raises(ValueError, match="bins must be between 1 and 1024"):
            get(bins=bins)
    with pytest.raises(ValueError, match="pair_bins must be between 1 and 128"):
        get(pair_bins=129)
    with pytest.raises(ValueError, match="pair_bins must be between 1 and 128"):
        get(pair_bins=0)
    for e in ([0.0, 1.0, 1.0, 2.0], [0.0, 2.0, 1.0], [0.0, np.nan, 1.0]):
        with pytest.raises(ValueError, match="strictly increasing"):
            get(bins=e)
        with pytest.raises(ValueError, match="strictly increasing"):
            get(pair_bins=e)
    with pytest.raises(ValueError, match="at least 2"):
        get(bins=[1.0])
    with pytest.raises(ValueError, match="at most 128 bins"):
        get(pair_bins=np.arange(130.0))
    with pytest.raises(TypeError, match="integer or bin edges"):
        get(bins=2.5)
    for pairs in ([(1, 1)], [(0, 1), (0, 0)]):
        with pytest.raises(ValueError, match="two different columns"):
            get(pairs=pairs)
    with pytest.raises(ValueError, match="counted from 0"):
        get(pairs=[(0, -1)])
    with pytest.raises(ValueError, match="pairs is"):
        get(pairs="every")
    with pytest.raises(ValueError, match="pairs is"):
        get(pairs=[(0, 1, 2)])
    with pytest.raises(ValueError, match="lo <= hi"):
        get(range=(1.0, 0.0))
    with pytest.raises(ValueError, match="range"):
        get(range=(0.0, 1.0, 2.0))
    with pytest.raises(ValueError, match="finite"):
        get(range=(0.0, np.inf))
    for thin in (0, -1, 1.5):
        with pytest.raises(ValueError, match="thin"):
            get(thin=thin)
    for discard in (-1, 0.5):
        with pytest.raises(ValueError, match="discard"):
            get(discard=discard)
    if W:
        for pairs in ([(0, W)], [(W + 2, 0)]):
            with pytest.raises(ValueError, match="outside the %d columns" % W):
                get(pairs=pairs)
        with pytest.raises(ValueError, match="every one of the %d columns" % W):
            get(bins=[np.arange(3.0)] * (W + 1))
        with pytest.raises(ValueError, match="every one of the %d columns" % W):
            get(range=np.zeros((W + 1, 2)))


def test_bad_arguments_before_any_device(no_device):
    from emcee_amd import targets
    s = EnsembleSampler(16, 2, targets.IsoGaussian())
    bad_argument_cases(s.get_histograms, 2)
    bad_argument_cases(s.get_blob_histograms, 0)
    with pytest.raises(AttributeError, match="run the sampler"):
        s.get_histograms()
    bad_argument_cases(Backend().get_histograms, 0)
    b = filled_backend()
    bad_argument_cases(b.get_histograms, D)
    for discard in (STEPS, STEPS + 3):
        with pytest.raises(ValueError, match="select none"):
            b.get_histograms(discard=discard)
    # more than 128 bins given as edges serve the marginals alone
    e = np.linspace(-4, 4, 201)
    with pytest.raises(ValueError, match="at most 128 bins"):
        b.get_histograms(bins=e)
    h = b.get_histograms(bins=e, pairs=None)
    assert h.counts[0].sum() == STEPS * N
    h = b.get_histograms(bins=e, pair_bins=3)
    assert h.pair_counts[0].shape == (3, 3)
