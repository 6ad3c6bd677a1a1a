"""EnsembleBatch.get_histograms without a GPU: the C ABI of emx_chain_minmax_batch / emx_histograms_batch, the argument checks
that must fire before any device is touched, the per-member edges (np.histogram_bin_edges, bit for bit) and the NumPy twin
summary.host_histograms_batch (np.histogram / np.histogram2d of every member, count for count)."""
import os
import re

import numpy as np
import pytest

from emcee_amd import EnsembleBatch, PTSampler, _lib, summary, targets
from emcee_amd.targets import BatchCallable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    """any attempt to create the device handle or to call the library fails the test"""
    def refuse(self):
        raise AssertionError("a device was touched before the arguments were checked")
    monkeypatch.setattr(EnsembleBatch, "_handle", refuse)
    monkeypatch.setattr(EnsembleBatch, "_lib", refuse)


def header_text():
    return open(os.path.join(ROOT, "include", "emx.h")).read()


def declared_types(name):
    txt = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, txt)
    assert m, "include/emx.h does not declare %s" % name
    return [p.strip().rsplit(None, 1)[0].replace(" *", "*") for p in m.group(1).split(",")]


def test_header_declares_and_library_exports_the_entry_points():
    assert declared_types("emx_chain_minmax_batch") == [
        "emx_batch*", "int32_t", "int32_t", "int32_t", "int64_t", "int64_t", "int64_t", "double*", "double*", "int64_t*"]
    assert declared_types("emx_histograms_batch") == [
        "emx_batch*", "int32_t", "int32_t", "int32_t", "int64_t", "int64_t", "int64_t", "const int64_t*", "const double*", "int64_t",
        "int64_t*", "const int64_t*", "const double*", "int64_t", "int64_t", "const int32_t*", "const int64_t*", "int64_t*", "int64_t*"]
    lib = _lib.load()
    for name, nargs in (("emx_chain_minmax_batch", 10), ("emx_histograms_batch", 19), ("emx_histograms_batch_info", 2)):
        assert hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.C.c_int and len(args) == nargs
    assert '"batch_hist_members"' in header_text()
    assert summary.BatchHistograms._fields == summary.Histograms._fields == (
        "nsamples", "edges", "counts", "pairs", "pair_edges", "pair_counts")


def bad_argument_cases(get, B, W, batch=True):
    for thin in (0, -1, 1.5):
        with pytest.raises(ValueError, match="thin"):
            get(thin=thin)
    for discard in (-1, 0.5):
        with pytest.raises(ValueError, match="discard"):
            get(discard=discard)
    for bins in (0, 1025, -3):
        with pytest.raises(ValueError, match="bins"):
            get(bins=bins)
    for bins in (2.5, True, "auto"):
        with pytest.raises(TypeError, match="bins"):
            get(bins=bins)
    with pytest.raises(ValueError, match="strictly increasing"):
        get(bins=[0.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="strictly increasing"):
        get(bins=[0.0, np.nan, 1.0])
    with pytest.raises(ValueError, match="one edge array for every one"):
        get(bins=[np.arange(3.0)] * (W + 1))
    with pytest.raises(ValueError, match="at most 1024"):
        get(bins=np.arange(1026.0))
    for rng in ((1.0, 0.0), (0.0, np.inf), (0.0, 1.0, 2.0), np.zeros((W + 1, 2)), np.zeros((W, 3))):
        with pytest.raises(ValueError, match="range"):
            get(range=rng)
    for pairs in ("some", [(0, 0)], [(0, -1)], [(0, W)], [(0, 1, 1)], [(0.5, 1)]):
        with pytest.raises(ValueError, match="pair"):
            get(pairs=pairs)
    for pb in (0, 129):
        with pytest.raises(ValueError, match="pair_bins"):
            get(pair_bins=pb)
    with pytest.raises(ValueError, match="pair panels have at most 128"):
        get(bins=np.arange(200.0))
    # the (B, W, 2) form
    for shape in ((B + 1, W, 2), (B, W + 1, 2), (B, W, 3)):
        with pytest.raises(ValueError, match="range"):
            get(range=np.zeros(shape) + np.arange(shape[2]))
    good = np.zeros((B, W, 2)) + [0.0, 1.0]
    if batch:
        bad = good.copy()
        bad[B - 1, 0] = [2.0, 1.0]
        with pytest.raises(ValueError, match=r"lo <= hi.*member\(s\) \[%d\]" % (B - 1)):
            get(range=bad)
        bad[B - 1, 0] = [np.nan, 1.0]
        with pytest.raises(ValueError, match="finite"):
            get(range=bad)
        # every argument is fine: the only thing missing is a stored chain -- get_summary's error
        for kw in (dict(range=good), dict(), dict(bins=[np.arange(4.0)] * W, pairs=[(1, 0)], pair_bins=128), dict(range=(0, 1), pairs=None)):
            with pytest.raises(ValueError, match="run the sampler"):
                get(**kw)
    else:
        with pytest.raises(ValueError, match="range"):
            get(range=good)                  # a member takes the single sampler's forms
        with pytest.raises(ValueError, match="run the sampler"):
            get(range=good[0])


def test_bad_arguments_before_any_device(no_device):
    bt = EnsembleBatch(3, 16, 2, targets.IsoGaussian(), seeds=[1, 2, 3])
    bad_argument_cases(bt.get_histograms, 3, 2)
    bad_argument_cases(bt[1].get_histograms, 3, 2, batch=False)
    for get in (bt.get_blob_histograms, bt[2].get_blob_histograms):
        with pytest.raises(ValueError, match="no blobs"):
            get()
    with pytest.raises(ValueError, match="members"):
        bt._histograms(0, 8, None, 0, 1, "all", None, 2, 2)
    with pytest.raises(ValueError, match="members"):
        bt._histograms(0, 8, None, 0, 1, "all", None, 0, 4)


def test_bad_arguments_before_any_device_ptsampler(no_device):
    pt = PTSampler(3, 16, 2, BatchCallable(lambda q: -0.5 * (q ** 2).sum(-1)), nbatch=2, seeds=[1, 2])
    bad_argument_cases(pt.get_histograms, 6, 2)
    with pytest.raises(ValueError, match="range"):
        pt.get_histograms(range=np.zeros((3, 2, 2, 2)) + [0.0, 1.0])
    with pytest.raises(ValueError, match="run the sampler"):
        pt.get_histograms(range=np.zeros((2, 3, 2, 2)) + [0.0, 1.0])


# --------------------------------------------------------------------------------------------------------------------- edges
def batch_samples():
    """(M, n, W) with ties, a constant column, scales from 1e-6 to 1e6 and a member of one sample"""
    rs = np.random.RandomState(5)
    M, n, W = 9, 400, 4
    x = rs.randn(M, n, W) * 10.0 ** rs.randint(-6, 7, size=(M, 1, W)) + rs.randn(M, 1, W)
    x[1] = np.round(x[1], 1)                       # ties
    x[2, :, 1] = -3.25                             # lo == hi
    x[3, :, 2] = 0.0
    x[4, 1:] = x[4, :1]                            # every sample equal
    return x


@pytest.mark.parametrize("bins", [1, 7, 64, 1024])
def test_member_edges_are_histogram_bin_edges_bit_for_bit(bins):
    x = batch_samples()
    M, _, W = x.shape
    edges = summary.member_edges(bins, None, M, W, (x.min(axis=1), x.max(axis=1)))
    assert len(edges) == W
    for d in range(W):
        assert edges[d].shape == (M, bins + 1) and edges[d].dtype == np.float64
        for m in range(M):
            ref = np.histogram_bin_edges(x[m, :, d], bins=bins)
            assert np.array_equal(edges[d][m], ref), (m, d)
            assert np.array_equal(edges[d][m], summary.column_edges(bins, None, W, (x[m].min(axis=0), x[m].max(axis=0)))[d])
    assert np.array_equal(edges[1][2], np.linspace(-3.75, -2.75, bins + 1))
    assert not summary.shared_edges(bins, None)


def test_member_edges_from_ranges_and_explicit_edges():
    M, W = 5, 3
    rs = np.random.RandomState(6)
    r3 = np.sort(rs.randn(M, W, 2), axis=2)
    r3[2, 1] = [0.5, 0.5]
    e = summary.member_edges(10, summary.check_batch_range(r3), M, W, None)
    for m in range(M):
        for d in range(W):
            assert np.array_equal(e[d][m], np.histogram_bin_edges(np.empty(0), bins=10, range=tuple(r3[m, d])))
    assert not summary.shared_edges(10, summary.check_batch_range(r3))
    for rng in ((-1.0, 2.0), [(-1.0, 2.0), (0.0, 0.0), (3.0, 4.5)]):
        r = summary.check_batch_range(rng)
        e = summary.member_edges(10, r, M, W, None)
        ref = summary.column_edges(10, r, W, None)
        assert summary.shared_edges(10, r)
        for d in range(W):
            assert np.array_equal(e[d], np.tile(ref[d], (M, 1)))
    own = [np.array([0.0, 1.0, 4.0]), np.arange(5.0), np.array([-1.0, 1.0])]
    e = summary.member_edges(summary.check_bins(own, "bins", 1024), None, M, W, None)
    assert [a.shape for a in e] == [(M, 3), (M, 5), (M, 2)] and all(np.array_equal(e[d][4], own[d]) for d in range(W))
    assert summary.shared_edges(own, None)
    # a step that underflows to 0 takes np.linspace's other expression: still the scalar call's bits
    lo, hi = np.array([[0.0, 0.0]]), np.array([[5e-324, 1.0]])
    e = summary.member_edges(4, None, 1, 2, (lo, hi))
    assert np.array_equal(e[0][0], np.linspace(0.0, 5e-324, 5)) and np.array_equal(e[1][0], np.linspace(0.0, 1.0, 5))


# ----------------------------------------------------------------------------------------------------------------- the twin
def test_host_histograms_batch_equals_numpy_per_member():
    x = batch_samples()
    M, n, W = x.shape
    fin = np.where(np.isfinite(x), x, 0.0)
    lo, hi = fin.min(axis=1), fin.max(axis=1)
    x = x.copy()
    x[0, ::7, 0] = np.nan                           # counted nowhere
    x[0, 3::11, 1] = np.inf
    x[5, 5::13, 3] = -np.inf
    for bins, pb in ((1, 1), (7, 5), (64, 33), (1024, 128)):
        edges = summary.member_edges(bins, None, M, W, (lo, hi))
        pedges = summary.member_edges(pb, None, M, W, (lo, hi))
        pairs = summary.column_pairs(summary.check_pairs("all"), W)
        counts, pc = summary.host_histograms_batch(x, edges, pedges, pairs)
        assert len(counts) == W and len(pc) == len(pairs) == W * (W - 1) // 2
        for d in range(W):
            assert counts[d].shape == (M, bins) and counts[d].dtype == np.int64
            for m in range(M):
                v = x[m, :, d]
                ref, _ = np.histogram(v[np.isfinite(v)], bins=edges[d][m])
                assert np.array_equal(counts[d][m], ref), (bins, m, d)
        for p, (i, j) in enumerate(pairs):
            assert pc[p].shape == (M, pb, pb) and pc[p].dtype == np.int64
            for m in range(M):
                ok = np.isfinite(x[m, :, i]) & np.isfinite(x[m, :, j])
                ref, _, _ = np.histogram2d(x[m, ok, i], x[m, ok, j], bins=[pedges[i][m], pedges[j][m]])
                assert np.array_equal(pc[p][m], ref.astype(np.int64)), (pb, m, i, j)
    # marginals alone
    counts, pc = summary.host_histograms_batch(x, edges, None, np.empty((0, 2), dtype=np.int64))
    assert pc == [] and len(counts) == W
