"""EnsembleSampler.get_histograms: emx_chain_minmax / emx_histograms (csrc/emx_hist.hpp) against np.histogram / np.histogram2d on
the host copy of the same chain (get_chain / get_blobs, never the code under test).  Every count is an integer sum, so equality
is np.array_equal on every count of every column and every panel; the edges are NumPy's own bits.

Shapes: the chains of tests/test_gpu_ensemble_summary.py::make_case (shared, only read) -- ties from rejected proposals
(66 x 7, a = 3), nothing a tile multiple (130 x 33), many workgroups a panel (8 192 x 64, all 2 016 pairs), a chain regrown between
two runs and counted in many chunks with a ragged last one (4 096 x 8, "hist_chunk_rows" 1 and 7), a single column with half the
samples outside (32 x 1), the exact-mode chain writer, and the blob plane of a DeviceFused target."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from emcee_amd import EnsembleSampler, summary
from emcee_amd._lib import EmxError
from emcee_amd.device import DeviceEnsemble

from test_gpu_ensemble_summary import make_case

pytestmark = pytest.mark.gpu


def all_pairs(W):
    return [(i, j) for i in range(W) for j in range(i + 1, W)]


def check(x, h, bins, rng=None, pairs="all", pair_bins=None, label=""):
    """h against NumPy on the (n, W) samples x.  bins / pair_bins: what NumPy is given per column -- an int (with the ranges
    `rng` (W, 2), or None: the column's min and max) or a list of W edge arrays."""
    n, W = x.shape
    assert isinstance(h, summary.Histograms) and h.nsamples == n, label
    assert len(h.edges) == len(h.counts) == len(h.pair_edges) == W, label
    cols = [np.ascontiguousarray(x[:, d]) for d in range(W)]
    for d in range(W):
        r = None if rng is None or not isinstance(bins, int) else tuple(rng[d])
        c, e = np.histogram(cols[d], bins=bins if isinstance(bins, int) else bins[d], range=r)
        assert h.counts[d].dtype == np.int64 and np.array_equal(h.edges[d], e), (label, d)
        assert np.array_equal(h.counts[d], c), (label, d, h.counts[d], c)
        if isinstance(pair_bins, int):
            r = None if rng is None else tuple(rng[d])
            assert np.array_equal(h.pair_edges[d], np.histogram_bin_edges(cols[d], bins=pair_bins, range=r)), (label, d)
        else:
            assert np.array_equal(h.pair_edges[d], pair_bins[d]), (label, d)
    want = all_pairs(W) if isinstance(pairs, str) else list(pairs or ())
    assert h.pairs.shape == (len(want), 2) and h.pairs.tolist() == [list(p) for p in want], label
    assert len(h.pair_counts) == len(want), label

    def ref(p):
        return np.histogram2d(cols[p[0]], cols[p[1]], bins=[h.pair_edges[p[0]], h.pair_edges[p[1]]])[0]
    with ThreadPoolExecutor(8) as ex:
        refs = list(ex.map(ref, want))
    for p, pc, c in zip(want, h.pair_counts, refs):
        assert pc.dtype == np.int64 and pc.shape == c.shape, (label, p)
        assert np.array_equal(pc, c), (label, p)
    return h


def flat(s, discard=0, thin=1, value=None):
    x = (value or s.get_chain)(discard=discard, thin=thin, flat=True)
    return x.reshape(len(x), -1)


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("discard,thin", [(0, 1), (5, 3), (36, 1)])
def test_ties_every_bin_count_and_all_pairs(discard, thin):
    s = make_case("diag_66x7")
    x = flat(s, discard, thin)
    assert discard == 36 or len(np.unique(x[:, 0])) < len(x)      # rejected proposals repeat rows: ties (one row alone has none)
    for bins in (1, 7, 64, 1024):
        h = check(x, s.get_histograms(bins=bins, discard=discard, thin=thin), bins, pair_bins=min(bins, 64), label="bins=%d" % bins)
        assert len(h.pair_counts) == 21
        assert all(c.sum() == len(x) for c in h.counts) and all(c.sum() == len(x) for c in h.pair_counts)
    lst = [(6, 0), (0, 6), (3, 2)]
    h = check(x, s.get_histograms(bins=33, pair_bins=9, pairs=lst, discard=discard, thin=thin), 33, pairs=lst, pair_bins=9, label="list")
    assert np.array_equal(h.pair_counts[0], h.pair_counts[1].T)
    check(x, s.get_histograms(bins=33, pairs=None, discard=discard, thin=thin), 33, pairs=None, pair_bins=33, label="marginals only")


@pytest.mark.parametrize("pair_bins", [128, 1])
def test_odd_width_all_528_pairs_the_largest_and_the_smallest_panel(pair_bins):
    s = make_case("iso_130x33")
    x = flat(s)
    h = check(x, s.get_histograms(bins=50, pair_bins=pair_bins), 50, pair_bins=pair_bins, label="iso_130x33")
    assert len(h.pair_counts) == 528 and h.pair_counts[0].shape == (pair_bins, pair_bins)
    x = flat(s, 3, 2)
    check(x, s.get_histograms(bins=1024, pair_bins=pair_bins, discard=3, thin=2, pairs=[(32, 0), (16, 31)]), 1024, pairs=[(32, 0), (16, 31)],
          pair_bins=pair_bins, label="iso_130x33 1024 bins: column tiles")


def test_many_workgroups_a_panel_all_2016_pairs():
    s = make_case("dense_8192x64_philox")
    x = flat(s)
    h = check(x, s.get_histograms(bins=64, pair_bins=32), 64, pair_bins=32, label="dense_8192x64")
    assert len(h.pair_counts) == 2016 and sum(int(c.sum()) for c in h.pair_counts) == 2016 * len(x)


def test_chain_regrown_between_two_runs_and_counted_in_chunks():
    s = make_case("iso_4096x8_regrown")
    assert s.get_chain().shape == (64, 4096, 8)
    ens = s.backend._dev
    kw = dict(bins=40, pair_bins=24, discard=3, thin=2)
    x = flat(s, 3, 2)
    got = []
    try:
        for rows in (0, 1, 7, 0):                          # 30 selected rows: one chunk, 30 chunks, 4 chunks of 7 and one of 2
            ens.set_tuning("hist_chunk_rows", rows)
            got.append(s.get_histograms(**kw))
    finally:
        ens.set_tuning("hist_chunk_rows", 0)
    check(x, got[0], 40, pair_bins=24, label="regrown")
    for g in got[1:]:
        assert all(np.array_equal(u, v) for u, v in zip(g.counts, got[0].counts))
        assert all(np.array_equal(u, v) for u, v in zip(g.pair_counts, got[0].pair_counts))
    check(flat(s), s.get_histograms(bins=64), 64, pair_bins=64, label="regrown, everything")


def test_one_column_half_the_samples_outside_and_the_closed_last_bin():
    s = make_case("box_32x1")
    x = flat(s)
    assert (x[:, 0] > 99).sum() * 2 == len(x)
    h = check(x, s.get_histograms(bins=10, range=(0, 1)), 10, rng=[(0.0, 1.0)], pair_bins=10, label="box range")
    assert h.pairs.shape == (0, 2) and h.pair_counts == [] and h.counts[0].sum() * 2 == len(x)
    h = check(x, s.get_histograms(bins=16), 16, pair_bins=16, label="box auto")
    assert h.counts[0].sum() == len(x) and h.counts[0][-1] >= 1 and h.edges[0][-1] == x.max()
    for discard, thin in ((4, 3), (29, 1)):
        check(flat(s, discard, thin), s.get_histograms(bins=5, discard=discard, thin=thin), 5, pair_bins=5, label="box")


def test_edges_made_of_stored_values_public_and_raw_call():
    s = make_case("diag_66x7")
    x = flat(s, 2, 2)
    rs = np.random.RandomState(3)
    edges = []
    for d in range(7):
        v = np.unique(x[:, d])
        edges.append(np.sort(rs.choice(v, size=min(len(v), 20 + 9 * d), replace=False)))      # every edge is a stored value
    check(x, s.get_histograms(bins=edges, discard=2, thin=2), edges, pair_bins=edges, label="own edges")
    one = edges[3]
    check(x, s.get_histograms(bins=one, pair_bins=edges, discard=2, thin=2), [one] * 7, pair_bins=edges, label="one edge array")
    # the raw call: rows 3, 5, ... of the stored chain
    pairs = np.array(all_pairs(7), dtype=np.int32)
    n, counts, pc = s.backend._dev.histograms(3, s.iteration, edges, edges, pairs, stride=2)
    assert n == len(x)
    check(x, summary.Histograms(n, edges, counts, pairs.astype(np.int64), edges, pc), edges, pair_bins=edges, label="raw")
    # what the library refuses
    for bad_edges, bad_pairs, msg in (([e[::-1] for e in edges], pairs, "strictly increasing"), (edges, [(0, 7)], "two different columns"),
                                      (edges, [(2, 2)], "two different columns"), ([np.arange(1026.0)] * 7, pairs, "1 ... 1024")):
        with pytest.raises(EmxError, match=msg):
            s.backend._dev.histograms(3, s.iteration, bad_edges, edges, bad_pairs, stride=2)
    with pytest.raises(EmxError, match="1 ... 128"):
        s.backend._dev.histograms(3, s.iteration, edges, [np.arange(130.0)] * 7, pairs, stride=2)


@pytest.mark.parametrize("name", ["diag_66x7", "iso_130x33", "iso_4096x8_regrown"])
def test_chain_minmax_is_exact(name):
    s = make_case(name)
    for discard, thin in ((0, 1), (4, 3)):
        x = flat(s, discard, thin)
        lo, hi, nf = s.backend._dev.chain_minmax(discard + thin - 1, s.iteration, thin)
        assert np.array_equal(lo, x.min(0)) and np.array_equal(hi, x.max(0)) and not nf.any() and nf.dtype == np.int64


def test_blob_plane_of_a_fused_target():
    from test_gpu_ensemble_fused_blobs import Model
    m = Model(5, 2)
    s = EnsembleSampler(64, 5, m.blobs(), rng="philox")
    s.run_mcmc(m.start(64), 30, skip_initial_state_check=True)
    assert s.backend._dev is not None and s.backend._dev_nblobs() == 2
    for discard, thin in ((0, 1), (4, 2)):
        x = flat(s, discard, thin, value=s.get_blobs)
        assert x.shape[1] == 2
        h = check(x, s.get_blob_histograms(bins=30, discard=discard, thin=thin), 30, pair_bins=30, label="blobs")
        assert len(h.pair_counts) == 1
        lo, hi, nf = s.backend._dev.chain_minmax(discard + thin - 1, s.iteration, thin, plane=2)
        assert np.array_equal(lo, x.min(0)) and np.array_equal(hi, x.max(0))
    check(flat(s), s.get_histograms(bins=30), 30, pair_bins=30, label="blob sampler's coordinates")
    m.close()


def test_exact_mode_chain_writer():
    s = make_case("iso_64x5_mt")
    for discard, thin in ((0, 1), (3, 2)):
        check(flat(s, discard, thin), s.get_histograms(bins=25, discard=discard, thin=thin), 25, pair_bins=25, label="mt19937")


def test_a_failing_device_call_falls_back_to_numpy(monkeypatch):
    s = make_case("diag_66x7")
    x = flat(s, 1, 2)
    called = []

    def refuse(self, *a, **k):
        called.append(1)
        raise EmxError("no room for the scratch")
    monkeypatch.setattr(DeviceEnsemble, "histograms", refuse)
    check(x, s.get_histograms(bins=12, discard=1, thin=2), 12, pair_bins=12, label="fallback")
    assert called
    monkeypatch.setattr(DeviceEnsemble, "chain_minmax", refuse)
    check(x, s.get_histograms(bins=12, discard=1, thin=2), 12, pair_bins=12, label="fallback, min / max too")
    check(x, s.get_histograms(bins=12, range=(-1, 1), discard=1, thin=2), 12, rng=[(-1.0, 1.0)] * 7, pair_bins=12, label="fallback, range")


def test_contexts_take_turns_above_64_kb_of_lds(monkeypatch):
    """A kernel's dynamic-LDS limit belongs to the function and the device, not to a context: a small call from a second
    context must not leave the first one's next large launch (1 024-bin tiles, 128 x 128 panels) without it.  Every call has to
    come back from the device: one that failed there would be answered by the NumPy fallback and pass `check` all the same."""
    done = []
    device_call = DeviceEnsemble.histograms

    def counted(self, *a, **k):
        out = device_call(self, *a, **k)
        done.append(self)
        return out
    monkeypatch.setattr(DeviceEnsemble, "histograms", counted)
    a, b = make_case("iso_130x33"), make_case("diag_66x7")
    assert a.backend._dev is not b.backend._dev
    xa, xb, pa, pb = flat(a), flat(b), [(32, 0), (16, 31)], [(6, 0), (3, 2)]
    turns = ((a, xa, pa, 1024, 128), (b, xb, pb, 7, 3), (a, xa, pa, 1024, 128), (b, xb, pb, 1024, 128), (a, xa, pa, 1000, 127))
    for turn, (s, x, pairs, bins, pair_bins) in enumerate(turns):
        check(x, s.get_histograms(bins=bins, pair_bins=pair_bins, pairs=pairs), bins, pairs=pairs, pair_bins=pair_bins, label="turn %d" % turn)
    assert [e is s.backend._dev for e, (s, *_) in zip(done, turns)] == [True] * len(turns)


def test_histograms_in_the_middle_of_a_run_change_no_later_sample():
    from emcee_amd import targets

    def run(look):
        s = EnsembleSampler(66, 7, targets.IsoGaussian(), rng="philox")
        s.random_state = np.random.RandomState(5).get_state()
        st = s.run_mcmc(np.random.RandomState(6).randn(66, 7), 20)
        if look:
            s.get_histograms(discard=3, thin=2)
        s.run_mcmc(st, 20)
        return s
    a, b = run(False), run(True)
    assert np.array_equal(a.get_chain(), b.get_chain()) and np.array_equal(a.get_log_prob(), b.get_log_prob())
    check(flat(b), b.get_histograms(bins=20), 20, pair_bins=20, label="after continuing")
