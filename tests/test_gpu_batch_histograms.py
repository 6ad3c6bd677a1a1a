"""EnsembleBatch.get_histograms / get_blob_histograms / PTSampler.get_histograms: emx_chain_minmax_batch and emx_histograms_batch
(csrc/emx_batch_hist.hpp) against NumPy on the host copy of the same chain (get_chain / get_blobs, never the code under test).

Every edge array must equal np.histogram_bin_edges of that member's column and every count np.histogram / np.histogram2d's,
with np.array_equal: the edges are np.linspace's bits and the counts are integers, so no tolerance exists or is needed.
Rejected proposals repeat rows, so every chain here has ties."""
import numpy as np
import pytest

from emcee_amd import EnsembleBatch, EnsembleSampler, PTSampler, _lib, moves, summary, targets
from emcee_amd.targets import BatchCallable

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- helpers
def expected_edges(x, bins, rng):
    """NumPy's edges for every member and column of x (M, n, W): W arrays (M, nb_d + 1)"""
    M, _, W = x.shape
    r = None if rng is None else np.broadcast_to(np.asarray(rng, dtype=np.float64), (M, W, 2))
    out = []
    for d in range(W):
        b = bins[d] if isinstance(bins, list) else bins
        out.append(np.stack([np.histogram_bin_edges(x[m, :, d], bins=b, range=None if r is None else tuple(r[m, d])) for m in range(M)]))
    return out


def check(r, x, bins, rng=None, pairs="all", pair_bins=None, what=""):
    """r (BatchHistograms of the M members of x (M, n, W)) against NumPy, array_equal throughout"""
    M, n, W = x.shape
    if isinstance(pairs, str):
        i, j = np.triu_indices(W, 1)
        pairs = np.stack([i, j], axis=1)
    pairs = np.asarray([] if pairs is None else pairs, dtype=np.int64).reshape(-1, 2)
    if pair_bins is None:
        pair_bins = min(bins, 64) if isinstance(bins, int) else bins
    assert isinstance(r, summary.BatchHistograms), what
    assert r.nsamples == n and np.array_equal(r.pairs, pairs), what
    assert len(r.edges) == len(r.counts) == len(r.pair_edges) == W and len(r.pair_counts) == len(pairs), what
    e, pe = expected_edges(x, bins, rng), expected_edges(x, pair_bins, rng)
    fin = np.isfinite(x)
    for d in range(W):
        assert r.edges[d].dtype == np.float64 and np.array_equal(r.edges[d], e[d]), (what, "edges", d)
        assert np.array_equal(r.pair_edges[d], pe[d]), (what, "pair edges", d)
        assert r.counts[d].dtype == np.int64 and r.counts[d].shape == (M, e[d].shape[1] - 1), (what, d)
        for m in range(M):
            ref, _ = np.histogram(x[m, fin[m, :, d], d], bins=e[d][m])
            assert np.array_equal(r.counts[d][m], ref), (what, "member", m, "column", d)
    for p, (i, j) in enumerate(pairs):
        assert r.pair_counts[p].dtype == np.int64 and r.pair_counts[p].shape == (M, pe[i].shape[1] - 1, pe[j].shape[1] - 1), (what, p)
        for m in range(M):
            ok = fin[m, :, i] & fin[m, :, j]
            ref, _, _ = np.histogram2d(x[m, ok, i], x[m, ok, j], bins=[pe[i][m], pe[j][m]])
            assert np.array_equal(r.pair_counts[p][m], ref.astype(np.int64)), (what, "member", m, "pair", (i, j))


def lift(h):
    """a member's plain Histograms with a leading member axis of 1"""
    assert isinstance(h, summary.Histograms)
    one = (lambda arrays: [a[None] for a in arrays])
    return summary.BatchHistograms(h.nsamples, one(h.edges), one(h.counts), h.pairs, one(h.pair_edges), one(h.pair_counts))


def same(a, b):
    return a.nsamples == b.nsamples and np.array_equal(a.pairs, b.pairs) and all(
        len(u) == len(v) and all(np.array_equal(p, q) for p, q in zip(u, v))
        for u, v in ((a.edges, b.edges), (a.counts, b.counts), (a.pair_edges, b.pair_edges), (a.pair_counts, b.pair_counts)))


def member_slice(r, b):
    cut = (lambda arrays: [a[b:b + 1] for a in arrays])
    return summary.BatchHistograms(r.nsamples, cut(r.edges), cut(r.counts), r.pairs, cut(r.pair_edges), cut(r.pair_counts))


def diag_targets(rs, B, D):
    mu, iv = 0.1 * rs.randn(B, D), 1.0 / (0.2 + rs.rand(B, D))
    return [targets.DiagGaussian(mu[b], iv[b]) for b in range(B)]


@pytest.fixture(scope="module")
def iso():
    """B = 3, 32 x 5, stretch, 200 steps -> (batch, its host chain (B, 200, 32, 5))"""
    rs = np.random.RandomState(0)
    bt = EnsembleBatch(3, 32, 5, targets.IsoGaussian(), moves=moves.StretchMove(), seeds=[100, 101, 102])
    bt.run_mcmc(rs.randn(3, 32, 5) * [[[1.0]], [[0.1]], [[3.0]]], 200)
    yield bt, bt.get_chain()
    bt.close()


def selected(chain, discard, thin):
    """get_chain(discard, thin, flat=True) of the host copy (B, steps, N, W)"""
    x = chain[:, discard + thin - 1::thin]
    return x.reshape(x.shape[0], -1, x.shape[3])


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("bins", [1, 7, 64, 1024])
def test_basic_counts_equal_numpy(iso, bins):
    bt, chain = iso
    assert (chain[:, 1:] == chain[:, :-1]).all(axis=3).any()               # rejections: ties
    for discard, thin in ((0, 1), (5, 3), (199, 1)):
        x = bt.get_chain(discard=discard, thin=thin, flat=True)
        assert np.array_equal(x, selected(chain, discard, thin))
        r = bt.get_histograms(bins=bins, discard=discard, thin=thin)
        check(r, x, bins, what="bins=%d discard=%d thin=%d" % (bins, discard, thin))
        assert all(c.sum(axis=1).tolist() == [x.shape[1]] * 3 for c in r.counts)        # min and max are edges: nothing is outside
        assert bt.histogram_launches() == 2                                # one binning pass and one pair pass for all members
    r = bt.get_histograms(bins=bins, pairs=None)
    check(r, selected(chain, 0, 1), bins, pairs=None, what="marginals only")
    assert r.pair_counts == [] and bt.histogram_launches() == 1


def test_odd_sizes_and_mixed_bin_counts():
    """33 x 7, DE + snooker: nothing is a multiple of a wave, a slice or a tile; a 128 x 128 panel fills 64 KB of LDS"""
    rs = np.random.RandomState(1)
    B, N, D = 3, 33, 7
    bt = EnsembleBatch(B, N, D, diag_targets(rs, B, D), moves=[(moves.DEMove(), 0.8), (moves.DESnookerMove(), 0.2)], seeds=[7, 8, 9])
    bt.run_mcmc(rs.randn(B, N, D), 131)
    nb = [3, 17, 64, 100, 255, 1000, 1024]
    for discard, thin in ((0, 1), (11, 5)):
        x = bt.get_chain(discard=discard, thin=thin, flat=True)
        # shared edges of the caller's, a little inside the data so that some samples are outside
        lo, hi = 0.9 * x.min(axis=(0, 1)), 0.9 * x.max(axis=(0, 1))
        edges = [np.linspace(lo[d], hi[d], nb[d] + 1) for d in range(D)]
        two = [(6, 0), (2, 5)]
        r = bt.get_histograms(bins=edges, pairs=two, pair_bins=128, discard=discard, thin=thin)       # the panels: every member's own range
        check(r, x, edges, pairs=two, pair_bins=128, what="list of edges")
        assert any(c.sum() < B * x.shape[1] for c in r.counts)
        pe = [np.linspace(lo[d], hi[d], 129 - d) for d in range(D)]
        r = bt.get_histograms(bins=64, pairs=two, pair_bins=pe, discard=discard, thin=thin)           # and the other way round
        check(r, x, 64, pairs=two, pair_bins=pe, what="list of pair edges")
        r = bt.get_histograms(bins=edges[:4] + edges[:3], pairs=[(0, 4), (5, 1), (3, 2)], discard=discard, thin=thin)     # bins serve the panels
        check(r, x, edges[:4] + edges[:3], pairs=[(0, 4), (5, 1), (3, 2)], what="bins as pair edges")
    bt.close()


def test_column_tiling():
    """64 x 32 dense with 1 024 bins a column: the edges and counters of 32 columns take several tiles; all 496 pairs"""
    rs = np.random.RandomState(2)
    B, N, D = 3, 64, 32
    A = rs.randn(D, D)
    icov = np.linalg.inv(A @ A.T / D + 0.5 * np.eye(D))
    bt = EnsembleBatch(B, N, D, targets.DenseGaussian(0.1 * rs.randn(D), 0.5 * (icov + icov.T)), seeds=[1, 2, 3])
    bt.run_mcmc(rs.randn(B, N, D), 41)
    x = bt.get_chain(discard=1, thin=2, flat=True)
    r = bt.get_histograms(bins=1024, pair_bins=16, discard=1, thin=2)
    assert len(r.pairs) == 496
    check(r, x, 1024, pair_bins=16, what="1024 bins x 32 columns")
    assert bt.histogram_launches() > 2                                     # more than one tile of columns
    r = bt.get_histograms(bins=16, pair_bins=16, discard=1, thin=2)
    check(r, x, 16, pair_bins=16, what="16 bins x 32 columns")
    assert bt.histogram_launches() == 2
    bt.close()


def test_single_column_and_ranges_of_their_own():
    rs = np.random.RandomState(0)
    p0 = rs.rand(3, 32, 1)
    p0[1, :16, 0] += 100.0              # these walkers never enter [0, 1]: half of member 1's samples are counted nowhere
    bt = EnsembleBatch(3, 32, 1, targets.UniformBox(), seeds=[100, 101, 102])
    bt.run_mcmc(p0, 64, skip_initial_state_check=True)
    x = bt.get_chain(flat=True)
    n = x.shape[1]
    r = bt.get_histograms(bins=10, range=(0, 1))
    check(r, x, 10, rng=(0, 1), what="range (0, 1)")
    assert r.counts[0].sum(axis=1).tolist() == [n, n // 2, n] and r.pairs.shape == (0, 2) and r.pair_counts == []
    own = np.array([[[0.0, 1.0]], [[100.0, 101.0]], [[0.25, 0.75]]])
    r = bt.get_histograms(bins=7, range=own)
    check(r, x, 7, rng=own, what="range (B, W, 2)")
    assert r.counts[0][1].sum() == n // 2 and 0 < r.counts[0][2].sum() < n
    r = bt.get_histograms(bins=5)                                        # member 1's own range is [0, 101]
    check(r, x, 5, what="own min and max")
    assert r.edges[0][1, -1] > 100.0
    check(lift(bt[1].get_histograms(bins=7, range=(100.0, 101.0))), x[1:2], 7, rng=(100.0, 101.0), what="member view")
    bt.close()


def test_values_exactly_on_edges(iso):
    """edges made of stored values, the minimum and the maximum included: half-open bins, the last one closed"""
    bt, chain = iso
    x = selected(chain, 3, 2)
    rs = np.random.RandomState(4)
    flat = x.reshape(-1, x.shape[2])
    edges = [np.unique(np.concatenate([[flat[:, d].min(), flat[:, d].max()], rs.choice(flat[:, d], 40)])) for d in range(5)]
    for d in range(5):
        assert 3 <= len(edges[d]) <= 42
        assert np.isin(flat[:, d], edges[d][1:-1]).any() and (flat[:, d] == edges[d][-1]).any() and (flat[:, d] == edges[d][0]).any()
    r = bt.get_histograms(bins=edges, discard=3, thin=2)
    check(r, x, edges, what="edges of stored values")
    assert all(c.sum() == 3 * x.shape[1] for c in r.counts)               # the value on the last edge is counted
    # a member's own edges through its own values: (B, W, 2) ranges that end on its extremes, one bin
    own = np.stack([x.min(axis=1), x.max(axis=1)], axis=2)
    r = bt.get_histograms(bins=1, range=own, discard=3, thin=2)
    check(r, x, 1, rng=own, what="one bin from min to max")
    assert all((c == x.shape[1]).all() for c in r.counts)


def test_member_ranges_and_chunking():
    rs = np.random.RandomState(5)
    B, N, D = 70, 32, 3
    bt = EnsembleBatch(B, N, D, diag_targets(rs, B, D), seeds=list(range(500, 500 + B)))
    bt.run_mcmc(rs.randn(B, N, D), 60)
    kw = dict(bins=33, pair_bins=20, discard=4, thin=3)
    for stored in (60, 97):
        if stored == 97:
            bt.run_mcmc(None, 37)                                          # the chain grows: the members' capacity is not their stored rows
        assert bt.iteration == stored
        x = bt.get_chain(discard=4, thin=3, flat=True)
        ref = bt.get_histograms(**kw)
        check(ref, x, 33, pair_bins=20, what="70 members, %d stored" % stored)
        assert bt.histogram_launches() == 2                                # as for 3 members
        for b in (0, 37, 69):
            m = bt[b].get_histograms(**kw)
            assert same(lift(m), member_slice(ref, b)), b
            assert all(u.shape == v.shape[1:] for u, v in zip(m.counts + m.pair_counts, ref.counts + ref.pair_counts))
        for key, values in (("batch_hist_members", (1, 7, 0)), ("batch_hist_rows", (1, 7, 0))):
            for k in values:
                bt.set_tuning(key, k)
                assert same(bt.get_histograms(**kw), ref), (key, k)
                if key == "batch_hist_members" and k:
                    assert bt.histogram_launches() == 2 * ((B + k - 1) // k)
        assert same(bt.get_histograms(**kw), ref)
    with pytest.raises(_lib.EmxError, match="batch_hist_members"):
        bt.set_tuning("batch_hist_members", -1)
    bt.close()


def test_member_equals_the_single_sampler():
    B, N, D = 3, 32, 4
    rs = np.random.RandomState(9)
    tg = diag_targets(rs, B, D)
    p0 = rs.randn(B, N, D)
    seeds = [11, 22, 33]
    bt = EnsembleBatch(B, N, D, tg, moves=moves.StretchMove(), seeds=seeds)
    bt.run_mcmc(p0, 150)
    own = [np.linspace(-2, 2, 9), np.linspace(-1, 3, 30), np.array([-0.5, 0.0, 0.25, 4.0]), np.linspace(-3, 3, 129)]
    for b in range(B):
        s = EnsembleSampler(N, D, tg[b], moves=moves.StretchMove(), rng="philox")
        s.random_state = np.random.RandomState(seeds[b]).get_state()
        s.run_mcmc(p0[b], 150)
        assert np.array_equal(s.get_chain(), bt[b].get_chain())
        assert s.backend._dev is not None                   # its get_histograms takes emx_histograms
        for kw in (dict(), dict(bins=1024, discard=10, thin=4), dict(bins=17, range=(-1.5, 2.0), pairs=[(3, 1)], pair_bins=128),
                   dict(bins=own, pairs=None), dict(bins=40, range=np.array([[-1, 1], [0, 0], [-2, 3], [0.5, 0.75]]), pair_bins=own)):
            u, v = bt[b].get_histograms(**kw), s.get_histograms(**kw)
            assert type(u) is type(v) is summary.Histograms and same(u, v), (b, kw)
            assert all(p.shape == q.shape for p, q in zip(u.edges + u.counts + u.pair_counts, v.edges + v.counts + v.pair_counts))
    bt.close()


def test_blob_plane():
    import torch

    def fn(q):                                               # blob 1: NaN for some rows, +inf for others
        lp = -0.5 * (q * q).sum(-1)
        b1 = torch.where(q[..., 0] > 1.0, torch.full_like(lp, float("nan")), torch.where(q[..., 0] < -1.0, torch.full_like(lp, float("inf")), q[..., 1]))
        return lp, torch.stack([q.sum(-1), b1], dim=-1)
    rs = np.random.RandomState(6)
    B, N, D = 3, 32, 3
    bt = EnsembleBatch(B, N, D, BatchCallable(fn, nblobs=2), seeds=[4, 5, 6])
    bt.run_mcmc(rs.randn(B, N, D), 80)
    bl = bt.get_blobs(discard=5, thin=2, flat=True)
    assert np.isnan(bl[..., 1]).any() and np.isposinf(bl[..., 1]).any() and np.isfinite(bl[..., 0]).all()
    with pytest.raises(ValueError, match="column 1") as e:
        bt.get_blob_histograms(discard=5, thin=2)
    assert "member 0 column 1" in str(e.value) and "column 0" not in str(e.value)
    rng = [(-6.0, 6.0), (-3.0, 3.0)]
    r = bt.get_blob_histograms(bins=50, range=rng, discard=5, thin=2)
    check(r, bl, 50, rng=rng, what="blobs")
    assert r.counts[1].sum() <= np.isfinite(bl[..., 1]).sum() < bl[..., 1].size     # the non-finite values are counted nowhere
    m = bt[2].get_blob_histograms(bins=50, range=rng, discard=5, thin=2)
    assert same(lift(m), member_slice(r, 2))
    check(bt.get_histograms(bins=12), bt.get_chain(flat=True), 12, what="the chain of a target with blobs")
    plain = EnsembleBatch(B, N, D, targets.IsoGaussian(), seeds=[4, 5, 6])
    plain.run_mcmc(rs.randn(B, N, D), 5)
    for get in (plain.get_blob_histograms, plain[0].get_blob_histograms):
        with pytest.raises(ValueError, match="no blobs"):
            get()
    plain.close()
    bt.close()


def test_ptsampler_histograms_have_rung_axes():
    G, T, N, D = 2, 3, 32, 2
    fn = lambda q: -0.5 * (q * q).sum(-1) - np.log(2 * np.pi)  # noqa: E731
    s = PTSampler(T, N, D, BatchCallable(fn), log_prior=(-10 * np.ones(D), 10 * np.ones(D)), Tmax=20.0, nbatch=G, seeds=[3, 4])
    s.run_mcmc(np.random.RandomState(0).uniform(-1, 1, size=(G, T, N, D)), 120)
    x = s.get_chain(discard=20, thin=2, flat=True)                       # (G, T, n, D)
    n = x.shape[2]
    r = s.get_histograms(bins=30, discard=20, thin=2)
    assert r.nsamples == n == 50 * N
    assert all(a.shape == (G, T, 31) for a in r.edges) and all(a.shape == (G, T, 30) for a in r.counts)
    assert len(r.pair_counts) == 1 and r.pair_counts[0].shape == (G, T, 30, 30) and r.pair_edges[0].shape == (G, T, 31)
    flat = (lambda arrays: [a.reshape((G * T,) + a.shape[2:]) for a in arrays])
    check(summary.BatchHistograms(r.nsamples, flat(r.edges), flat(r.counts), r.pairs, flat(r.pair_edges), flat(r.pair_counts)),
          x.reshape(G * T, n, D), 30, what="every rung")
    for o in range(G):                                                   # and rung by rung, on get_chain()[o, t]
        for t in range(T):
            for d in range(D):
                ref, e = np.histogram(x[o, t, :, d], bins=30)
                assert np.array_equal(r.counts[d][o, t], ref) and np.array_equal(r.edges[d][o, t], e)
    own = np.zeros((G, T, D, 2)) + [-1.0, 1.0]
    own[1, 2] = [-8.0, 8.0]                                              # the hottest rung of object 1
    r = s.get_histograms(bins=9, range=own, pairs=None)
    for o in range(G):
        for t in range(T):
            ref, e = np.histogram(s.get_chain()[o, t, :, :, 0].ravel(), bins=9, range=tuple(own[o, t, 0]))
            assert np.array_equal(r.counts[0][o, t], ref) and np.array_equal(r.edges[0][o, t], e)
    s.close()
