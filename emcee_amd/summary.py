"""Posterior summaries of :class:`~emcee_amd.EnsembleBatch` chains: the host side.

The device (``emx_summary_batch``, ``csrc/emx_batch_summary.hip``) returns means, covariances, the best stored sample and
*order statistics* -- the k-th smallest stored value of every parameter of every member.  Quantiles are interpolated here from
those, with NumPy's default ("linear") rule: for ``n`` samples and a quantile ``q``, :func:`quantile_ranks` gives the two ranks
``lo`` / ``hi`` around the virtual index ``(n - 1) q`` and its fractional part ``g``, and :func:`lerp` -- NumPy's ``_lerp`` --
interpolates between the two order statistics.  Together they reproduce ``np.quantile(x, q)`` of NumPy 2.2 bit for bit.
"""
from collections import namedtuple

import numpy as np

__all__ = ["BatchSummary", "Histograms", "BatchHistograms", "RHat", "Evidence", "split_rhat", "quantile_ranks", "lerp", "MAX_QUANTILES",
           "MAX_BINS", "MAX_PAIR_BINS"]

MAX_QUANTILES = 16          # two ranks a quantile: the 32 ranks of one emx_summary_batch call

BatchSummary = namedtuple("BatchSummary", ["nsamples", "mean", "cov", "quantiles", "map_coords", "map_log_prob"])
BatchSummary.__doc__ = """The result of ``get_summary``: ``nsamples`` (selected steps x walkers), ``mean`` ``(..., ndim)``, ``cov``
``(..., ndim, ndim)`` (``ddof = 1``; None when not asked for), ``quantiles`` ``(..., nq, ndim)``, ``map_coords`` ``(..., ndim)`` and
``map_log_prob`` ``(...)``: the stored sample with the largest stored log-prob."""

MAX_BINS = 1024             # marginal bins a column of one emx_histograms call
MAX_PAIR_BINS = 128         # pair-panel bins a column: a panel's counters fit a workgroup's LDS

Histograms = namedtuple("Histograms", ["nsamples", "edges", "counts", "pairs", "pair_edges", "pair_counts"])
Histograms.__doc__ = """The result of ``get_histograms``: ``nsamples`` (selected steps x walkers); per column ``edges`` (float64,
``(nb_d + 1,)``) and ``counts`` (int64, ``(nb_d,)``): ``np.histogram``'s; ``pairs`` ``(P, 2)`` column pairs ``(i, j)``, per column
``pair_edges`` (``(pb_d + 1,)``) and per pair ``pair_counts`` (int64, ``(pb_i, pb_j)``, axis 0 is column ``i``):
``np.histogram2d(x[:, i], x[:, j], bins=[pair_edges[i], pair_edges[j]])``'s."""

BatchHistograms = namedtuple("BatchHistograms", ["nsamples", "edges", "counts", "pairs", "pair_edges", "pair_counts"])
BatchHistograms.__doc__ = """The result of ``EnsembleBatch.get_histograms``: :class:`Histograms` with a leading member axis on every
per-column and per-panel array -- ``nsamples`` (selected steps x walkers, of every member); per column ``edges`` (float64,
``(M, nb_d + 1)``: every member has its own) and ``counts`` (int64, ``(M, nb_d)``); ``pairs`` ``(P, 2)``, common to all members; per
column ``pair_edges`` (``(M, pb_d + 1)``) and per pair ``pair_counts`` (int64, ``(M, pb_i, pb_j)``, axis 1 is column ``i``).  Member
``m``'s numbers are ``np.histogram`` / ``np.histogram2d``'s on that member's samples with that member's edges.  The count arrays
may be views of the two buffers the device filled (copy one to keep it without the rest)."""


def quantile_ranks(n, q):
    """-> ``(lo, hi, g)``: NumPy's linear rule for the quantile(s) ``q`` of ``n`` sorted values: ``h = (n - 1) q``,
    ``lo = floor(h)``, ``hi = min(lo + 1, n - 1)``, ``g = h - lo``.  Integer arrays ``lo`` / ``hi`` and a float array ``g`` of
    ``q``'s shape."""
    n = int(n)
    if n < 1:
        raise ValueError("quantile_ranks needs n >= 1; got %d" % n)
    q = np.asarray(q, dtype=np.float64)
    if not (np.isfinite(q).all() and (q >= 0).all() and (q <= 1).all()):
        raise ValueError("quantiles must be finite and in [0, 1]; got %r" % (q.tolist(),))
    h = (n - 1) * q
    fl = np.floor(h)
    lo = np.minimum(fl.astype(np.int64), n - 1)
    hi = np.minimum(lo + 1, n - 1)
    return lo, hi, h - fl


def lerp(a, b, g):
    """NumPy's ``_lerp``: ``a + (b - a) g`` where ``g < 0.5``, else ``b - (b - a) (1 - g)``."""
    a, b, g = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(g, dtype=np.float64)
    diff = b - a
    return np.where(g >= 0.5, b - diff * (1 - g), a + diff * g)


def check_quantiles(quantiles):
    """-> the quantiles as a 1-d float array, or ValueError: finite, in [0, 1], at most :data:`MAX_QUANTILES`."""
    q = np.atleast_1d(np.asarray(quantiles, dtype=np.float64)).ravel()
    if len(q) > MAX_QUANTILES:
        raise ValueError("at most %d quantiles in one call; got %d" % (MAX_QUANTILES, len(q)))
    if not (np.isfinite(q).all() and (q >= 0).all() and (q <= 1).all()):
        raise ValueError("every quantile must be finite and in [0, 1]; got %r" % (q.tolist(),))
    return q


def plan_ranks(n, q):
    """-> ``(ranks, ilo, ihi, g)``: the distinct ranks (sorted, at most ``2 len(q)``) that the quantiles ``q`` of ``n`` samples
    need, and for each quantile the positions of its ``lo`` / ``hi`` in ``ranks`` and its ``g``."""
    lo, hi, g = quantile_ranks(n, q)
    ranks = np.unique(np.concatenate([lo, hi])).astype(np.int64)
    return ranks, np.searchsorted(ranks, lo), np.searchsorted(ranks, hi), g


def interpolate(order, ilo, ihi, g):
    """``order`` ``(members, nranks, ndim)`` order statistics -> ``(members, nq, ndim)`` quantiles."""
    if len(g) == 0:
        return np.empty((order.shape[0], 0, order.shape[2]))
    return lerp(order[:, ilo, :], order[:, ihi, :], g[None, :, None])


# ---- histograms: the host side (argument forms, edges, and the NumPy twin of emx_histograms) --------------------------------
def _edge_array(e, what, maxbins):
    e = np.asarray(e, dtype=np.float64)
    if e.ndim != 1 or len(e) < 2:
        raise ValueError("%s: bin edges are a 1-D array of at least 2 values; got shape %s" % (what, e.shape))
    if not (np.diff(e) > 0).all():              # NaN fails too
        raise ValueError("%s: bin edges must be strictly increasing" % what)
    if len(e) - 1 > maxbins:
        raise ValueError("%s: at most %d bins a column; got %d" % (what, maxbins, len(e) - 1))
    return e


def check_bins(bins, what, maxbins):
    """-> an int (bins of every column), one float64 edge array (for every column) or a list of edge arrays (one a column, its
    length checked by :func:`column_edges`), or ValueError / TypeError: nothing here needs the number of columns."""
    if isinstance(bins, (bool, np.bool_)):
        raise TypeError("%s must be an integer or bin edges; got %r" % (what, bins))
    if isinstance(bins, (int, np.integer)):
        if not 1 <= bins <= maxbins:
            raise ValueError("%s must be between 1 and %d; got %d" % (what, maxbins, bins))
        return int(bins)
    if np.isscalar(bins) or (isinstance(bins, np.ndarray) and bins.ndim == 0):
        raise TypeError("%s must be an integer or bin edges; got %r" % (what, bins))
    if all(np.isscalar(b) for b in bins):
        return _edge_array(bins, what, maxbins)
    return [_edge_array(b, what, maxbins) for b in bins]


def check_range(range):
    """-> None, or a float64 ``(2,)`` / ``(W, 2)`` array with finite ``lo <= hi``"""
    if range is None:
        return None
    r = np.asarray(range, dtype=np.float64)
    if r.shape != (2,) and not (r.ndim == 2 and r.shape[1] == 2):
        raise ValueError("range is None, (lo, hi) or an array (ncolumns, 2); got shape %s" % (r.shape,))
    if not np.isfinite(r).all():
        raise ValueError("range must be finite; got %r" % (r.tolist(),))
    if (r[..., 0] > r[..., 1]).any():
        raise ValueError("range needs lo <= hi; got %r" % (r.tolist(),))
    return r


def check_pairs(pairs):
    """-> "all", or an int64 ``(P, 2)`` array of pairs ``i != j``, none negative (the upper bound needs the number of columns:
    :func:`column_pairs`)"""
    if isinstance(pairs, str):
        if pairs != "all":
            raise ValueError("pairs is 'all', None or a sequence of (i, j); got %r" % (pairs,))
        return pairs
    if pairs is None or len(pairs) == 0:
        return np.empty((0, 2), dtype=np.int64)
    p = np.asarray(pairs)
    if p.ndim != 2 or p.shape[1] != 2 or p.dtype.kind not in "iu":
        raise ValueError("pairs is 'all', None or a sequence of integer (i, j); got %r" % (pairs,))
    p = p.astype(np.int64)
    if (p[:, 0] == p[:, 1]).any():
        raise ValueError("a pair needs two different columns; got %r" % (p[p[:, 0] == p[:, 1]][0].tolist(),))
    if (p < 0).any():
        raise ValueError("pair columns are counted from 0; got %r" % (p[(p < 0).any(axis=1)][0].tolist(),))
    return p


def column_pairs(pairs, W):
    """the checked ``pairs`` for ``W`` columns -> int64 ``(P, 2)``"""
    if isinstance(pairs, str):
        i, j = np.triu_indices(W, 1)
        return np.stack([i, j], axis=1).astype(np.int64)
    if (pairs >= W).any():
        raise ValueError("pair %r is outside the %d columns" % (pairs[(pairs >= W).any(axis=1)][0].tolist(), W))
    return pairs


def check_columns(bins, range, W, what):
    """what of the checked ``bins`` / ``range`` depends on the number of columns"""
    if isinstance(bins, list) and len(bins) != W:
        raise ValueError("%s: one edge array for every one of the %d columns; got %d" % (what, W, len(bins)))
    if range is not None and range.ndim == 2 and len(range) != W:
        raise ValueError("range: one (lo, hi) for every one of the %d columns; got %d" % (W, len(range)))


def needs_minmax(bins, pair_bins, range):
    """whether some column's edges come from the data's min and max"""
    return range is None and (isinstance(bins, int) or isinstance(pair_bins, int))


def column_edges(bins, range, W, minmax):
    """-> the W edge arrays: ``np.linspace(lo, hi, bins + 1)`` -- ``np.histogram``'s own expression -- for an integer ``bins``
    (``lo == hi`` widened by 0.5 each way as NumPy does), else the caller's edges.  ``minmax``: ``(lo (W), hi (W))`` of the data,
    used where ``range`` is None."""
    if isinstance(bins, int):
        if range is None:
            lo, hi = (np.asarray(v, dtype=np.float64) for v in minmax)
        else:
            r = np.broadcast_to(range, (W, 2))
            lo, hi = r[:, 0], r[:, 1]
        out = []
        for a, b in zip(lo, hi):
            if a == b:
                a, b = a - 0.5, b + 0.5
            out.append(np.linspace(a, b, bins + 1))
        return out
    return list(bins) if isinstance(bins, list) else [bins] * W


def bin_index(x, e):
    """-> (bin of every x in the edges e under np.histogram's rule, whether it has one)"""
    ok = (x >= e[0]) & (x <= e[-1])                     # NaN: False
    b = np.searchsorted(e, x, side="right") - 1
    b[b == len(e) - 1] = len(e) - 2                     # the last bin is closed
    return b, ok


def host_histograms(x, edges, pair_edges, pairs):
    """the NumPy twin of ``emx_histograms`` on the ``(n, W)`` samples ``x`` -> ``(counts, pair_counts)``"""
    W = x.shape[1]
    counts = []
    for d in range(W):
        b, ok = bin_index(x[:, d], edges[d])
        counts.append(np.bincount(b[ok], minlength=len(edges[d]) - 1).astype(np.int64))
    code = {}
    for d in sorted(set(np.asarray(pairs).ravel().tolist())):
        code[d] = bin_index(x[:, d], pair_edges[d])
    pc = []
    for i, j in pairs:
        (bi, oi), (bj, oj) = code[i], code[j]
        ni, nj = len(pair_edges[i]) - 1, len(pair_edges[j]) - 1
        ok = oi & oj
        pc.append(np.bincount(bi[ok] * nj + bj[ok], minlength=ni * nj).astype(np.int64).reshape(ni, nj))
    return counts, pc


# ---- histograms of a batch: every member its own edges ----------------------------------------------------------------------
def check_batch_range(range):
    """:func:`check_range`, or additionally a float64 ``(B, W, 2)`` array: one ``(lo, hi)`` for every column of every member"""
    if range is not None:
        r = np.asarray(range, dtype=np.float64)
        if r.ndim == 3:
            if r.shape[2] != 2:
                raise ValueError("range is None, (lo, hi), (ncolumns, 2) or (nmembers, ncolumns, 2); got shape %s" % (r.shape,))
            if not np.isfinite(r).all():
                raise ValueError("range must be finite; got a non-finite bound for member(s) %s"
                                 % np.flatnonzero(~np.isfinite(r).all(axis=(1, 2))).tolist())
            if (r[..., 0] > r[..., 1]).any():
                raise ValueError("range needs lo <= hi; not so for member(s) %s" % np.flatnonzero((r[..., 0] > r[..., 1]).any(axis=1)).tolist())
            return r
    return check_range(range)


def check_batch_columns(bins, range, B, W, what):
    """:func:`check_columns` for a batch of ``B`` members: a 3-d ``range`` is ``(B, W, 2)``"""
    if range is not None and range.ndim == 3:
        if range.shape[:2] != (B, W):
            raise ValueError("range: one (lo, hi) for every one of the %d columns of every one of the %d members, shape (%d, %d, 2); "
                             "got %s" % (W, B, B, W, range.shape,))
        range = None
    check_columns(bins, range, W, what)


def shared_edges(bins, range):
    """whether every member of a batch has the same edges: the caller's own, or an integer ``bins`` over a ``range`` given once"""
    return not isinstance(bins, int) or (range is not None and range.ndim < 3)


def member_edges(bins, range, M, W, minmax):
    """-> the W edge arrays of ``M`` members, each ``(M, nb_d + 1)``: row ``m`` is what :func:`column_edges` gives member ``m`` --
    ``np.linspace(lo, hi, bins + 1)`` for an integer ``bins``, bit for bit (``lo == hi`` widened by 0.5 each way), else the
    caller's edges for every member.  ``range``: None (``minmax`` = ``(lo (M, W), hi (M, W))`` of every member's data), one
    ``(2,)`` / ``(W, 2)`` for all members, or ``(M, W, 2)``."""
    if not isinstance(bins, int):
        return [np.tile(e, (M, 1)) for e in column_edges(bins, None, W, None)]
    if range is None:
        lo, hi = (np.array(v, dtype=np.float64).reshape(M, W) for v in minmax)
    else:
        r = np.broadcast_to(range, (M, W, 2))
        lo, hi = r[..., 0].copy(), r[..., 1].copy()
    same = lo == hi
    lo[same] -= 0.5
    hi[same] += 0.5
    # np.linspace over arrays runs the scalar call's operations element by element (arange * step + start, the last value set to
    # stop) unless some step underflows to 0, where it takes another expression for ALL elements: then member by member
    if M * W == 0 or ((hi - lo) / bins == 0).any():
        rows = [column_edges(bins, np.stack([lo[m], hi[m]], axis=1), W, None) for m in np.arange(M)]
        return [np.stack([rows[m][d] for m in np.arange(M)]) if M else np.empty((0, bins + 1)) for d in np.arange(W)]
    e = np.linspace(lo, hi, bins + 1, axis=-1)                  # (M, W, bins + 1)
    return [np.ascontiguousarray(e[:, d, :]) for d in np.arange(W)]


def host_histograms_batch(x, edges, pair_edges, pairs):
    """the NumPy twin of ``emx_histograms_batch`` on the ``(M, n, W)`` samples ``x`` with the per-member ``edges`` / ``pair_edges`` of
    :func:`member_edges` -> ``(counts, pair_counts)``: per column ``(M, nb_d)``, per pair ``(M, pb_i, pb_j)``, int64"""
    M, _, W = x.shape
    per = [host_histograms(x[m], [e[m] for e in edges], None if pair_edges is None else [e[m] for e in pair_edges], pairs)
           for m in range(M)]
    counts = [np.stack([per[m][0][d] for m in range(M)]) for d in range(W)]
    pc = [np.stack([per[m][1][p] for m in range(M)]) for p in range(len(pairs))]
    return counts, pc


# ---- split-R-hat: the definition, the host fallback of get_rhat, and what get_rhat does with the device's two arrays --------
RHat = namedtuple("RHat", ["rhat", "within", "between", "nchains", "length"])
RHat.__doc__ = """The result of ``get_rhat`` / :func:`split_rhat`: ``rhat``, ``within`` and ``between`` of one shape (the last axis the
parameters, plus one for the log-prob column when asked for), ``nchains`` the number C of half-series in a group and ``length``
their length h.  ``rhat`` is ``np.sqrt((length - 1) / length + between / within)`` bit for bit."""

Evidence = namedtuple("Evidence", ["logz_ss", "err_ss", "logz_ti", "dlogz_ti", "err_ti", "log_ratios", "mean_logl", "tail", "block_logz_ss",
                                   "block_logz_ti", "betas", "nblocks", "block_length"])
Evidence.__doc__ = """The result of ``PTSampler.get_evidence`` / :func:`emcee_amd.pt.stepping_stone_log_evidence`, for ``G`` objects,
``T`` rungs and ``K = nblocks`` blocks of ``block_length`` selected steps: ``logz_ss`` ``(G,)`` the stepping-stone log-evidence and
``err_ss`` its Monte-Carlo error (the standard error of the ``K`` single-block estimates ``block_logz_ss`` ``(G, K)``; NaN for
``K = 1``); ``logz_ti`` / ``dlogz_ti`` thermodynamic integration and ptemcee's discretisation estimate, ``err_ti`` its Monte-Carlo
error from ``block_logz_ti`` ``(G, K)``; ``log_ratios`` ``(G, T - 1)`` the estimates of ``log Z(b[j]) / Z(b[j + 1])``;
``mean_logl`` ``(G, T)`` the mean log-likelihood of every rung; ``tail`` ``(G,)`` the part of ``logz_ss`` extrapolated from the
hottest rung to ``beta = 0`` (0 when the ladder ends there); ``betas`` ``(G, T)`` the ladder used."""

RHAT_DEFINITION = """The split-R-hat of Gelman and Rubin (BDA3 section 11.4, the Stan reference manual):

    * Selection: the one ``get_chain(discard, thin)`` makes, ``nt`` stored steps.  ``h = nt // 2``: every series is split into its
      first ``h`` selected samples and its last ``h``; the middle one is dropped when ``nt`` is odd.  ``nt < 4`` raises ``ValueError``.
    * A series is one walker's values of one parameter; a group holds ``C = 2 x (walkers pooled)`` half-series ("chains") of
      length ``h``.
    * For every group and parameter, with ``mu_c`` the chain means and ``s_c^2`` the chain variances (``ddof = 1``):
      ``within = mean_c s_c^2``, ``between = var_c(mu_c, ddof = 1)``, ``rhat = sqrt((h - 1) / h + between / within)``.
      A constant group gives 0 / 0 = NaN and a non-finite sample NaN; neither raises.
    * ``chains="walkers"``: every ensemble is its own group, its walkers the chains (the convention of the common emcee
      converters).  ``chains="members"`` pools replicates.
    * ``log_prob=True`` adds the same statistic of the stored log-prob series as one trailing column; a stored ``-inf`` gives NaN
      there and nowhere else."""


def rhat_of(within, between, length):
    """``np.sqrt((h - 1) / h + between / within)``: the one expression every ``rhat`` comes from"""
    h = int(length)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt((h - 1) / h + between / within)


def check_chains(chains, allowed):
    if chains not in allowed:
        raise ValueError("chains must be %s; got %r" % (" or ".join(repr(a) for a in allowed), chains))
    return chains


def check_rhat_length(nt):
    """-> h = nt // 2, or ValueError where fewer than 4 steps are selected"""
    if nt < 4:
        raise ValueError("the split R-hat needs at least 4 selected steps; got %d" % nt)
    return nt // 2


def split_rhat(x, log_prob=None, pool=False):
    """-> :class:`RHat` of the array ``x``: ``(nsteps, nwalkers, ndim)``, one ensemble, result shape ``(ndim,)``; or ``(nsteps, B,
    nwalkers, ndim)``, ``B`` ensembles -- each its own group, ``(B, ndim)``, or with ``pool=True`` all ``B nwalkers`` walkers one
    group, ``(ndim,)``.  ``log_prob`` (``x``'s shape without the last axis) adds its column last.  This is the definition that
    ``get_rhat`` computes next to the chain, and its fallback for chains kept on the host.

    %s

    The arithmetic is the device's, in NumPy's summation order, and holds far from the origin: a chain's variance is the
    corrected two-pass form ``(G - r^2 / h) / (h - 1)`` about a centre within rounding of the chain's own mean (its first sample
    plus the mean of the differences from it, so that a constant chain has variance 0 exactly), and ``between`` is the same form
    over the residual chain means about one chain's centre.  Nothing is relative to ``|mean|``."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim not in (3, 4):
        raise ValueError("x is (nsteps, nwalkers, ndim) or (nsteps, B, nwalkers, ndim); got shape %s" % (x.shape,))
    if pool and x.ndim != 4:
        raise ValueError("pool=True needs (nsteps, B, nwalkers, ndim); got shape %s" % (x.shape,))
    if log_prob is not None:
        lp = np.asarray(log_prob, dtype=np.float64)
        if lp.shape != x.shape[:-1]:
            raise ValueError("log_prob must have shape %s; got %s" % (x.shape[:-1], lp.shape))
        x = np.concatenate([x, lp[..., None]], axis=-1)
    nt, W = x.shape[0], x.shape[-1]
    h = check_rhat_length(nt)
    if x.ndim == 3 or pool:
        y = x.reshape(nt, 1, -1, W)                     # member-major, then walker: the first chain is member 0's walker 0
    else:
        y = x
    K = y.shape[2]
    C = 2 * K
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        z = np.stack([y[:h], y[nt - h:]], axis=3)       # (h, G, K, 2, W)
        x0 = z[0]
        mu0 = x0 + (z - x0).sum(axis=0) / h
        d = z - mu0
        r = d.sum(axis=0)
        var = ((d * d).sum(axis=0) - r * r / h) / (h - 1)
        e = (mu0 - mu0[:, :1, :1, :]) + r / h
        within = var.sum(axis=(1, 2)) / C
        e1 = e.sum(axis=(1, 2))
        between = ((e * e).sum(axis=(1, 2)) - e1 * e1 / C) / (C - 1)
    if x.ndim == 3 or pool:
        within, between = within[0], between[0]
    return RHat(rhat_of(within, between, h), within, between, C, h)


split_rhat.__doc__ = split_rhat.__doc__ % RHAT_DEFINITION
