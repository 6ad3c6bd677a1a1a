"""Posterior summaries of :class:`~emcee_amd.EnsembleBatch` chains: the host side.

The device (``emx_summary_batch``, ``csrc/emx_batch_summary.hip``) returns means, covariances, the best stored sample and
*order statistics* -- the k-th smallest stored value of every parameter of every member.  Quantiles are interpolated here from
those, with NumPy's default ("linear") rule: for ``n`` samples and a quantile ``q``, :func:`quantile_ranks` gives the two ranks
``lo`` / ``hi`` around the virtual index ``(n - 1) q`` and its fractional part ``g``, and :func:`lerp` -- NumPy's ``_lerp`` --
interpolates between the two order statistics.  Together they reproduce ``np.quantile(x, q)`` of NumPy 2.2 bit for bit.
"""
from collections import namedtuple

import numpy as np

__all__ = ["BatchSummary", "quantile_ranks", "lerp", "MAX_QUANTILES"]

MAX_QUANTILES = 16          # two ranks a quantile: the 32 ranks of one emx_summary_batch call

BatchSummary = namedtuple("BatchSummary", ["nsamples", "mean", "cov", "quantiles", "map_coords", "map_log_prob"])
BatchSummary.__doc__ = """The result of ``get_summary``: ``nsamples`` (selected steps x walkers), ``mean`` ``(..., ndim)``, ``cov``
``(..., ndim, ndim)`` (``ddof = 1``; None when not asked for), ``quantiles`` ``(..., nq, ndim)``, ``map_coords`` ``(..., ndim)`` and
``map_log_prob`` ``(...)``: the stored sample with the largest stored log-prob."""


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
