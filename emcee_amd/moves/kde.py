"""KDEMove: proposals resampled from a Gaussian KDE of the complement (reference
``moves/kde.py:16-45``).  Host proposal (scipy), device accept/commit like every custom
split-ensemble move.  In the sampler's Philox mode (``EnsembleSampler(rng="philox")``) proposal and
log density ratio run on the device (``csrc/emx_walkkde.hip``) for the Scott, Silverman and scalar
bandwidth rules."""
import numpy as np

from .. import _lib
from .red_blue import RedBlueMove
from .walk import MAX_NDIM

__all__ = ["KDEMove"]


def kde_desc(bw_method, nsplits, randomize_split, ndim):
    """MoveDesc of a KDEMove for the device (Philox mode), or None (a callable or unknown bw_method, ndim > 128)."""
    if ndim > MAX_NDIM:
        return None
    if bw_method is None or (isinstance(bw_method, str) and bw_method == "scott"):
        rule, factor = _lib.KDE_BW_SCOTT, 0.0
    elif isinstance(bw_method, str) and bw_method == "silverman":
        rule, factor = _lib.KDE_BW_SILVERMAN, 0.0
    elif isinstance(bw_method, (int, float, np.integer, np.floating)) and not isinstance(bw_method, bool) and \
            np.isfinite(bw_method) and bw_method > 0:
        rule, factor = _lib.KDE_BW_SCALAR, float(bw_method)
    else:
        return None
    return _lib.MoveDesc(_lib.MOVE_KDE, int(nsplits), int(bool(randomize_split)), rule, factor, 0.0, 0.0, 0.0)


class KDEMove(RedBlueMove):
    """:param bw_method: bandwidth rule passed to ``scipy.stats.gaussian_kde``."""

    def __init__(self, bw_method=None, **kwargs):
        try:
            from scipy.stats import gaussian_kde  # noqa: F401
        except ImportError:
            raise ImportError("you need scipy.stats.gaussian_kde to use the KDEMove")
        self.bw_method = bw_method
        super(KDEMove, self).__init__(**kwargs)

    _philox_kind = _lib.MOVE_KDE

    def _philox_desc(self, ndim):
        return kde_desc(self.bw_method, self.nsplits, self.randomize_split, ndim)

    def get_proposal(self, s, c, random):
        from scipy.stats import gaussian_kde
        density = gaussian_kde(np.concatenate(c, axis=0).T, bw_method=self.bw_method)
        q = density.resample(len(s), random)
        log_ratio = density.logpdf(s.T) - density.logpdf(q)
        return q.T, log_ratio
