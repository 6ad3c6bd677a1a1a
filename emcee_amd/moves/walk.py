"""WalkMove: the Goodman & Weare "walk move" (reference ``moves/walk.py:10-42``).

In the sampler's Philox mode (``EnsembleSampler(rng="philox")``) the proposal runs on the device
(``csrc/emx_walkkde.hip``: ``q = x + sum_j w_j c_j`` over ``s`` helpers, or ``x + L z`` with the
Cholesky factor of the whole complement).  Everywhere else it is host code (a covariance of ``s``
helper walkers per updated walker and a ``multivariate_normal`` draw); the Metropolis accept and the
commit still run on the device through :meth:`RedBlueMove._propose_custom` / ``emx_accept_proposals``."""
import numpy as np

from .. import _lib
from .red_blue import RedBlueMove

__all__ = ["WalkMove"]

WALK_MAX_S = 1024       # helper walkers per update the device proposal takes (include/emx.h)
MAX_NDIM = 128          # ndim bound of the device WalkMove / KDEMove


def walk_desc(s, nsplits, randomize_split, ndim):
    """MoveDesc of a WalkMove for the device (Philox mode), or None: the host get_proposal."""
    if ndim > MAX_NDIM:
        return None
    if s is None:
        take = 0
    else:
        take = int(s)
        if take != s or take < 2 or take > WALK_MAX_S:
            return None
    return _lib.MoveDesc(_lib.MOVE_WALK, int(nsplits), int(bool(randomize_split)), take, 0.0, 0.0, 0.0, 0.0)


class WalkMove(RedBlueMove):
    """:param s: number of helper walkers (default: the whole complement)."""

    _philox_kind = _lib.MOVE_WALK

    def __init__(self, s=None, **kwargs):
        self.s = s
        super(WalkMove, self).__init__(**kwargs)

    def _philox_desc(self, ndim):
        return walk_desc(self.s, self.nsplits, self.randomize_split, ndim)

    def get_proposal(self, s, c, random):
        helpers = np.concatenate(c, axis=0)
        nc = len(helpers)
        take = nc if self.s is None else self.s
        q = np.empty_like(s)
        for k, here in enumerate(s):
            picked = random.choice(nc, take, replace=False)
            spread = np.atleast_2d(np.cov(helpers[picked], rowvar=0))
            q[k] = random.multivariate_normal(here, spread)
        return q, np.zeros(len(s), dtype=np.float64)
