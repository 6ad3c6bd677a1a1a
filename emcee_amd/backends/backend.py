"""Backend: chain storage (reference ``backends/backend.py:11-237``), device-resident by default.

When a sampler drives the GPU path it attaches its :class:`DeviceEnsemble`: the chain
``(nsteps, nwalkers, ndim)``, the log-prob chain and the per-walker accept counters then live in
HBM (the half-step kernel appends to them directly) and ``get_value`` copies only the requested
``discard/thin`` slice to the host.  Without a device attached (user-written moves running
through ``Move.propose``) it is a plain in-memory store with the reference's ``save_step``."""
import numpy as np

from .. import autocorr
from .. import summary as _summary
from .._lib import EmxError
from ..state import State

__all__ = ["Backend"]


class Backend(object):
    """A backend that keeps the chain in memory (HBM when attached to a device ensemble)."""

    def __init__(self, dtype=None):
        self.initialized = False
        self.dtype = np.float64 if dtype is None else dtype
        self._dev = None

    # ---- lifecycle ----
    def reset(self, nwalkers, ndim):
        """Forget every stored sample and size the backend for ``(nwalkers, ndim)``."""
        self.nwalkers = int(nwalkers)
        self.ndim = int(ndim)
        self._iteration = 0
        self._accepted = np.zeros(self.nwalkers, dtype=self.dtype)
        self._chain = np.empty((0, self.nwalkers, self.ndim), dtype=self.dtype)
        self._log_prob = np.empty((0, self.nwalkers), dtype=self.dtype)
        self._blobs = None
        self.random_state = None
        self.initialized = True
        if self._dev is not None:
            self._dev.chain_reset()

    def _attach(self, ens):
        """Move storage to the device ensemble ``ens`` (idempotent)."""
        if self._dev is ens:
            return
        if self._dev is not None:
            self._detach()
        ens.chain_reset()
        if self._iteration > 0:
            raise RuntimeError("cannot attach a device to a backend that already holds host samples")
        self._dev = ens

    def _detach(self):
        """Pull everything to host arrays and drop the device."""
        if self._dev is None:
            return
        it = self.iteration
        self._chain = self._dev.chain_read(0, 0, it)
        self._log_prob = self._dev.chain_read(1, 0, it)
        if self._dev_nblobs():
            self._blobs = self._dev.chain_read(2, 0, it)
        self._accepted = self._dev.accepted_counts().astype(self.dtype)
        self._iteration = it
        self._dev = None

    # ---- reference attributes ----
    @property
    def iteration(self):
        if self._dev is not None:
            return self._dev.iteration()[0]
        return self._iteration

    @iteration.setter
    def iteration(self, v):
        self._iteration = v

    @property
    def accepted(self):
        if self._dev is not None:
            return self._dev.accepted_counts().astype(self.dtype)
        return self._accepted

    @accepted.setter
    def accepted(self, v):
        self._accepted = v

    @property
    def chain(self):
        if self._dev is not None:
            return self._dev.chain_read(0, 0, self.iteration)
        return self._chain

    @chain.setter
    def chain(self, v):
        self._chain = v

    @property
    def log_prob(self):
        if self._dev is not None:
            return self._dev.chain_read(1, 0, self.iteration)
        return self._log_prob

    @log_prob.setter
    def log_prob(self, v):
        self._log_prob = v

    def _dev_nblobs(self):
        """blobs a sample that the attached device keeps next to its chain (a DeviceFused target with nblobs); 0: none there"""
        return self._dev.nblobs() if self._dev is not None else 0

    @property
    def blobs(self):
        if self._dev_nblobs():
            return self._dev.chain_read(2, 0, self.iteration)
        return self._blobs

    @blobs.setter
    def blobs(self, v):
        self._blobs = v

    def has_blobs(self):
        """Whether blob storage has been set up (the log-prob function returns metadata)."""
        return self._blobs is not None or self._dev_nblobs() > 0

    def get_value(self, name, flat=False, thin=1, discard=0):
        it = self.iteration
        if it <= 0:
            raise AttributeError("you must run the sampler with 'store == True' before accessing the results")
        if name == "blobs" and not self.has_blobs():
            return None
        start = discard + thin - 1                     # reference backend.py:53
        if self._dev is not None and (name in ("chain", "log_prob") or (name == "blobs" and self._dev_nblobs())):
            v = self._dev.chain_read({"chain": 0, "log_prob": 1, "blobs": 2}[name], min(start, it), it, thin)
        else:
            v = getattr(self, name)[start:it:thin]
        if flat:
            s = list(v.shape[1:])
            s[0] = int(np.prod(v.shape[:2]))
            return v.reshape(s)
        return v

    def get_chain(self, **kwargs):
        """Stored samples, ``(nsteps, nwalkers, ndim)``.

        Keyword arguments (all optional): ``flat`` merges the step and walker axes, ``thin`` keeps
        every thin-th stored step, ``discard`` drops that many initial steps (burn-in)."""
        return self.get_value("chain", **kwargs)

    def get_blobs(self, **kwargs):
        """Stored blobs, one per walker and step (``None`` when the model has none); same
        ``flat`` / ``thin`` / ``discard`` keywords as :meth:`get_chain`."""
        return self.get_value("blobs", **kwargs)

    def get_log_prob(self, **kwargs):
        """Stored log-probabilities, ``(nsteps, nwalkers)``; same keywords as :meth:`get_chain`."""
        return self.get_value("log_prob", **kwargs)

    def get_last_sample(self):
        """The most recently stored step as a :class:`State` (with the RNG state saved alongside)."""
        if (not self.initialized) or self.iteration <= 0:
            raise AttributeError("you must run the sampler with 'store == True' before accessing the results")
        it = self.iteration
        blobs = self.get_blobs(discard=it - 1)
        if blobs is not None:
            blobs = blobs[0]
        return State(self.get_chain(discard=it - 1)[0], log_prob=self.get_log_prob(discard=it - 1)[0],
                     blobs=blobs, random_state=self.random_state)

    def get_autocorr_time(self, discard=0, thin=1, **kwargs):
        """Integrated autocorrelation time per parameter, in steps (reference backend.py:130-150).

        A device-resident chain is analysed where it lives (``emx_autocorr``: batched FFTs next to the chain, Sokal window,
        only ``ndim`` numbers come back); the reference's ``tol`` / ``quiet`` handling (autocorr.py:110-121) is applied here.
        Host-side chains (custom moves, blobs) go through :func:`emcee_amd.autocorr.integrated_time`."""
        only = {k: v for k, v in kwargs.items() if k in ("c", "tol", "quiet")}
        if self._dev is not None and kwargs.get("has_walkers", True) and len(only) == len(kwargs):
            c, tol, quiet = only.get("c", 5), only.get("tol", 50), only.get("quiet", False)
            try:
                tau_est, _, n_t = self._dev.autocorr(discard=discard, thin=thin, c=c)
            except EmxError as e:
                # libhipfft not loadable, no room for the work buffers next to a long chain, an empty selection ...: the host
                # estimator below computes the same numbers from a copy of the chain (and raises the reference's own errors)
                autocorr.logger.debug("device autocorrelation unavailable (%s): host estimator", e)
                tau_est = None
            if tau_est is not None:
                flag = tol * tau_est > n_t
                if np.any(flag):
                    msg = ("The chain is shorter than {0} times the integrated autocorrelation time for {1} parameter(s). "
                           "Use this estimate with caution and run a longer chain!\n").format(tol, np.sum(flag))
                    msg += "N/{0} = {1:.0f};\ntau: {2}".format(tol, n_t / tol, tau_est)
                    if not quiet:
                        raise autocorr.AutocorrError(tau_est, msg)
                    autocorr.logger.warning(msg)
                return thin * tau_est
        x = self.get_chain(discard=discard, thin=thin)
        return thin * autocorr.integrated_time(x, **kwargs)

    COV_MAX_DEVICE = 256        # columns of emx_summary's covariance

    def get_summary(self, discard=0, thin=1, quantiles=(0.16, 0.5, 0.84), cov=True):
        """-> :class:`~emcee_amd.summary.BatchSummary` of the stored samples over the steps of ``get_chain(discard=discard,
        thin=thin)`` and all walkers: ``nsamples``, ``mean`` ``(ndim,)``, ``cov`` ``(ndim, ndim)`` (``np.cov(flat.T)``, exactly
        symmetric; None with ``cov=False``), ``quantiles`` ``(nq, ndim)`` (``np.quantile``'s default rule, at most 16),
        ``map_coords`` ``(ndim,)`` / ``map_log_prob``: the stored sample with the largest stored log-prob, the earliest step and
        then the lowest walker among equals.

        A device-resident chain is reduced where it lives (``emx_summary``): only these numbers cross to the host.  A chain on
        the host (user-written moves, Python blobs) is reduced with NumPy into the same tuple, and so is a device chain whose
        call fails (no room for the scratch next to a long chain).  On the device ``cov=True`` needs ``ndim <= 256``.

        Far from the origin (|mean| / sd of 2^20 ... 2^40) only the device path keeps the mean to one rounding and the
        covariance to its summation error (a residual pass and the corrected two-pass form); the NumPy path is ``x.mean`` and
        ``np.cov`` bit for bit and loses what they lose."""
        return self._summary("chain", discard, thin, quantiles, cov)

    def get_blob_summary(self, discard=0, thin=1, quantiles=(0.16, 0.5, 0.84), cov=True):
        """-> :class:`~emcee_amd.summary.BatchSummary` of the stored BLOBS: what :meth:`get_summary` returns with the blobs of
        a sample in its coordinates' place (``map_coords``: the blobs of the sample with the largest stored log-prob).  The blob
        plane of a ``DeviceFused`` target is reduced on the device; blobs kept on the host must be plain floats of shape
        ``(nsteps, nwalkers)`` or ``(nsteps, nwalkers, K)`` (``TypeError`` otherwise).  ``ValueError`` when there are no blobs."""
        return self._summary("blobs", discard, thin, quantiles, cov)

    def _summary(self, name, discard, thin, quantiles, cov):
        if int(thin) != thin or thin < 1:
            raise ValueError("thin must be an integer >= 1; got %r" % (thin,))
        if int(discard) != discard or discard < 0:
            raise ValueError("discard must be an integer >= 0; got %r" % (discard,))
        q = _summary.check_quantiles(quantiles)
        thin, discard = int(thin), int(discard)
        it = self.iteration if self.initialized else 0
        if it <= 0:
            raise AttributeError("you must run the sampler with 'store == True' before accessing the results")
        if name == "blobs" and not self.has_blobs():
            raise ValueError("the target has no blobs (nblobs = 0): there is no blob plane to summarise")
        start = min(discard + thin - 1, it)                 # reference backend.py:53
        nt = len(range(start, it, thin))
        if nt < 1:
            raise ValueError("discard = %d, thin = %d select none of the %d stored steps" % (discard, thin, it))
        n = nt * self.nwalkers
        ranks, ilo, ihi, g = _summary.plan_ranks(n, q)
        on_device = self._dev is not None and (name == "chain" or self._dev_nblobs())
        if on_device:
            width = self.ndim if name == "chain" else self._dev_nblobs()
            if cov and width > self.COV_MAX_DEVICE:
                raise ValueError("the covariance of %d columns is not computed on the device (at most %d): pass cov=False"
                                 % (width, self.COV_MAX_DEVICE))
            try:
                nd, mean, c, order, mx, mlp = self._dev.summary(start, it, thin, ranks, cov, 0 if name == "chain" else 2)
            except EmxError as e:
                autocorr.logger.debug("device summary unavailable (%s): NumPy on a copy of the chain", e)
            else:
                assert nd == n
                return _summary.BatchSummary(n, mean, c, _summary.interpolate(order[None], ilo, ihi, g)[0], mx, mlp)
        x = self.get_value(name, discard=discard, thin=thin, flat=True)
        if name == "blobs":
            x = np.asarray(x)
            if x.dtype.kind != "f" or x.ndim not in (1, 2):
                raise TypeError("get_blob_summary needs plain float blobs of shape (nsteps, nwalkers) or (nsteps, nwalkers, K); "
                                "got dtype %s, shape %s a step" % (x.dtype, x.shape[1:]))
        x = np.asarray(x, dtype=np.float64).reshape(n, -1)
        lp = np.asarray(self.get_value("log_prob", discard=discard, thin=thin, flat=True))
        at = int(np.argmax(lp))                             # the first maximum in (step, walker) order
        with np.errstate(invalid="ignore", divide="ignore"):
            c = np.atleast_2d(np.cov(x.T)) if cov and n > 1 else np.full((x.shape[1], x.shape[1]), np.nan) if cov else None
        qs = np.quantile(x, q, axis=0) if len(q) else np.empty((0, x.shape[1]))
        return _summary.BatchSummary(n, x.mean(axis=0), c, qs, x[at].copy(), float(lp[at]))

    def get_rhat(self, discard=0, thin=1, chains="walkers", log_prob=False):
        """-> :class:`~emcee_amd.summary.RHat` ``(rhat, within, between, nchains, length)`` of the stored samples over the steps
        of ``get_chain(discard=discard, thin=thin)``, each array ``(ndim,)`` -- ``(ndim + 1,)`` with ``log_prob=True``.

        %s

        One ensemble is one group: only ``chains="walkers"`` is accepted here (``ValueError`` otherwise).  A device-resident
        chain is reduced where it lives (``emx_rhat``): ``within`` and ``between`` come from the device, ``rhat`` is formed from
        them on the host, and only these numbers cross.  A chain on the host (user-written moves, Python blobs) goes through
        :func:`emcee_amd.summary.split_rhat`, and so does a device chain whose call fails (no room for the scratch next to a
        long chain)."""
        _summary.check_chains(chains, ("walkers",))
        if int(thin) != thin or thin < 1:
            raise ValueError("thin must be an integer >= 1; got %r" % (thin,))
        if int(discard) != discard or discard < 0:
            raise ValueError("discard must be an integer >= 0; got %r" % (discard,))
        thin, discard = int(thin), int(discard)
        it = self.iteration if self.initialized else 0
        if it <= 0:
            raise AttributeError("you must run the sampler with 'store == True' before accessing the results")
        start = min(discard + thin - 1, it)                 # reference backend.py:53
        h = _summary.check_rhat_length(len(range(start, it, thin)))
        if self._dev is not None:
            try:
                within, between, nc, hd = self._dev.rhat(start, it, thin, log_prob)
            except EmxError as e:
                autocorr.logger.debug("device R-hat unavailable (%s): NumPy on a copy of the chain", e)
            else:
                assert hd == h and nc == 2 * self.nwalkers
                return _summary.RHat(_summary.rhat_of(within, between, h), within, between, nc, h)
        lp = self.get_value("log_prob", discard=discard, thin=thin) if log_prob else None
        return _summary.split_rhat(self.get_value("chain", discard=discard, thin=thin), log_prob=lp)

    def get_histograms(self, bins=64, range=None, discard=0, thin=1, pairs="all", pair_bins=None):
        """-> :class:`~emcee_amd.summary.Histograms`: the marginal histogram of every parameter and the 2-d histogram of every
        requested parameter pair (a corner plot's panels) over the steps of ``get_chain(discard=discard, thin=thin)`` and all
        walkers -- ``np.histogram`` / ``np.histogram2d`` count for count.

        ``bins``: an int (1 ... 1024) for every column, one strictly increasing edge array for every column, or a sequence of
        such arrays, one a column.  ``range`` (with an integer ``bins``): None (every column's min and max), ``(lo, hi)`` or
        ``(ndim, 2)``; the edges are ``np.linspace(lo, hi, bins + 1)``.  ``pairs``: ``"all"`` (every ``i < j``), None (marginals
        only) or a sequence of ``(i, j)``.  ``pair_bins``: as ``bins``, at most 128; None: ``min(bins, 64)`` over the same range,
        or the edges given as ``bins``.  A value falls in bin ``b`` iff ``edges[b] <= x < edges[b + 1]``, the last bin closed on
        the right; NaN and everything outside are counted nowhere.  A non-finite value in a column whose range is taken from
        the data raises ``ValueError``.

        A device-resident chain is counted where it lives (``emx_chain_minmax``, ``emx_histograms``): the chain is read once
        whatever the number of pairs and only the integer counts cross to the host.  A chain on the host (user-written moves,
        Python blobs) is counted with NumPy into the same tuple, and so is a device chain whose call fails (no room for the
        scratch next to a long chain)."""
        return self._histograms("chain", bins, range, discard, thin, pairs, pair_bins)

    def get_blob_histograms(self, bins=64, range=None, discard=0, thin=1, pairs="all", pair_bins=None):
        """-> :class:`~emcee_amd.summary.Histograms` of the stored BLOBS: what :meth:`get_histograms` returns with the blobs of a
        sample in its coordinates' place.  The blob plane of a ``DeviceFused`` target is counted on the device; blobs kept on the
        host must be plain floats of shape ``(nsteps, nwalkers)`` or ``(nsteps, nwalkers, K)`` (``TypeError`` otherwise).
        ``ValueError`` when there are no blobs."""
        return self._histograms("blobs", bins, range, discard, thin, pairs, pair_bins)

    def _histograms(self, name, bins, rng, discard, thin, pairs, pair_bins):
        if int(thin) != thin or thin < 1:
            raise ValueError("thin must be an integer >= 1; got %r" % (thin,))
        if int(discard) != discard or discard < 0:
            raise ValueError("discard must be an integer >= 0; got %r" % (discard,))
        thin, discard = int(thin), int(discard)
        bins = _summary.check_bins(bins, "bins", _summary.MAX_BINS)
        rng = _summary.check_range(rng)
        pairs = _summary.check_pairs(pairs)
        if pair_bins is not None:
            pair_bins = _summary.check_bins(pair_bins, "pair_bins", _summary.MAX_PAIR_BINS)
        elif isinstance(bins, int):
            pair_bins = min(bins, 64)
        if name == "chain" and self.initialized:                # the checks that need the number of columns
            _summary.check_columns(bins, rng, self.ndim, "bins")
            _summary.check_columns(pair_bins, None, self.ndim, "pair_bins")
            _summary.column_pairs(pairs, self.ndim)
        it = self.iteration if self.initialized else 0
        if it <= 0:
            raise AttributeError("you must run the sampler with 'store == True' before accessing the results")
        if name == "blobs" and not self.has_blobs():
            raise ValueError("the target has no blobs (nblobs = 0): there is no blob plane to histogram")
        start = min(discard + thin - 1, it)                 # reference backend.py:53
        nt = len(range(start, it, thin))
        if nt < 1:
            raise ValueError("discard = %d, thin = %d select none of the %d stored steps" % (discard, thin, it))
        n = nt * self.nwalkers
        on_device = self._dev is not None and (name == "chain" or self._dev_nblobs())
        x = None
        if on_device:
            W = self.ndim if name == "chain" else self._dev_nblobs()
        else:
            x = self.get_value(name, discard=discard, thin=thin, flat=True)
            if name == "blobs":
                x = np.asarray(x)
                if x.dtype.kind != "f" or x.ndim not in (1, 2):
                    raise TypeError("get_blob_histograms needs plain float blobs of shape (nsteps, nwalkers) or (nsteps, nwalkers, K); "
                                    "got dtype %s, shape %s a step" % (x.dtype, x.shape[1:]))
            x = np.asarray(x, dtype=np.float64).reshape(n, -1)
            W = x.shape[1]
        _summary.check_columns(bins, rng, W, "bins")
        _summary.check_columns(pair_bins, None, W, "pair_bins")
        pairs = _summary.column_pairs(pairs, W)
        if pair_bins is None:                               # the edges given as bins serve the panels too
            if len(pairs) and max(len(e) - 1 for e in (bins if isinstance(bins, list) else [bins])) > _summary.MAX_PAIR_BINS:
                raise ValueError("pair panels have at most %d bins a column: pass pair_bins, or pairs=None for the marginals alone"
                                 % _summary.MAX_PAIR_BINS)
            pair_bins = bins
        plane = 0 if name == "chain" else 2

        def finish(minmax, count):
            edges = _summary.column_edges(bins, rng, W, minmax)
            pedges = _summary.column_edges(pair_bins, rng, W, minmax)
            counts, pc = count(edges, pedges)
            return _summary.Histograms(n, edges, counts, pairs, pedges, pc)

        def finite(nonfinite):
            if np.any(nonfinite):
                raise ValueError("autodetected range of column(s) %s is not finite" % np.flatnonzero(nonfinite).tolist())

        auto = _summary.needs_minmax(bins, pair_bins, rng)
        if on_device:
            try:
                minmax = None
                if auto:
                    lo, hi, nf = self._dev.chain_minmax(start, it, thin, plane)
                    finite(nf)
                    minmax = (lo, hi)

                def count(edges, pedges):
                    nd, counts, pc = self._dev.histograms(start, it, edges, pedges, pairs, thin, plane)
                    assert nd == n
                    return counts, pc
                return finish(minmax, count)
            except EmxError as e:
                autocorr.logger.debug("device histograms unavailable (%s): NumPy on a copy of the chain", e)
            x = np.asarray(self.get_value(name, discard=discard, thin=thin, flat=True), dtype=np.float64).reshape(n, -1)
        minmax = None
        if auto:
            finite(~np.isfinite(x).all(axis=0))
            minmax = (x.min(axis=0), x.max(axis=0))
        return finish(minmax, lambda edges, pedges: _summary.host_histograms(x, edges, pedges, pairs))

    @property
    def shape(self):
        """``(nwalkers, ndim)`` of the ensemble this backend was reset for."""
        return self.nwalkers, self.ndim

    # ---- growth / saving ----
    def _check_blobs(self, blobs):
        if self._dev_nblobs():
            return                  # the device appends its own blob plane: nothing of the host's to keep consistent
        has_blobs = self.has_blobs()
        if has_blobs and blobs is None:
            raise ValueError("inconsistent use of blobs")
        if self.iteration > 0 and blobs is not None and not has_blobs:
            raise ValueError("inconsistent use of blobs")

    def grow(self, ngrow, blobs):
        """Make room for ``ngrow`` more steps (reference backend.py:164-185); ``blobs`` (the current
        blob array or None) fixes the blob dtype on first use."""
        self._check_blobs(blobs)
        it = self.iteration
        if self._dev is not None:
            self._dev.chain_config(it + ngrow)
            have = 0 if self._blobs is None else len(self._blobs)
        else:
            i = ngrow - (len(self._chain) - it)
            a = np.empty((i, self.nwalkers, self.ndim), dtype=self.dtype)
            self._chain = np.concatenate((self._chain, a), axis=0)
            a = np.empty((i, self.nwalkers), dtype=self.dtype)
            self._log_prob = np.concatenate((self._log_prob, a), axis=0)
            have = len(self._chain) - i
        if blobs is not None:
            i = it + ngrow - (0 if self._blobs is None else len(self._blobs))
            dt = np.dtype((blobs.dtype, blobs.shape[1:]))
            a = np.empty((max(i, 0), self.nwalkers), dtype=dt)
            self._blobs = a if self._blobs is None else np.concatenate((self._blobs, a), axis=0)
        del have

    def _check(self, state, accepted):
        """Shape / blob consistency of a step about to be saved (reference backend.py:187-212)."""
        self._check_blobs(state.blobs)
        nwalkers, ndim = self.shape
        expect = (
            (state.coords.shape == (nwalkers, ndim), "invalid coordinate dimensions; expected {0}".format((nwalkers, ndim))),
            (state.log_prob.shape == (nwalkers,), "invalid log probability size; expected {0}".format(nwalkers)),
            (state.blobs is None or self.has_blobs(), "unexpected blobs"),
            (state.blobs is not None or not self.has_blobs(), "expected blobs, but none were given"),
            (state.blobs is None or len(state.blobs) == nwalkers, "invalid blobs size; expected {0}".format(nwalkers)),
            (accepted.shape == (nwalkers,), "invalid acceptance size; expected {0}".format(nwalkers)),
        )
        for ok, message in expect:
            if not ok:
                raise ValueError(message)

    def save_step(self, state, accepted):
        """Append ``state`` and add ``accepted`` to the per-walker counters -- the host-side path
        (user-written moves, foreign samplers); reference backend.py:214-231."""
        if self._dev is not None:
            self._detach()
        self._check(state, accepted)
        self._chain[self._iteration, :, :] = state.coords
        self._log_prob[self._iteration, :] = state.log_prob
        if state.blobs is not None:
            self._blobs[self._iteration, :] = state.blobs
        self._accepted = self._accepted + accepted
        self.random_state = state.random_state
        self._iteration += 1

    @property
    def random_state(self):
        """RNG state after the last stored step.  During a device run the sampler hands over a provider (the MT19937
        state then lives in libemx and is only copied out when somebody asks)."""
        v = self._rstate
        return v() if callable(v) else v

    @random_state.setter
    def random_state(self, value):
        self._rstate = value

    def _device_step_saved(self, state_blobs, random_state):
        """Book-keeping after the kernel appended a step to the device chain."""
        if state_blobs is not None:
            self._blobs[self.iteration - 1, :] = state_blobs
        self.random_state = random_state

    def __getstate__(self):
        """Pickling materialises the device chain on the host (contexts are process-local)."""
        d = dict(self.__dict__)
        d["_rstate"] = self.random_state          # resolve a lazy provider
        if self._dev is not None:
            it = self.iteration
            d["_chain"] = self._dev.chain_read(0, 0, it)
            d["_log_prob"] = self._dev.chain_read(1, 0, it)
            if self._dev_nblobs():
                d["_blobs"] = self._dev.chain_read(2, 0, it)
            d["_accepted"] = self._dev.accepted_counts().astype(self.dtype)
            d["_iteration"] = it
            d["_dev"] = None
        return d

    def __setstate__(self, d):
        d = dict(d)
        if "blobs" in d:            # pickled before `blobs` became a property over `_blobs`
            d["_blobs"] = d.pop("blobs")
        self.__dict__.update(d)

    def __enter__(self):
        return self

    def __exit__(self, exception_type, exception_value, traceback):
        pass


Backend.get_rhat.__doc__ = Backend.get_rhat.__doc__ % _summary.RHAT_DEFINITION
