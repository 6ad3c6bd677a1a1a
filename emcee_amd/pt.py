"""Parallel tempering: one ensemble per rung of a temperature ladder, swaps between adjacent rungs on the device.

:class:`PTSampler` is the ptemcee algorithm (Vousden, Farr & Mandel 2016) for ``nbatch`` independent objects at once.  Group g
(one object of a catalogue) has ``ntemps`` ensembles of ``nwalkers`` walkers; rung t samples ``beta_t * L(x) + P(x)``.  They run
as the members of one :class:`~emcee_amd.EnsembleBatch` handle, member ``g * ntemps + t`` being rung t of group g, with the
user's :class:`~emcee_amd.targets.BatchCallable` / :class:`~emcee_amd.targets.BatchKernel` as the untempered likelihood.

Fused form.  A :class:`~emcee_amd.targets.PTFused` likelihood -- the user's per-row ``__device__`` likelihood and, optionally,
prior compiled into the tempered kernel ``k_pt_run`` (:func:`~emcee_amd.targets.compile_fused_pt`) -- runs one workgroup an
object: all its rungs in LDS, the half-steps of every rung side by side, the swap pass and the ladder update between workgroup
barriers, ONE launch per ``run_mcmc`` chunk of up to 4 096 steps.  Everything below holds unchanged, and the run is bit for bit the
``BatchKernel`` run of the same functions (while no proposal has a non-finite coordinate: the fused form rejects such a row without
calling a functor).  An object must fit one workgroup's LDS (``emx_pt_fused_check``); larger ones keep the callback path.
A ``PTFused(..., ndata=)`` likelihood (``compile_fused_pt(..., data=True)``) sums over the object's data with a wave a row.

Tempered log-probability.  ``lp = beta * L + P`` as two separate IEEE operations (no contraction).  At ``beta == 0``,
``lp = P``, so ``0 * -inf`` never occurs.  Where ``P == -inf`` the row's ``L`` is ignored (NaN included) and kept as ``-inf``.
The commit is :class:`~emcee_amd.EnsembleBatch`'s Metropolis rule on the tempered ``lp``; ``L`` and ``lp`` are kept per walker.
A NaN ``L`` where ``P`` is finite raises the reference's "Probability function returned NaN", naming the object and the rung.

Swap pass (ptemcee's order), after every ``swap_every``-th proposal step (``0``: never).  Pairs run from the hottest,
``i = ntemps-1 ... 1``.  Walker k of rung i is paired with walker ``pi_i(k)`` of rung i-1, and the swap is accepted when
``(beta_{i-1} - beta_i) * (L_i[k] - L_{i-1}[pi_i(k)]) > log u_{i,k}``; NaN (``-inf - -inf`` included) is rejected.  An accepted
swap exchanges ``x``, ``L`` and ``P`` and recomputes ``lp`` at both destinations.  Each pair sees the result of the pair
before it.  ``pi_i`` and ``u`` are keyed by group g's rung-0 Philox seed and the step just taken
(``emx_host_pt_swap_draws`` in ``include/emx.h`` rebuilds them on the host).

Blobs (``PTSampler(..., blobs=True)``).  A likelihood with ``nblobs = K`` (1 ... 32: a ``BatchCallable`` / ``BatchKernel`` /
``PTFused`` with ``nblobs``) produces K float64 values with every untempered ``L``; the prior produces none (a ``log_prior`` target
with blobs is a ``TypeError``).  Recording is asked for: without ``blobs=True`` a likelihood with blobs is refused with a
``TypeError``, as it always was, so that nobody pays for a plane they did not ask for.  A
walker's blobs are replaced exactly when its proposal is accepted by the tempered commit.  An accepted swap exchanges the blobs
together with ``x``, ``L`` and ``P``: a blob belongs to the point, not to the rung, so a blob that records ``member`` names the rung
where the point was last evaluated.  Where ``P == -inf`` the row's ``L`` is already ignored and kept as ``-inf``; its blobs are
likewise ignored and stored as NaN (the fused form never calls the likelihood there, the callback path calls it and discards the
result, and this rule makes the two equal); such a row can only be an initial-state walker.  The ladder update does not touch
blobs.  Coordinates, ``lp``, ``L``, ``P``, accept counts, swap counts, ladders and the Philox step of a run with blobs are bit for
bit those of the same function without blobs.  :meth:`get_blobs`, :meth:`get_blob_summary` and :meth:`get_blob_histograms` read the
blob plane next to the chain; ``get_last_sample().blobs`` the current state's.

Stored rows are the state after the step's swap pass: coordinates, tempered ``lp`` (:meth:`get_log_prob`), ``L``
(:meth:`get_log_likelihood`) and the blobs.  Accept counts are per member; swap attempts and accepts per (group, pair).

Seeds.  ``seeds`` holds ``nbatch`` integers.  Member (g, t) draws as the :class:`~emcee_amd.EnsembleBatch` member seeded with
``s[g, t] = np.random.RandomState(seeds[g]).randint(0, 2**32, size=ntemps, dtype=np.uint64)[t]``, i.e. its Philox seed is
``philox_seed(np.random.RandomState(s[g, t]))``.

Adaptive ladder (``adaptive=True``; ptemcee's rule, Vousden, Farr & Mandel 2016).  Each swap pass ends with an update of every
object's own ladder from that pass's accepted swaps, on the device (``emx_pt_set_adaptation`` in ``include/emx.h``): with
``r[j]`` the acceptance of pair ``j + 1`` in the pass and ``t`` the updates made before (:attr:`adaptation_updates`),
``kappa = (lag / (t + lag)) / time``, the temperature gaps ``1/b[j+1] - 1/b[j]`` are scaled by ``exp(kappa (r[j] - r[j+1]))`` and
the ladder rebuilt from rung 0; rungs 0 and ``ntemps - 1`` stay.  Pairs that accept more than their hotter neighbour widen,
so acceptance evens out along the ladder.  Two departures from ptemcee: the new betas are stored as computed (ptemcee adds the
difference), and the moved rungs' ``lp`` is recomputed as ``beta' L + P`` (ptemcee adds ``L dbeta``), which keeps the
two-roundings rule and the ``P = -inf`` / ``beta = 0`` cases.  :attr:`ladder` is the current ladder, :meth:`get_betas` the
ladder of every stored step; :attr:`betas` stays the initial one.  At most 256 rungs while adapting.

Evidence (:meth:`log_evidence_estimate`).  ``mean_logL[g, t]``, the mean of ``L`` over the stored steps after
``int(fburnin * iteration)`` and over all walkers, is computed on the device; thermodynamic integration over each object's
ladder (:func:`thermodynamic_integration_log_evidence`) gives ``log Z`` and ptemcee's error estimate.  The ladder must be
constant over those steps: freeze adaptation (``adaptive = False``) and discard the adaptive phase first.
:meth:`get_evidence` reduces the stored ``L`` plane next to the chain into per-block sums (``emx_pt_evidence``) and returns the
stepping-stone estimate (:func:`stepping_stone_log_evidence`, which states the definition) beside thermodynamic integration, each
with a Monte-Carlo error from consecutive blocks of the chain.
"""
import ctypes as C

import numpy as np

from . import _lib
from . import summary as _summary
from .batch import EnsembleBatch, _trampoline
from .ensemble import _refuse_extended_precision, walkers_independent
from .state import State
from .targets import BatchCallable, BatchFused, BatchKernel, BatchTarget, DeviceFused, DeviceTarget, PTFused

__all__ = ["PTSampler", "default_betas", "thermodynamic_integration_log_evidence", "stepping_stone_log_evidence"]

_ADAPT_MAX_T = 256          # k_pt_swap keeps an adapting ladder in LDS (PT_ADAPT_MAX_T)

_ILL = ("Initial state has a large condition number. Make sure that your walkers are linearly independent for the best "
        "performance")


def default_betas(ntemps, ndim, Tmax=None):
    """The default ladder: ``geomspace(1, 1/Tmax, ntemps)`` for a finite ``Tmax``; otherwise temperatures in the ratio
    ``1 + sqrt(2 / ndim)``, with a last rung at ``beta = 0`` when ``Tmax`` is ``np.inf``."""
    ntemps, ndim = int(ntemps), int(ndim)
    if ntemps < 1 or ndim < 1:
        raise ValueError("ntemps and ndim must be positive")
    if ntemps == 1:
        return np.ones(1)
    if Tmax is not None and np.isfinite(Tmax):
        if not Tmax > 1:
            raise ValueError("Tmax must be > 1; got %r" % (Tmax,))
        return np.geomspace(1.0, 1.0 / float(Tmax), ntemps)
    if Tmax is not None and Tmax != np.inf:
        raise ValueError("Tmax must be None, a finite number > 1 or np.inf; got %r" % (Tmax,))
    ratio = 1.0 + np.sqrt(2.0 / ndim)
    if Tmax is None:
        return ratio ** -np.arange(ntemps, dtype=np.float64)
    return np.concatenate([ratio ** -np.arange(ntemps - 1, dtype=np.float64), [0.0]])


def _check_betas(betas):
    betas = np.asarray(betas, dtype=np.float64).reshape(-1)
    if betas.size < 1 or betas[0] != 1.0:
        raise ValueError("betas[0] must be 1")
    if not np.all(np.isfinite(betas)) or betas[-1] < 0:
        raise ValueError("betas must be finite and >= 0")
    if np.any(np.diff(betas) >= 0):
        raise ValueError("betas must be strictly decreasing")
    return np.ascontiguousarray(betas)


def _trapezoid(y, x):
    return np.sum(0.5 * (x[..., 1:] - x[..., :-1]) * (y[..., 1:] + y[..., :-1]), axis=-1)


def _ti(betas, logls):
    """the rule on ladders (..., T) that all end at beta 0 or all end above it"""
    zero = np.zeros(betas.shape[:-1] + (1,))
    if betas[..., -1].flat[0] != 0:
        betas = np.concatenate([betas, zero], axis=-1)
        logls = np.concatenate([logls, logls[..., -1:]], axis=-1)
    betas2 = np.concatenate([betas[..., :-1:2], zero], axis=-1)
    logls2 = np.concatenate([logls[..., :-1:2], logls[..., -1:]], axis=-1)
    logz = -_trapezoid(logls, betas)
    logz2 = -_trapezoid(logls2, betas2)
    return logz, np.abs(logz - logz2)


def thermodynamic_integration_log_evidence(betas, logls):
    """ptemcee's estimate: ``logls[..., t]`` the mean log-likelihood at ``betas[..., t]`` (decreasing along the last axis).  When
    a ladder's last beta is > 0 a rung at ``beta = 0`` with the hottest rung's mean is appended.  -> ``(logZ, dlogZ)``: the
    negative trapezoid integral over the ladder, and its distance from the same integral over every other rung.  ``betas`` of
    shape ``(T,)`` serves every row of ``logls``; ``(..., T)`` (one ladder a row, e.g. :attr:`PTSampler.ladder`) broadcasts
    against ``logls``."""
    betas = np.asarray(betas, dtype=np.float64)
    logls = np.asarray(logls, dtype=np.float64)
    if betas.ndim <= 1:
        return _ti(betas, logls)
    betas, logls = np.broadcast_arrays(betas, logls)
    shape = betas.shape[:-1]
    fb, fl = betas.reshape(-1, betas.shape[-1]), logls.reshape(-1, logls.shape[-1])
    logz, dlogz = np.empty(len(fb)), np.empty(len(fb))
    last0 = fb[:, -1] == 0
    for sel in (last0, ~last0):          # the ladders that end at beta 0 and those that get the beta = 0 rung appended
        if sel.any():
            logz[sel], dlogz[sel] = _ti(fb[sel], fl[sel])
    return logz.reshape(shape), dlogz.reshape(shape)


EVIDENCE_DEFINITION = """The definition (``csrc/emx_pt_evidence.hip`` states the same):

    * Selection: the rows ``get_chain(discard, thin)`` selects, ``nt`` of them.  ``K = nblocks``, ``bl = nt // K``: the LAST
      ``K bl`` selected rows are used (the remainder is dropped at the early, burn-in end), cut into ``K`` consecutive blocks
      aligned in time across all rungs of an object.  ``bl < 1`` raises ``ValueError``; ``K = 1`` gives NaN errors.
    * Pair ``j`` (``0 ... T - 2``) covers rungs ``j`` and ``j + 1``: ``d = b[j] - b[j + 1]``; over the ``n = bl nwalkers`` values
      ``L`` of rung ``j + 1``, the hotter one, in block ``k``: ``a = d L``, ``M = max a``, ``S = sum exp(a - M)``; the block's
      log-ratio is ``M + log(S / n)``.  ``L = -inf`` contributes 0; a block of nothing else gives ``-inf``, never NaN; a NaN
      sample makes the block NaN.
    * The whole selection merges the blocks in block order: ``M* = max_k M``, ``S* = sum_k S_k exp(M_k - M*)``,
      ``log_ratios[g, j] = M* + log(S* / (K n))``: the forward stepping-stone estimate of ``Z(b[j]) / Z(b[j + 1])`` (Xie et al.
      2011), whose weights are bounded by the hotter rung's own maximum.
    * ``mean_logl[g, t]``: the blocks' sums of ``L`` added in block order, over ``K n``.  ``tail[g] = b[T - 1] mean_logl[g, T - 1]``
      when ``b[T - 1] > 0`` -- the extrapolation thermodynamic integration makes when it appends a rung at 0 -- else 0.
    * ``logz_ss = sum_j log_ratios[:, j] + tail`` (``j`` ascending); ``block_logz_ss[:, k]`` the same from block ``k`` alone;
      ``err_ss = std_k(block_logz_ss, ddof=1) / sqrt(K)``.  ``logz_ti, dlogz_ti =``
      :func:`thermodynamic_integration_log_evidence` ``(b, mean_logl)``, ``block_logz_ti`` the same from each block's means,
      ``err_ti`` formed like ``err_ss``.  With one rung there are no pairs: ``logz_ss = tail``."""


def _check_nblocks(nblocks):
    if isinstance(nblocks, (bool, np.bool_)) or int(nblocks) != nblocks or nblocks < 1:
        raise ValueError("nblocks must be an integer >= 1; got %r" % (nblocks,))
    return int(nblocks)


def _block_length(nt, K):
    if nt // K < 1:
        raise ValueError("nblocks = %d blocks need at least as many selected steps; got %d" % (K, nt))
    return nt // K


def _std_error(blocks):
    """std over the last axis (ddof = 1) / sqrt(K); NaN for K = 1"""
    K = blocks.shape[-1]
    if K < 2:
        return np.full(blocks.shape[:-1], np.nan)
    with np.errstate(invalid="ignore"):
        return np.std(blocks, axis=-1, ddof=1) / np.sqrt(K)


def _evidence_from_blocks(b, A, M, S, bl, n):
    """the host's half of the definition: the ladders ``b`` (G, T), the blocks' sums of L ``A`` (G, T, K) and the pairs' ``M`` and
    ``S`` (G, T - 1, K) of blocks of ``n`` samples -> :class:`~emcee_amd.summary.Evidence`"""
    G, T, K = A.shape
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        block_lr = M + np.log(S / n)                                        # (G, T - 1, K)
        Ms = np.fmax.reduce(M, axis=-1, initial=-np.inf)
        w = np.where(M == -np.inf, S, S * np.exp(M - Ms[..., None]))        # a block without weight holds 0 (NaN for a NaN sample)
        Ss, tot = np.zeros((G, T - 1)), np.zeros((G, T))
        for k in range(K):
            Ss = Ss + w[..., k]
            tot = tot + A[..., k]
        log_r = Ms + np.log(Ss / (K * n))
        mean = tot / (K * n)
        block_mean = A / n                                                  # (G, T, K)
        ends_above = b[:, -1] > 0
        tail = np.where(ends_above, b[:, -1] * np.where(ends_above, mean[:, -1], 0.0), 0.0)
        block_tail = np.where(ends_above[:, None], b[:, -1:] * np.where(ends_above[:, None], block_mean[:, -1], 0.0), 0.0)
        logz, block_logz = np.zeros(G), np.zeros((G, K))
        for j in range(T - 1):
            logz = logz + log_r[:, j]
            block_logz = block_logz + block_lr[:, j]
        logz, block_logz = logz + tail, block_logz + block_tail
        ti, dti = thermodynamic_integration_log_evidence(b, mean)
        block_ti = np.stack([thermodynamic_integration_log_evidence(b, block_mean[..., k])[0] for k in range(K)], axis=-1)
    return _summary.Evidence(logz, _std_error(block_logz), ti, dti, _std_error(block_ti), log_r, mean, tail, block_logz, block_ti, b, K,
                             int(bl))


def stepping_stone_log_evidence(betas, logls, nblocks=8):
    """-> :class:`~emcee_amd.summary.Evidence` from stored log-likelihoods: ``logls`` ``(..., T, nsteps, nwalkers)`` (e.g.
    :meth:`PTSampler.get_log_likelihood`), ``betas`` ``(T,)`` or ``(..., T)``, decreasing.  :meth:`PTSampler.get_evidence` computes
    the same next to the chain; this is its definition on arrays.  The leading axes ``...`` are flattened into ``G``.

    %s"""
    logls = np.asarray(logls, dtype=np.float64)
    if logls.ndim < 3:
        raise ValueError("logls is (..., T, nsteps, nwalkers); got shape %s" % (logls.shape,))
    K = _check_nblocks(nblocks)
    T, nt, N = logls.shape[-3:]
    bl = _block_length(nt, K)
    n = bl * N
    betas = np.asarray(betas, dtype=np.float64)
    if betas.shape[-1:] != (T,):
        raise ValueError("betas holds %s values a ladder for %d rungs" % (betas.shape[-1:], T))
    b = np.ascontiguousarray(np.broadcast_to(betas, logls.shape[:-2])).reshape(-1, T)
    x = logls.reshape((-1, T, nt, N))[:, :, nt - K * bl:].reshape(-1, T, K, n)
    with np.errstate(invalid="ignore", over="ignore"):
        A = x.sum(axis=-1)
        d = b[:, :-1] - b[:, 1:]
        a = d[:, :, None, None] * x[:, 1:]
        M = np.fmax.reduce(a, axis=-1, initial=-np.inf)                     # a NaN is passed over here and met in S
        S = np.where(a == -np.inf, 0.0, np.exp(a - M[..., None])).sum(axis=-1)
    return _evidence_from_blocks(b, A, M, S, bl, n)


stepping_stone_log_evidence.__doc__ %= EVIDENCE_DEFINITION


class PTSampler(object):
    """``nbatch`` independent parallel-tempered ensembles: ``ntemps`` rungs of ``nwalkers`` walkers in ``ndim`` dimensions each.

    ``log_likelihood``: a :class:`~emcee_amd.targets.BatchCallable` (``fn(q)`` gets a ``(nbatch, ntemps, R, ndim)`` view of the
    proposal block and returns ``(nbatch, ntemps, R)``) or a :class:`~emcee_amd.targets.BatchKernel` (``nbatch * ntemps`` members
    in (object, rung) order), evaluated untempered.  ``log_prior``: None (flat, improper), ``(lo, hi)`` (a box the kernel
    evaluates: 0 inside, -inf outside), or a BatchCallable / BatchKernel called on the same block before the likelihood.
    A :class:`~emcee_amd.targets.PTFused` likelihood (module docstring) takes ``log_prior`` None or ``(lo, hi)`` only, and neither
    when its launcher carries a prior functor.
    ``betas``: strictly decreasing from 1 to >= 0, else :func:`default_betas` ``(ntemps, ndim, Tmax)``; every object starts on
    it.  ``moves``: the schedule forms of :class:`~emcee_amd.EnsembleBatch`'s callback path.  ``adaptive``: adapt each object's
    ladder after every swap pass (module docstring; ptemcee's ``adaptation_lag`` and ``adaptation_time``, both > 0).
    ``adaptive`` and ``swap_every`` may be changed between runs.  ``blobs=True``: record the blobs of a likelihood with ``nblobs >
    0`` (module docstring, "Blobs"); without it such a likelihood is refused."""

    def __init__(self, ntemps, nwalkers, ndim, log_likelihood, log_prior=None, betas=None, Tmax=None, nbatch=1, moves=None,
                 seeds=None, swap_every=1, device=None, rng="philox", adaptive=False, adaptation_lag=10000, adaptation_time=100,
                 blobs=False):
        if rng != "philox":
            raise ValueError("PTSampler runs rng='philox' only (the MT19937 stream is made by one host generator a sampler; use "
                             "EnsembleSampler for rng=%r)" % (rng,))
        self.ntemps, self.nwalkers, self.ndim, self.nbatch = int(ntemps), int(nwalkers), int(ndim), int(nbatch)
        if min(self.ntemps, self.nwalkers, self.ndim, self.nbatch) < 1:
            raise ValueError("ntemps, nwalkers, ndim and nbatch must be positive")
        if isinstance(log_likelihood, BatchFused):
            raise TypeError("PTSampler's log_likelihood is a targets.BatchCallable or targets.BatchKernel; a BatchFused is not: the "
                            "tempered commit and the swap pass run on the batched callback path (a fused tempered kernel does not exist)")
        if isinstance(log_likelihood, DeviceFused):
            raise TypeError("PTSampler's log_likelihood is a targets.BatchCallable, targets.BatchKernel or targets.PTFused; a DeviceFused "
                            "is not: its launcher carries the single sampler's half-step kernel (compile the model as a PTFused)")
        if isinstance(log_likelihood, BatchTarget):
            nb = int(getattr(log_likelihood, "nblobs", 0))
            if nb > 0 and not blobs:
                raise TypeError("PTSampler records blobs only when asked to: pass blobs=True to keep the %d blobs a sample of this "
                                "log_likelihood next to the chain (nblobs = %d), or give a target with nblobs = 0" % (nb, nb))
            if blobs and nb == 0:
                raise ValueError("blobs=True needs a log_likelihood that produces blobs (a target with nblobs > 0); got nblobs = 0")
        if not isinstance(log_likelihood, BatchTarget):
            kind = "fused device target" if isinstance(log_likelihood, DeviceTarget) else type(log_likelihood).__name__
            raise TypeError("PTSampler's log_likelihood is a targets.BatchCallable or targets.BatchKernel; a %s is not (wrap the "
                            "model in BatchCallable)" % kind)
        fused = isinstance(log_likelihood, PTFused)
        if fused and log_likelihood.ndim != self.ndim:
            raise ValueError("the PTFused target was compiled for ndim %d; the sampler has ndim %d" % (log_likelihood.ndim, self.ndim))
        self.betas = _check_betas(betas) if betas is not None else default_betas(self.ntemps, self.ndim, Tmax)
        if len(self.betas) != self.ntemps:
            raise ValueError("betas holds %d rungs for ntemps = %d" % (len(self.betas), self.ntemps))
        self._box, self._prior = None, None
        if log_prior is not None:
            if isinstance(log_prior, BatchFused):
                raise TypeError("log_prior is None, (lo, hi) or a targets.BatchCallable / BatchKernel; a BatchFused is not")
            if fused and log_likelihood.has_prior:
                raise ValueError("the PTFused launcher carries a prior functor: log_prior must be None")
            if fused and isinstance(log_prior, BatchTarget):
                raise TypeError("with a PTFused likelihood log_prior is None or (lo, hi): a BatchCallable / BatchKernel prior would need "
                                "the callback path (compile the prior into the launcher: compile_fused_pt(..., prior=...))")
            if isinstance(log_prior, BatchTarget) and getattr(log_prior, "nblobs", 0) > 0:
                raise TypeError("log_prior is a target with nblobs = 0: the prior produces no blobs, the likelihood does (got nblobs = %d)"
                                % log_prior.nblobs)
            if isinstance(log_prior, BatchTarget):
                self._prior = log_prior
            elif isinstance(log_prior, DeviceTarget) or callable(log_prior):
                raise TypeError("log_prior is None, (lo, hi) or a targets.BatchCallable / BatchKernel")
            else:
                lo, hi = (np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1)) for v in log_prior)
                if lo.shape != (self.ndim,) or hi.shape != (self.ndim,):
                    raise ValueError("a box prior is (lo, hi) of ndim = %d values each" % self.ndim)
                if not np.all(lo <= hi):
                    raise ValueError("a box prior needs lo <= hi")
                self._box = (lo, hi)
        self.swap_every = int(swap_every)
        if self.swap_every < 0:
            raise ValueError("swap_every must be >= 0 (0: never)")
        self.adaptation_lag, self.adaptation_time = float(adaptation_lag), float(adaptation_time)
        for name, v in (("adaptation_lag", self.adaptation_lag), ("adaptation_time", self.adaptation_time)):
            if not (np.isfinite(v) and v > 0):
                raise ValueError("%s must be finite and > 0; got %r" % (name, v))
        self.adaptive = bool(adaptive)
        if self.adaptive:
            self._check_adaptive()
        if seeds is None:
            seeds = np.random.randint(0, 2 ** 32, size=self.nbatch, dtype=np.uint64)
        seeds = [int(s) for s in np.asarray(seeds).reshape(-1)]
        if len(seeds) != self.nbatch:
            raise ValueError("seeds must hold nbatch = %d integers; got %d" % (self.nbatch, len(seeds)))
        self.seeds = seeds
        self.member_seeds = np.stack([np.random.RandomState(s).randint(0, 2 ** 32, size=self.ntemps, dtype=np.uint64)
                                      for s in seeds])
        self._b = EnsembleBatch(self.nbatch * self.ntemps, self.nwalkers, self.ndim, self._wrap(log_likelihood), moves=moves,
                                seeds=self.member_seeds.reshape(-1), device=device, _tempered=True, _ntemps=self.ntemps)
        self._fused = log_likelihood if fused else None
        self.nblobs = self._b.nblobs        # blobs a sample of the likelihood (0: none)
        if fused:           # an object must fit one workgroup's LDS: refused here, before any device is touched
            msg = C.create_string_buffer(512)
            d = self._b._descs
            arr = (_lib.MoveDesc * len(d))(*d)
            if _lib.load().emx_pt_fused_check_blobs(self.ntemps, self.nwalkers, self.ndim, len(d), arr, self.nblobs, msg, 512) != 0:
                raise ValueError("PTSampler: %s" % msg.value.decode())
        self.device = self._b.device
        self._h = None
        self._prior_keep = None

    def _check_adaptive(self):
        if self.ntemps > _ADAPT_MAX_T:
            raise ValueError("an adaptive ladder has at most %d rungs; ntemps = %d" % (_ADAPT_MAX_T, self.ntemps))
        if self.ntemps > 1 and not self.betas[-2] > 0:
            raise ValueError("an adaptive ladder needs betas[0 ... ntemps - 2] > 0")

    def _wrap(self, t):
        """a BatchCallable's fn sees (nbatch, ntemps, R, ndim) -- and, with nblobs = K, returns (lp, blobs) of shapes (nbatch, ntemps,
        R) and (nbatch, ntemps, R, K); a BatchKernel the handle's members as they are"""
        if isinstance(t, (BatchKernel, PTFused)):
            return t
        fn, G, T, D, K = t.fn, self.nbatch, self.ntemps, self.ndim, t.nblobs
        if not K:
            return BatchCallable(lambda q: fn(q.view(G, T, q.shape[1], D)))

        def with_blobs(q):
            R = q.shape[1]
            res = fn(q.view(G, T, R, D))
            if not (isinstance(res, (tuple, list)) and len(res) == 2):
                raise ValueError("with nblobs = %d the likelihood returns (log_likelihood, blobs); got %s" % (K, type(res).__name__))
            lp, bl = res
            got = tuple(bl.shape) if hasattr(bl, "shape") else np.shape(bl)
            if got != (G, T, R, K):
                raise ValueError("the likelihood returned blobs of shape %s; expected (nbatch, ntemps, rows, nblobs) = %s" % (got, (G, T, R, K)))
            return lp, bl.reshape(G * T, R, K)
        return BatchCallable(with_blobs, nblobs=K)

    # ------------------------------------------------------------------ device plumbing
    def _ck(self, rc):
        self._b._ck(rc)

    def _handle(self):
        lib = _lib.load()
        if self._h is None:
            h = self._b._handle()
            ptr = (lambda a: None if a is None else a.ctypes.data_as(C.c_void_p))
            lo, hi = self._box if self._box is not None else (None, None)
            rc = lib.emx_pt_set_tempering(h, self.ntemps, self.betas, ptr(lo), ptr(hi))
            if rc != 0 and self._fused is not None and b"carries a prior functor" in lib.emx_batch_last_error(h):
                raise ValueError("the PTFused launcher carries a prior functor: log_prior must be None")
            self._ck(rc)
            if self._prior is not None:
                p = self._wrap(self._prior)
                if isinstance(p, BatchKernel):
                    fn = p.fn_ptr if isinstance(p.fn_ptr, _lib.BATCH_LOG_PROB_FN) else C.cast(p.fn_ptr, _lib.BATCH_LOG_PROB_FN)
                    user = p.user_ptr if isinstance(p.user_ptr, C.c_void_p) else C.c_void_p(p.user_ptr)
                else:
                    fn, user = _lib.BATCH_LOG_PROB_FN(_trampoline(p.fn, self.device, self._b._cb_box)), None
                self._prior_keep = fn
                self._ck(lib.emx_set_batch_prior_callback(h, fn, user))
            if self.nblobs and self._fused is None:      # a callback with blobs is bound to the handle once it is tempered
                self._b._bind_callback(h, tempered=True)
            self._h = h
        self._ck(lib.emx_pt_set_swap_every(self._h, self.swap_every))
        if self.adaptive:
            self._check_adaptive()
        self._ck(lib.emx_pt_set_adaptation(self._h, int(bool(self.adaptive)), self.adaptation_lag, self.adaptation_time))
        return self._h

    def _who(self, m):
        return "object %d, rung %d" % divmod(int(m), self.ntemps)

    def _raise_on_status(self, what):
        bits = np.zeros(self.nbatch * self.ntemps, dtype=np.uint32)
        self._ck(_lib.load().emx_batch_status(self._h, bits))
        bad = np.flatnonzero(bits)
        if len(bad):
            m = int(bad[0])
            text = ("At least one parameter value was infinite or NaN" if bits[m] & 2 else
                    "The initial log_prob was NaN" if what == "eval" else "Probability function returned NaN")
            more = "" if len(bad) == 1 else " (and %d more members)" % (len(bad) - 1)
            raise ValueError("(%s): %s%s" % (self._who(m), text, more))

    def set_tuning(self, key, value):
        """as :meth:`EnsembleBatch.set_tuning`"""
        self._b.set_tuning(key, value)

    def launch_info(self):
        """-> dict(threads, plan_steps, launches): the last launch's shape and the library's launches so far."""
        return self._b.launch_info()

    def close(self):
        self._b.close()
        self._h = None

    # ------------------------------------------------------------------ sampling
    def _check_state(self, coords):
        coords = np.asarray(coords)
        _refuse_extended_precision(coords)
        want = (self.nbatch, self.ntemps, self.nwalkers, self.ndim)
        if coords.shape != want:
            raise ValueError("incompatible input dimensions %s: expected (nbatch, ntemps, nwalkers, ndim) = %s" % (coords.shape, want))
        coords = np.ascontiguousarray(coords, dtype=np.float64)
        for g in range(self.nbatch):
            for t in range(self.ntemps):
                if not np.all(np.isfinite(coords[g, t])):
                    raise ValueError("(object %d, rung %d): %s" % (g, t, "At least one parameter value was infinite"
                                     if np.any(np.isinf(coords[g, t])) else "At least one parameter value was NaN"))
        return coords

    def run_mcmc(self, initial_state, nsteps, thin_by=1, store=True, skip_initial_state_check=False):
        """Advance every rung of every object ``nsteps`` stored steps (``nsteps * thin_by`` proposals, each followed by the swap
        pass on the ``swap_every`` cadence) -> :class:`State` with ``(nbatch, ntemps, nwalkers, ndim)`` coordinates and the
        tempered ``(nbatch, ntemps, nwalkers)`` log-probs.  ``initial_state``: ``(nbatch, ntemps, nwalkers, ndim)`` or None to
        continue.  Checks as :meth:`EnsembleBatch.run_mcmc`; errors name ``(object, rung)``."""
        nsteps, thin_by = int(nsteps), int(thin_by)
        if thin_by <= 0:
            raise ValueError("Invalid thinning argument")
        if nsteps < 0:
            raise ValueError("nsteps must be >= 0")
        b = self._b
        coords = None
        if initial_state is None:
            if not b._ran:
                raise ValueError("Cannot have `initial_state=None` if run_mcmc has never been called.")
        else:
            coords = self._check_state(initial_state.coords if isinstance(initial_state, State) else initial_state)
            if not skip_initial_state_check:
                for g in range(self.nbatch):
                    for t in range(self.ntemps):
                        if not walkers_independent(coords[g, t]):
                            raise ValueError("(object %d, rung %d): %s" % (g, t, _ILL))
        for m in b._moves:
            if self.nwalkers < 2 * self.ndim and hasattr(m, "nsplits") and not getattr(m, "live_dangerously", False):
                raise RuntimeError("It is unadvisable to use a red-blue move with fewer walkers than twice the number of dimensions.")
        lib = _lib.load()
        h = self._handle()
        if coords is not None:
            self._ck(lib.emx_batch_set_state(h, coords.reshape(-1, self.nwalkers, self.ndim), None))
            self._ck(lib.emx_batch_eval_state_log_prob(h))
            self._raise_on_status("eval")
            b._ran = True
        if store:
            self._ck(lib.emx_batch_chain_config(h, self.iteration + nsteps))
        self._ck(lib.emx_batch_run(h, nsteps, thin_by, int(bool(store))))
        b._sync_moves()
        step = C.c_uint64(0)
        self._ck(lib.emx_batch_get_philox(h, np.zeros(self.nbatch * self.ntemps, dtype=np.uint64), C.byref(step)))
        b._step = step.value
        self._raise_on_status("run")
        return self.get_last_sample()

    def _swap(self):
        """one swap pass on the current state with the last step's draws (emx_pt_swap; tests)"""
        self._ck(_lib.load().emx_pt_swap(self._handle()))

    def _pt_state(self):
        """-> (L, P), each (nbatch, ntemps, nwalkers)"""
        L = np.empty((self.nbatch, self.ntemps, self.nwalkers))
        P = np.empty_like(L)
        self._ck(_lib.load().emx_pt_get_state(self._handle(), L, P))
        return L, P

    def _pt_blobs(self):
        """-> the current state's blobs (nbatch, ntemps, nwalkers, nblobs) (emx_pt_get_blobs), None without blobs"""
        if not self.nblobs:
            return None
        out = np.empty((self.nbatch, self.ntemps, self.nwalkers, self.nblobs))
        self._ck(_lib.load().emx_pt_get_blobs(self._handle(), out))
        return out

    def _set_pt_state(self, coords, L, P):
        """set (coords, L, P) and lp from them (emx_pt_set_state; tests).  The blobs of a likelihood that has them become NaN: the
        state bypasses the likelihood."""
        f = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
        self._ck(_lib.load().emx_pt_set_state(self._handle(), f(coords), f(L), f(P)))

    # ------------------------------------------------------------------ results
    @property
    def iteration(self):
        """Stored steps of every rung."""
        return self._b.iteration

    def _read(self, what, discard, thin, flat):
        out = self._b._read(what, 0, self.nbatch * self.ntemps, discard, thin, flat)
        return out.reshape((self.nbatch, self.ntemps) + out.shape[1:])

    def get_chain(self, discard=0, thin=1, flat=False):
        """``(nbatch, ntemps, nsteps, nwalkers, ndim)``; ``flat`` -> ``(nbatch, ntemps, nsteps * nwalkers, ndim)``."""
        return self._read(0, discard, thin, flat)

    def get_log_prob(self, discard=0, thin=1, flat=False):
        """the tempered log-probs, ``(nbatch, ntemps, nsteps, nwalkers)``."""
        return self._read(1, discard, thin, flat)

    def get_log_likelihood(self, discard=0, thin=1, flat=False):
        """the untempered log-likelihoods, ``(nbatch, ntemps, nsteps, nwalkers)``."""
        return self._read(2, discard, thin, flat)

    def get_blobs(self, discard=0, thin=1, flat=False):
        """the blobs stored with every sample, ``(nbatch, ntemps, nsteps, nwalkers, nblobs)``; ``flat`` -> ``(nbatch, ntemps, nsteps *
        nwalkers, nblobs)``.  None when the likelihood has no blobs."""
        if not self.nblobs:
            return None
        return self._read(4, discard, thin, flat)

    def get_betas(self, discard=0, thin=1):
        """the ladder of every stored step, ``(nbatch, nsteps, ntemps)`` (each row as stored: after the step's swap pass and
        ladder update)."""
        it = self.iteration
        if it <= 0:
            raise AttributeError("you must run the sampler with 'store == True' before accessing the results")
        thin, discard = int(thin), int(discard)
        start = min(discard + thin - 1, it)
        nsel = len(range(start, it, thin))
        out = np.empty((self.nbatch * self.ntemps, nsel))
        if nsel:
            self._ck(_lib.load().emx_batch_chain_read(self._h, 3, 0, self.nbatch * self.ntemps, start, it, thin, out))
        return np.ascontiguousarray(out.reshape(self.nbatch, self.ntemps, nsel).transpose(0, 2, 1))

    @property
    def ladder(self):
        """``(nbatch, ntemps)``: every object's current ladder (:attr:`betas` for each before the first run)."""
        if self._h is None:
            return np.tile(self.betas, (self.nbatch, 1))
        out = np.empty((self.nbatch, self.ntemps))
        self._ck(_lib.load().emx_pt_get_ladder(self._h, out.ctypes.data_as(C.c_void_p), None))
        return out

    @property
    def adaptation_updates(self):
        """the ladder updates made so far (the counter ``t`` of the adaptation rule; one per swap pass while adapting)."""
        if self._h is None:
            return 0
        t = C.c_int64(0)
        self._ck(_lib.load().emx_pt_get_ladder(self._h, None, C.byref(t)))
        return t.value

    @property
    def acceptance_fraction(self):
        """``(nbatch, ntemps, nwalkers)``"""
        return self._b.acceptance_fraction.reshape(self.nbatch, self.ntemps, self.nwalkers)

    def _swap_counts(self):
        att = np.zeros((self.nbatch, max(self.ntemps - 1, 0)), dtype=np.uint64)
        acc = np.zeros_like(att)
        if self._h is not None and self.ntemps > 1:
            self._ck(_lib.load().emx_pt_swap_counts(self._h, att, acc))
        return att, acc

    @property
    def tswap_acceptance_fraction(self):
        """``(nbatch, ntemps - 1)``: accepted / attempted swaps of each pair (rung i with i + 1); 0 before any attempt."""
        att, acc = self._swap_counts()
        return np.where(att > 0, acc / np.maximum(att, 1).astype(np.float64), 0.0)

    def get_autocorr_time(self, discard=0, thin=1, c=5, tol=50, quiet=False, on_device=True):
        """``(nbatch, ntemps, ndim)``: :meth:`EnsembleBatch.get_autocorr_time` of every rung (``emx_autocorr_batch`` on the
        device by default)."""
        tau = self._b.get_autocorr_time(discard=discard, thin=thin, c=c, tol=tol, quiet=quiet, on_device=on_device)
        return tau.reshape(self.nbatch, self.ntemps, self.ndim)

    def get_summary(self, discard=0, thin=1, quantiles=(0.16, 0.5, 0.84), cov=True):
        """:meth:`EnsembleBatch.get_summary` of every rung, with ``(nbatch, ntemps, ...)`` leading axes.  The best sample is
        taken on the stored tempered log-prob (rung 0 is the posterior)."""
        r = self._b.get_summary(discard=discard, thin=thin, quantiles=quantiles, cov=cov)
        lead = (self.nbatch, self.ntemps)
        return type(r)(r.nsamples, *[None if a is None else a.reshape(lead + a.shape[1:]) for a in r[1:]])

    def get_blob_summary(self, discard=0, thin=1, quantiles=(0.16, 0.5, 0.84), cov=True):
        """:meth:`EnsembleBatch.get_blob_summary` of every rung, with ``(nbatch, ntemps, ...)`` leading axes: :meth:`get_summary` over
        the blob plane, ``nblobs`` in ``ndim``'s place.  ``ValueError`` when the likelihood has no blobs."""
        r = self._b.get_blob_summary(discard=discard, thin=thin, quantiles=quantiles, cov=cov)
        lead = (self.nbatch, self.ntemps)
        return type(r)(r.nsamples, *[None if a is None else a.reshape(lead + a.shape[1:]) for a in r[1:]])

    def get_rhat(self, discard=0, thin=1, chains="walkers", log_prob=False):
        """-> :class:`~emcee_amd.summary.RHat` of the rungs (:meth:`EnsembleBatch.get_rhat` on the underlying batch, the same
        bits).  ``chains="walkers"``: every rung of every object is its own group, its walkers the chains, arrays ``(nbatch,
        ntemps, ndim)``.  ``chains="members"``: each rung is pooled over the objects, ``nbatch nwalkers`` walkers a group, arrays
        ``(ntemps, ndim)`` -- with an adaptive ladder the same rung of different objects settles at different temperatures, so
        the pooled chains then sample different distributions and a large R-hat says only that.  ``log_prob=True`` adds the
        stored tempered log-prob as a last column."""
        _summary.check_chains(chains, ("walkers", "members"))
        r = self._b._rhat(discard, thin, 0, self.nbatch * self.ntemps, self.ntemps if chains == "members" else 0, log_prob)
        if chains == "members":
            return r
        lead = (self.nbatch, self.ntemps)
        return type(r)(*[a.reshape(lead + a.shape[1:]) for a in r[:3]], r.nchains, r.length)

    def get_histograms(self, bins=64, range=None, discard=0, thin=1, pairs="all", pair_bins=None):
        """:meth:`EnsembleBatch.get_histograms` of every rung -> :class:`~emcee_amd.summary.BatchHistograms` with ``(nbatch, ntemps,
        ...)`` leading axes on every per-column and per-panel array.  ``range`` may additionally be ``(nbatch, ntemps, ndim, 2)``."""
        return self._histograms(self._b.get_histograms, self.ndim, bins, range, discard, thin, pairs, pair_bins)

    def get_blob_histograms(self, bins=64, range=None, discard=0, thin=1, pairs="all", pair_bins=None):
        """:meth:`EnsembleBatch.get_blob_histograms` of every rung, reshaped as :meth:`get_histograms` is, ``nblobs`` in ``ndim``'s
        place.  ``ValueError`` when the likelihood has no blobs."""
        return self._histograms(self._b.get_blob_histograms, self.nblobs, bins, range, discard, thin, pairs, pair_bins)

    def _histograms(self, get, W, bins, range, discard, thin, pairs, pair_bins):
        if range is not None and np.ndim(range) == 4:
            range = np.asarray(range, dtype=np.float64)
            if range.shape[:2] != (self.nbatch, self.ntemps):
                raise ValueError("range: (nbatch, ntemps, ndim, 2) = (%d, %d, %d, 2); got %s" % (self.nbatch, self.ntemps, W, range.shape))
            range = range.reshape((self.nbatch * self.ntemps,) + range.shape[2:])
        r = get(bins=bins, range=range, discard=discard, thin=thin, pairs=pairs, pair_bins=pair_bins)
        lead = (self.nbatch, self.ntemps)
        split = (lambda arrays: [a.reshape(lead + a.shape[1:]) for a in arrays])
        return type(r)(r.nsamples, split(r.edges), split(r.counts), r.pairs, split(r.pair_edges), split(r.pair_counts))

    def _has_normalised_prior(self):
        return not (self._box is None and self._prior is None and not (self._fused is not None and self._fused.has_prior))

    def _evidence_rows(self, discard, thin, nblocks, need_prior=False):
        """-> (start, stop, nt, K, bl) after the argument checks (no device is touched)"""
        if int(thin) != thin or thin < 1:
            raise ValueError("thin must be an integer >= 1; got %r" % (thin,))
        if int(discard) != discard or discard < 0:
            raise ValueError("discard must be an integer >= 0; got %r" % (discard,))
        K = _check_nblocks(nblocks)
        if need_prior and not self._has_normalised_prior():
            raise ValueError("the evidence needs a normalised prior: with log_prior=None the prior is flat and improper")
        it = self.iteration
        if it <= 0:
            raise AttributeError("you must run the sampler with 'store == True' before accessing the results")
        thin, discard = int(thin), int(discard)
        start = min(discard + thin - 1, it)
        nt = len(range(start, it, thin))
        return start, it, nt, K, _block_length(nt, K)

    def _evidence_blocks(self, discard=0, thin=1, nblocks=8, lo=0, hi=None):
        """``emx_pt_evidence`` on objects [lo, hi) -> (sum_L (objects, T, K), amax (objects, T - 1, K), sexp (objects, T - 1, K),
        betas (objects, T), ladder_changed (objects), block length): what the device makes of the L plane."""
        hi = self.nbatch if hi is None else int(hi)
        lo = int(lo)
        if not 0 <= lo < hi <= self.nbatch:
            raise ValueError("objects [%d, %d) outside the %d of the sampler" % (lo, hi, self.nbatch))
        start, it, _, K, bl = self._evidence_rows(discard, thin, nblocks)
        G, T = hi - lo, self.ntemps
        A, M, S = np.empty((G, T, K)), np.empty((G, T - 1, K)), np.empty((G, T - 1, K))
        b, changed = np.empty((G, T)), np.zeros(G, dtype=np.int32)
        ptr = (lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None)
        rows = C.c_int64(0)
        self._ck(self._b._lib().emx_pt_evidence(self._h, lo, hi, start, it, int(thin), K, ptr(A), ptr(M), ptr(S), ptr(b), ptr(changed),
                                                C.byref(rows)))
        assert rows.value == bl
        return A, M, S, b, changed, bl

    def get_evidence(self, discard=0, thin=1, nblocks=8):
        """-> :class:`~emcee_amd.summary.Evidence`: every object's log-evidence by the stepping-stone estimator and by
        thermodynamic integration, each with a Monte-Carlo error from ``nblocks`` consecutive blocks of the selected steps
        (``get_chain``'s ``discard`` / ``thin``).  The stored log-likelihood plane is reduced next to the chain
        (``emx_pt_evidence``); only ``nbatch ntemps nblocks`` sums cross to the host.  The stepping-stone estimate needs far fewer
        rungs than thermodynamic integration, and stays finite where the likelihood is ``-inf`` on part of the prior (there the
        hottest rung's mean ``L``, and with it ``logz_ti``, is ``-inf``).  Needs a normalised prior (a box, or a prior callable),
        and a ladder that did not change over the used steps: freeze adaptation (``adaptive = False``) and discard the
        adaptive phase first.  :func:`stepping_stone_log_evidence` is the same on :meth:`get_log_likelihood`'s array.  A device
        failure raises :class:`emcee_amd._lib.EmxError` (no fallback).

        %s"""
        start, _, nt, K, bl = self._evidence_rows(discard, thin, nblocks, need_prior=True)
        A, M, S, b, changed, bl = self._evidence_blocks(discard, thin, K)
        if changed.any():
            bad = np.flatnonzero(changed)
            raise ValueError("object %d%s: the ladder changed within the %d used steps from stored step %d on: the evidence needs one "
                             "ladder. Freeze adaptation (adaptive = False), run on, and discard the adaptive phase (discard)"
                             % (bad[0], "" if len(bad) == 1 else " (and %d more)" % (len(bad) - 1), K * bl,
                                start + (nt - K * bl) * int(thin)))
        return _evidence_from_blocks(b, A, M, S, bl, bl * self.nwalkers)

    def mean_log_likelihood(self, discard=0):
        """``(nbatch, ntemps)``: the mean of ``L`` over the stored steps from ``discard`` on and every walker, on the device
        (:meth:`get_evidence` gives the same per block, with ``thin``, and the evidence estimates made from it)."""
        it = self.iteration
        if it <= 0:
            raise AttributeError("you must run the sampler with 'store == True' before accessing the results")
        discard = int(discard)
        if not 0 <= discard < it:
            raise ValueError("discard = %d leaves none of the %d stored steps" % (discard, it))
        out = np.empty(self.nbatch * self.ntemps)
        self._ck(_lib.load().emx_pt_mean_loglike(self._h, discard, it, 1, out))
        return out.reshape(self.nbatch, self.ntemps)

    def log_evidence_estimate(self, fburnin=0.1):
        """-> ``(logZ, dlogZ)``, each ``(nbatch,)``: thermodynamic integration over each object's ladder of the mean ``L`` of the
        stored steps after ``int(fburnin * iteration)``.  Needs a normalised prior (a box, or a prior callable), and a ladder
        that did not change over those steps.  :meth:`get_evidence` adds the stepping-stone estimate, which needs far fewer
        rungs, and the Monte-Carlo error of both."""
        if self._box is None and self._prior is None and not (self._fused is not None and self._fused.has_prior):
            raise ValueError("the evidence needs a normalised prior: with log_prior=None the prior is flat and improper")
        discard = int(fburnin * self.iteration)
        means = self.mean_log_likelihood(discard)
        lad = self.get_betas(discard=discard)
        if not np.array_equal(lad, np.broadcast_to(lad[:, :1], lad.shape)):
            raise ValueError("the ladder changed within the %d stored steps after %d: thermodynamic integration needs one ladder. "
                             "Freeze adaptation (adaptive = False), run on, and discard the adaptive phase (fburnin)"
                             % (lad.shape[1], discard))
        return thermodynamic_integration_log_evidence(lad[:, 0], means)

    def get_last_sample(self):
        """:class:`State` with ``(nbatch, ntemps, nwalkers, ndim)`` coordinates, tempered ``(nbatch, ntemps, nwalkers)``
        log-probs and, for a likelihood with blobs, ``(nbatch, ntemps, nwalkers, nblobs)`` blobs (else None)."""
        s = self._b.get_last_sample()
        lead = (self.nbatch, self.ntemps, self.nwalkers)
        return State(s.coords.reshape(lead + (self.ndim,)), log_prob=s.log_prob.reshape(lead),
                     blobs=None if s.blobs is None else s.blobs.reshape(lead + (self.nblobs,)))


PTSampler.get_rhat.__doc__ += "\n\n        " + _summary.RHAT_DEFINITION
PTSampler.get_evidence.__doc__ %= EVIDENCE_DEFINITION.replace("\n", "\n    ")
