"""Many independent small ensembles in one launch.

:class:`EnsembleBatch` runs B ensembles of one shape ``(nwalkers, ndim)`` -- replicated runs of one posterior, one fit per
object of a catalogue, a parameter sweep -- each with its own initial state, seed and (optionally) target parameters.  Every
``run_mcmc`` chunk is ONE launch of the one-workgroup kernel (``emx_batch_*`` in ``include/emx.h``): workgroup b runs
member b exactly as :class:`~emcee_amd.EnsembleSampler` with ``rng="philox"`` runs that ensemble, so member b is bit for bit
the sampler built with the same target, moves and initial state whose private generator was seeded with ``seeds[b]``::

    s = EnsembleSampler(nwalkers, ndim, target_b, moves, rng="philox")
    s.random_state = np.random.RandomState(seeds[b]).get_state()

Philox mode only; fused device targets (``IsoGaussian``, ``DiagGaussian``, ``DenseGaussian``, ``Rosenbrock``,
``UniformBox``); stretch, DE, snooker and Gaussian moves; every member must fit one workgroup (``nwalkers <= 4096``,
``ndim <= 256`` and the LDS bound).  A :class:`~emcee_amd.targets.BatchFused` -- the user's per-row ``__device__`` function
compiled into that kernel (:func:`~emcee_amd.targets.compile_fused`) -- runs the same way, at the same one launch per chunk.
With ``ndata`` (``compile_fused(..., data=True)``: a model with ``base`` and ``term`` whose log-probability sums over per-member
data, ragged counts included) every proposal gets a wave for the data sum instead of one lane.

The user's own model -- one fit per catalogue object, with per-object data -- is a
:class:`~emcee_amd.targets.BatchCallable` (or its native form, :class:`~emcee_amd.targets.BatchKernel`): one function called
once per phase of a step on the proposals of ALL members, a ``(B, R, ndim)`` block on the device, with the per-member data in
its closure.  A step is then ``S_max`` launches of the library's kernel (``k_batch_cb``: every member's commit and next
proposals) and ``S_max`` calls of that function, whatever B; member b is bit for bit the sampler above with
``DeviceCallable`` of the function restricted to member b.  ``S_max`` / ``S_min`` are the largest / smallest ``nsplits`` of the
schedule (a GaussianMove, one split, only as the sole move); ``R = ceil(nwalkers / S_min)``, and rows of ``q[b]`` past the
member's current split are padding -- copies of its walkers, their values ignored.  The LDS bound does not apply there.
Host callables, ``DeviceCallable`` and ``DeviceKernel`` targets run through :class:`~emcee_amd.EnsembleSampler`.

Blobs.  A ``BatchFused`` / ``BatchCallable`` / ``BatchKernel`` with ``nblobs = K > 0`` produces K float64 derived quantities with
every log-probability (the reference's ``log_prob_fn`` returning ``(lp, blobs...)``).  They stay on the device: committed exactly
when the log-probability is (a rejected proposal keeps the walker's previous ones), stored in a blob plane next to the chain,
read with :meth:`EnsembleBatch.get_blobs` / ``get_last_sample().blobs`` and summarised with :meth:`EnsembleBatch.get_blob_summary`.
Coordinates, log-probs and accept counts are bit for bit those of the same function without blobs.
"""
import ctypes as C

import numpy as np

from . import _lib
from . import autocorr
from . import summary as _summary
from .autocorr import integrated_time
from .ensemble import _native_desc, _parse_move_schedule, _refuse_extended_precision, philox_seed, walkers_independent
from .state import State
from .targets import (BatchFused, BatchKernel, BatchTarget, DeviceFused, PTFused, DenseGaussian, DeviceCallable, DeviceKernel, DeviceTarget, DiagGaussian, IsoGaussian,
                      Rosenbrock, UniformBox)

__all__ = ["EnsembleBatch"]

_TARGETS = (IsoGaussian, DiagGaussian, DenseGaussian, Rosenbrock, UniformBox)
_MOVES = (_lib.MOVE_STRETCH, _lib.MOVE_DE, _lib.MOVE_SNOOKER, _lib.MOVE_GAUSS)
_ILL = ("Initial state has a large condition number. Make sure that your walkers are linearly independent for the best "
        "performance")


def _member_error(b, text):
    return ValueError("member %d: %s" % (b, text))


class EnsembleBatch(object):
    """B independent ensembles of ``nwalkers`` walkers in ``ndim`` dimensions, run together on one GPU.

    ``target``: one :class:`~emcee_amd.targets.DeviceTarget` for every member, or a sequence of B targets of one class (one
    per member); or one :class:`~emcee_amd.targets.BatchCallable` / :class:`~emcee_amd.targets.BatchKernel` /
    :class:`~emcee_amd.targets.BatchFused` evaluating every member (its per-member parameters are its own).  ``moves``: the schedule forms of :class:`~emcee_amd.EnsembleSampler` over StretchMove, DEMove,
    DESnookerMove and GaussianMove.  ``seeds``: B integers; member b draws as a sampler whose generator was seeded with
    ``np.random.RandomState(seeds[b])``.  ``None`` draws them from NumPy's global state."""

    def __init__(self, nbatch, nwalkers, ndim, target, moves=None, seeds=None, device=None, rng="philox", _tempered=False, _ntemps=1):
        if rng != "philox":
            raise ValueError("EnsembleBatch runs rng='philox' only (the MT19937 stream is made by one host generator a "
                             "sampler; use EnsembleSampler for rng=%r)" % (rng,))
        self.nbatch, self.nwalkers, self.ndim = int(nbatch), int(nwalkers), int(ndim)
        if self.nbatch < 1 or self.nwalkers < 1 or self.ndim < 1:
            raise ValueError("nbatch, nwalkers and ndim must be positive")
        self.rng = rng
        self.device = 0 if device is None else int(device)
        self._tempered = bool(_tempered)      # PTSampler's handle: the only one that takes a PTFused
        self._pt_ntemps = int(_ntemps)        # (its rungs an object: members of the handle = objects x rungs)
        self._targets, self._per_member = self._parse_targets(target)
        self._moves, self._weights = _parse_move_schedule(moves)
        self._descs = []
        for m in self._moves:
            d = _native_desc(m, self.ndim, True, False)
            if d is None or d.kind not in _MOVES:
                raise ValueError("EnsembleBatch runs StretchMove, DEMove, DESnookerMove and GaussianMove; %s is not one of "
                                 "them (use EnsembleSampler)" % type(m).__name__)
            self._descs.append(d)
        if any(d.kind == _lib.MOVE_GAUSS and d.reserved == _lib.GAUSS_SEQUENTIAL for d in self._descs) and len(self._descs) > 1:
            raise ValueError("EnsembleBatch runs a sequential GaussianMove only as the one move of the schedule")
        lib = _lib.load()
        msg = C.create_string_buffer(256)
        arr = (_lib.MoveDesc * len(self._descs))(*self._descs)
        self.nblobs = int(getattr(self._targets[0], "nblobs", 0)) if isinstance(self._targets[0], BatchTarget) else 0
        # (a PTFused's blobs live in the tempered kernel's LDS map, whose bound depends on ntemps: PTSampler checks them)
        check_blobs = 0 if isinstance(self._targets[0], PTFused) else self.nblobs
        if lib.emx_check_batch_blobs(self.nwalkers, self.ndim, self._targets[0].kind, len(self._descs), arr, check_blobs, msg, 256) != 0:
            raise ValueError("EnsembleBatch: %s" % msg.value.decode())
        if seeds is None:
            seeds = np.random.randint(0, 2 ** 32, size=self.nbatch, dtype=np.uint64)
        seeds = [int(s) for s in np.asarray(seeds).reshape(-1)]
        if len(seeds) != self.nbatch:
            raise ValueError("seeds must hold nbatch = %d integers; got %d" % (self.nbatch, len(seeds)))
        self.seeds = seeds
        self._philox = np.array([philox_seed(np.random.RandomState(s)) for s in seeds], dtype=np.uint64)
        self._h = None
        self._cb_box = [None]             # an exception raised by a BatchCallable, handed to the caller by _ck
        self._cb_keep = None
        self._tuning = {}
        self._step = 0
        self._ran = False

    # ------------------------------------------------------------------ argument checks (no device involved)
    def _parse_targets(self, target):
        if isinstance(target, BatchFused) and target.ndim != self.ndim:
            raise ValueError("the BatchFused target was compiled for ndim %d; the batch has ndim %d" % (target.ndim, self.ndim))
        if isinstance(target, BatchFused):
            self._check_counts_length("BatchFused", target.ndata, self.nbatch, "a member")
        if isinstance(target, PTFused):
            if not self._tempered:
                raise TypeError("a PTFused is a likelihood of PTSampler: its launcher carries the tempered kernel (for an EnsembleBatch "
                                "compile the model as a BatchFused)")
            if target.ndim != self.ndim:
                raise ValueError("the PTFused target was compiled for ndim %d; the sampler has ndim %d" % (target.ndim, self.ndim))
            self._check_counts_length("PTFused", target.ndata, self.nbatch // self._pt_ntemps, "an object")
        if isinstance(target, BatchTarget):
            return [target], False
        if isinstance(target, DeviceFused):
            raise TypeError("a DeviceFused is a target of EnsembleSampler: its launcher carries the single sampler's half-step kernel "
                            "(for an EnsembleBatch compile the model as a BatchFused: the functor is the same)")
        if isinstance(target, DeviceTarget) or callable(target):
            targets, per_member = [target], False
        else:
            targets, per_member = list(target), True
            if any(isinstance(t, BatchTarget) for t in targets):
                raise TypeError("EnsembleBatch takes ONE BatchCallable / BatchKernel for all members: per-member parameters "
                                "belong to its function")
            if len(targets) != self.nbatch:
                raise ValueError("target: one DeviceTarget for all members or a sequence of nbatch = %d; got %d"
                                 % (self.nbatch, len(targets)))
        for t in targets:
            if isinstance(t, (DeviceCallable, DeviceKernel)) or not isinstance(t, _TARGETS):
                raise TypeError("EnsembleBatch runs the fused device targets (%s) or a BatchCallable / BatchKernel; run %s with "
                                "EnsembleSampler" % (", ".join(k.__name__ for k in _TARGETS), type(t).__name__))
        if len({type(t) for t in targets}) != 1:
            raise ValueError("the targets of a batch must be of one class; got %s" % sorted({type(t).__name__ for t in targets}))
        for b, t in enumerate(targets):
            if t.ndim is not None and t.ndim != self.ndim:
                raise ValueError("member %d: target of ndim %d in a batch of ndim %d" % (b, t.ndim, self.ndim))
        return targets, per_member

    @staticmethod
    def _check_counts_length(who, ndata, n, each):      # a fused data target's counts: None, one for all, or n (one `each`)
        if ndata is not None and not np.isscalar(ndata) and len(ndata) != n:
            raise ValueError("the %s target's ndata holds one count %s: nbatch = %d integers (or one for all); got %d" % (who, each, n, len(ndata)))

    def _check_state(self, coords):
        coords = np.asarray(coords)
        _refuse_extended_precision(coords)
        if coords.shape != (self.nbatch, self.nwalkers, self.ndim):
            raise ValueError("incompatible input dimensions %s: expected (nbatch, nwalkers, ndim) = %s"
                             % (coords.shape, (self.nbatch, self.nwalkers, self.ndim)))
        coords = np.ascontiguousarray(coords, dtype=np.float64)
        for b in range(self.nbatch):
            if not np.all(np.isfinite(coords[b])):
                raise _member_error(b, "At least one parameter value was infinite" if np.any(np.isinf(coords[b]))
                                    else "At least one parameter value was NaN")
        return coords

    # ------------------------------------------------------------------ device plumbing
    def _lib(self):
        return _lib.load()

    def _ck(self, rc):
        exc = self._cb_box[0]
        if exc is not None:               # raised inside the batched log-prob callback: the caller's own exception
            self._cb_box[0] = None
            raise exc
        if rc != 0:
            msg = self._lib().emx_batch_last_error(self._h)
            raise _lib.EmxError((msg or b"unknown error").decode() + " (code %d)" % rc)

    def _handle(self):
        if self._h is not None:
            return self._h
        lib = self._lib()
        h = C.c_void_p()
        if lib.emx_batch_create(self.device, self.nbatch, self.nwalkers, self.ndim, C.byref(h)) != 0:
            raise _lib.EmxError("emx_batch_create failed (no usable HIP device %d, or out of memory)" % self.device)
        self._h = h
        if isinstance(self._targets[0], BatchFused):
            self._bind_user_fused(h)
        elif isinstance(self._targets[0], PTFused):
            self._bind_pt_fused(h)
        elif isinstance(self._targets[0], BatchTarget):
            self._bind_callback(h)
        else:
            self._bind_fused(h)
        cdf = np.cumsum(self._weights)
        cdf /= cdf[-1]
        arr = (_lib.MoveDesc * len(self._descs))(*self._descs)
        self._ck(lib.emx_batch_set_moves(h, len(self._descs), arr, np.ascontiguousarray(cdf)))
        for i, m in enumerate(self._moves):
            vec = getattr(m, "_scale_vector", None)
            v = vec() if vec is not None and self._descs[i].kind == _lib.MOVE_GAUSS else None
            if v is not None:              # per-coordinate standard deviations (None: the isotropic sigma)
                v = np.ascontiguousarray(v, dtype=np.float64)
                self._ck(lib.emx_batch_set_move_scale(h, i, v, len(v)))
        for k, v in self._tuning.items():
            self._ck(lib.emx_batch_set_tuning(h, k.encode(), int(v)))
        self._ck(lib.emx_batch_set_philox(h, self._philox, self._step))
        return h

    def _bind_fused(self, h):
        kind = self._targets[0].kind
        params = [t.emx_params() for t in self._targets]
        p0 = p1 = None
        if kind in (_lib.TARGET_DIAG, _lib.TARGET_DENSE):
            p0 = np.ascontiguousarray(np.stack([p[1] for p in params]), dtype=np.float64)
            p1 = np.ascontiguousarray(np.stack([p[2] for p in params]), dtype=np.float64)
        scales = np.ascontiguousarray([p[3] for p in params], dtype=np.float64)
        ptr = (lambda a: None if a is None else a.ctypes.data_as(C.c_void_p))
        self._ck(self._lib().emx_batch_set_target(h, kind, ptr(p0), ptr(p1), ptr(scales), int(self._per_member)))

    def _bind_callback(self, h, tempered=False):
        """the handle's callback.  A tempered handle takes a callback with blobs once it is tempered (emx_pt_set_tempering refuses a
        handle that already has blobs), so PTSampler's handle is first bound as if the target had none -- that binding is never
        called -- and PTSampler binds again with ``tempered=True`` after emx_pt_set_tempering."""
        t = self._targets[0]
        nblobs = self.nblobs if tempered or not self._tempered else 0
        ftype = _lib.BATCH_LOG_PROB_BLOBS_FN if nblobs else _lib.BATCH_LOG_PROB_FN
        if isinstance(t, BatchKernel):
            fn = t.fn_ptr if isinstance(t.fn_ptr, ftype) else C.cast(t.fn_ptr, ftype)
            user = t.user_ptr if isinstance(t.user_ptr, C.c_void_p) else C.c_void_p(t.user_ptr)
        else:
            fn, user = ftype(_trampoline(t.fn, self.device, self._cb_box, nblobs)), None
        self._cb_keep = fn                # the library holds the pointer: keep the object alive
        if nblobs:
            self._ck(self._lib().emx_set_batch_target_callback_blobs(h, fn, user, self.nblobs))
        else:
            self._ck(self._lib().emx_set_batch_target_callback(h, fn, user))

    def _bind_fused_target(self, h, ftype, setter, *extra, counts=None, repeat=1):
        """``setter(h, fn, ndim, user, *extra)``, `extra` the counts of a data target: ``counts``, one for all or one each, each ``repeat`` times"""
        t = self._targets[0]
        fn = t.fn_ptr if isinstance(t.fn_ptr, ftype) else C.cast(t.fn_ptr, ftype)
        self._cb_keep = (fn, t)           # the library holds the launcher and the user's device pointer: keep both alive
        if counts is not None:
            extra = (np.ascontiguousarray(np.repeat(np.broadcast_to(np.asarray(counts, dtype=np.int64), (self.nbatch // repeat,)), repeat)),)
        self._ck(setter(h, fn, t.ndim, C.c_void_p(t.user_address()), *extra))

    def _bind_user_fused(self, h):
        t, lib = self._targets[0], self._lib()
        if t.ndata is not None:           # a data target: its own launcher type, and the members' counts
            self._bind_fused_target(h, _lib.FUSED_BATCH_DATA_FN, lib.emx_set_batch_target_fused_data, counts=t.ndata)
        elif self.nblobs:
            self._bind_fused_target(h, _lib.FUSED_BATCH_FN, lib.emx_set_batch_target_fused_blobs, self.nblobs)
        else:
            self._bind_fused_target(h, _lib.FUSED_BATCH_FN, lib.emx_set_batch_target_fused)

    def _bind_pt_fused(self, h):
        t, lib = self._targets[0], self._lib()
        if t.ndata is not None:           # a data target: one count an object, every rung of an object its object's
            self._bind_fused_target(h, _lib.PT_FUSED_FN, lib.emx_pt_set_target_fused_data, counts=t.ndata, repeat=self._pt_ntemps)
        elif self.nblobs:
            self._bind_fused_target(h, _lib.PT_FUSED_FN, lib.emx_pt_set_target_fused_blobs, self.nblobs)
        else:
            self._bind_fused_target(h, _lib.PT_FUSED_FN, lib.emx_pt_set_target_fused)

    def set_tuning(self, key, value):
        """``"batch_threads"`` / ``"batch_plan_steps"`` (include/emx.h): the launch shape; ``"batch_acf_series"``: series per
        FFT chunk of ``get_autocorr_time(on_device=True)``; ``"batch_summary_members"``: members per pass of
        ``get_summary``; ``"batch_rhat_members"``: members per pass of ``get_rhat``; ``"batch_hist_members"`` /
        ``"batch_hist_rows"``: members and rows of a member per chunk of ``get_histograms``.  No bit depends on them."""
        self._tuning[key] = int(value)
        if self._h is not None:
            self._ck(self._lib().emx_batch_set_tuning(self._h, key.encode(), int(value)))

    def launch_info(self):
        """-> dict(threads, plan_steps, launches): the last launch's shape and the launches so far."""
        t, p, n = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        if self._h is not None:
            self._ck(self._lib().emx_batch_launch_info(self._h, C.byref(t), C.byref(p), C.byref(n)))
        return dict(threads=t.value, plan_steps=p.value, launches=n.value)

    def close(self):
        if self._h is not None:
            self._lib().emx_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _raise_on_status(self, what):
        bits = np.zeros(self.nbatch, dtype=np.uint32)
        self._ck(self._lib().emx_batch_status(self._h, bits))
        bad = np.flatnonzero(bits)
        if len(bad):
            b = int(bad[0])
            text = ("At least one parameter value was infinite or NaN" if bits[b] & 2 else
                    "The initial log_prob was NaN" if what == "eval" else "Probability function returned NaN")
            more = "" if len(bad) == 1 else " (and members %s)" % bad[1:].tolist()
            raise ValueError("member %d: %s%s" % (b, text, more))

    # ------------------------------------------------------------------ sampling
    def run_mcmc(self, initial_state, nsteps, thin_by=1, store=True, skip_initial_state_check=False):
        """Advance every member ``nsteps`` stored steps (``nsteps * thin_by`` proposals) -> :class:`State` with ``(B, nwalkers,
        ndim)`` coordinates and ``(B, nwalkers)`` log-probs.  ``initial_state`` ``(B, nwalkers, ndim)`` (an array or a State),
        or None to continue from where the last call stopped.  Checks as ``EnsembleSampler.run_mcmc``, member by member."""
        nsteps, thin_by = int(nsteps), int(thin_by)
        if thin_by <= 0:
            raise ValueError("Invalid thinning argument")
        if nsteps < 0:
            raise ValueError("nsteps must be >= 0")
        coords = None
        if initial_state is None:
            if not self._ran:
                raise ValueError("Cannot have `initial_state=None` if run_mcmc has never been called.")
        else:
            coords = self._check_state(initial_state.coords if isinstance(initial_state, State) else initial_state)
            if not skip_initial_state_check:
                for b in range(self.nbatch):
                    if not walkers_independent(coords[b]):
                        raise _member_error(b, _ILL)
        for m in self._moves:
            if self.nwalkers < 2 * self.ndim and hasattr(m, "nsplits") and not getattr(m, "live_dangerously", False):
                raise RuntimeError("It is unadvisable to use a red-blue move with fewer walkers than twice the number of dimensions.")
        lib = self._lib()
        h = self._handle()
        if coords is not None:
            self._ck(lib.emx_batch_set_state(h, coords, None))
            self._ck(lib.emx_batch_eval_state_log_prob(h))
            self._raise_on_status("eval")
            self._ran = True
        if store:
            self._ck(lib.emx_batch_chain_config(h, self.iteration + nsteps))
        self._ck(lib.emx_batch_run(h, nsteps, thin_by, int(bool(store))))
        self._sync_moves()
        step = C.c_uint64(0)
        self._ck(lib.emx_batch_get_philox(h, np.zeros(self.nbatch, dtype=np.uint64), C.byref(step)))
        self._step = step.value
        self._raise_on_status("run")
        return self.get_last_sample()

    def _sync_moves(self):
        for i, m in enumerate(self._moves):          # the sequential Gaussian mode's cursor lives in the move
            prop = getattr(m, "get_proposal", None)
            if hasattr(m, "_scale_vector") and getattr(prop, "mode", None) == "sequential":
                d = _lib.MoveDesc()
                self._ck(self._lib().emx_batch_get_move(self._h, i, C.byref(d)))
                prop.index = int(d.gammas)

    # ------------------------------------------------------------------ results
    @property
    def iteration(self):
        """Stored steps of every member."""
        if self._h is None:
            return 0
        s, p = C.c_int64(0), C.c_int64(0)
        self._ck(self._lib().emx_batch_iteration(self._h, C.byref(s), C.byref(p)))
        return s.value

    def _read(self, what, lo, hi, discard, thin, flat):
        it = self.iteration
        if it <= 0:
            raise AttributeError("you must run the sampler with 'store == True' before accessing the results")
        thin, discard = int(thin), int(discard)
        start = min(discard + thin - 1, it)                 # reference backend.py:53
        nsel = len(range(start, it, thin))
        shape = (hi - lo, nsel, self.nwalkers) + ((self.ndim,) if what == 0 else (self.nblobs,) if what == 4 else ())
        out = np.empty(shape)
        if nsel and hi > lo:
            self._ck(self._lib().emx_batch_chain_read(self._h, what, lo, hi, start, it, thin, out))
        if flat:
            out = out.reshape((hi - lo, nsel * self.nwalkers) + shape[3:])
        return out

    def get_chain(self, discard=0, thin=1, flat=False):
        """``(B, nsteps, nwalkers, ndim)``; ``flat`` -> ``(B, nsteps * nwalkers, ndim)``."""
        return self._read(0, 0, self.nbatch, discard, thin, flat)

    def get_log_prob(self, discard=0, thin=1, flat=False):
        """``(B, nsteps, nwalkers)``; ``flat`` -> ``(B, nsteps * nwalkers)``."""
        return self._read(1, 0, self.nbatch, discard, thin, flat)

    def get_blobs(self, discard=0, thin=1, flat=False):
        """``(B, nsteps, nwalkers, nblobs)``; ``flat`` -> ``(B, nsteps * nwalkers, nblobs)``: the blobs stored with every sample
        of the chain.  None when the target has no blobs (as the reference's)."""
        if not self.nblobs:
            return None
        return self._read(4, 0, self.nbatch, discard, thin, flat)

    def _accepted(self):
        out = np.zeros((self.nbatch, self.nwalkers))
        if self._h is not None:
            self._ck(self._lib().emx_batch_accepted_counts(self._h, out))
        return out

    @property
    def acceptance_fraction(self):
        """``(B, nwalkers)``: the fraction of proposed steps that were accepted."""
        return self._accepted() / float(self.iteration)

    def get_autocorr_time(self, discard=0, thin=1, c=5, tol=50, quiet=False, on_device=False):
        """``(B, ndim)``: :func:`emcee_amd.autocorr.integrated_time` of each member's chain, in steps.

        The default copies each member's chain to the host and runs the NumPy estimator.  ``on_device=True`` computes the same
        estimator for every member next to the chain (``emx_autocorr_batch``: batched hipFFT, Sokal's window on the device) and
        copies back only the ``(B, ndim)`` results; the ``tol`` rule is then applied per member, and the error names the
        members that fail it.  A device failure raises :class:`emcee_amd._lib.EmxError` (no fallback)."""
        if not on_device:
            return np.stack([self[b].get_autocorr_time(discard=discard, thin=thin, c=c, tol=tol, quiet=quiet)
                             for b in range(self.nbatch)])
        tau, _, nt = self._autocorr_device(discard, thin, c, 0, self.nbatch)
        _check_tol(tau, nt, tol, quiet, list(range(self.nbatch)), tau)
        return thin * tau

    def _autocorr_device(self, discard=0, thin=1, c=5, lo=0, hi=None):
        """-> (tau (hi - lo, ndim) in units of the selected samples, Sokal windows (hi - lo, ndim), series length nt):
        ``emx_autocorr_batch`` on members [lo, hi).  Arguments are checked before any device is touched."""
        hi = self.nbatch if hi is None else int(hi)
        lo = int(lo)
        if int(thin) != thin or thin < 1:
            raise ValueError("thin must be an integer >= 1; got %r" % (thin,))
        if int(discard) != discard or discard < 0:
            raise ValueError("discard must be an integer >= 0; got %r" % (discard,))
        if not 0 <= lo < hi <= self.nbatch:
            raise ValueError("members [%d, %d) outside a batch of %d" % (lo, hi, self.nbatch))
        if self._h is None or self.iteration <= 0:
            raise ValueError("you must run the sampler with 'store == True' before computing autocorrelation times")
        from .device import DeviceEnsemble
        lib = self._lib()
        DeviceEnsemble._load_hipfft(lib)
        tau = np.empty((hi - lo, self.ndim))
        win = np.empty((hi - lo, self.ndim), dtype=np.int32)
        nt = C.c_int64(0)
        self._ck(lib.emx_autocorr_batch(self._h, lo, hi, int(discard), int(thin), float(c), tau, win, C.byref(nt)))
        return tau, win, nt.value

    def get_summary(self, discard=0, thin=1, quantiles=(0.16, 0.5, 0.84), cov=True):
        """-> :class:`~emcee_amd.summary.BatchSummary` of every member over the selected steps (``get_chain``'s ``discard`` /
        ``thin``) and all walkers, computed next to the chain (``emx_summary_batch``): ``mean`` ``(B, ndim)``, ``cov``
        ``(B, ndim, ndim)`` (``np.cov(flat.T)``, exactly symmetric; None with ``cov=False``), ``quantiles`` ``(B, nq, ndim)``
        (``np.quantile``'s default rule, at most 16), ``map_coords`` ``(B, ndim)`` / ``map_log_prob`` ``(B,)``: the stored sample
        with the largest stored log-prob, the earliest step and then the lowest walker among equals.  Only these cross to the
        host.  A device failure raises :class:`emcee_amd._lib.EmxError` (no fallback)."""
        return self._summary(discard, thin, quantiles, cov, 0, self.nbatch)

    def get_blob_summary(self, discard=0, thin=1, quantiles=(0.16, 0.5, 0.84), cov=True):
        """-> :class:`~emcee_amd.summary.BatchSummary` of every member's BLOBS: what :meth:`get_summary` returns, computed over the
        blob plane on the device by the same kernels, with ``nblobs`` in ``ndim``'s place -- ``mean`` ``(B, nblobs)``, ``cov``
        ``(B, nblobs, nblobs)``, ``quantiles`` ``(B, nq, nblobs)``; ``map_coords`` ``(B, nblobs)`` holds the blobs of the stored
        sample with the largest stored log-prob (``map_log_prob``).  Raises ``ValueError`` when the target has no blobs."""
        return self._summary(discard, thin, quantiles, cov, 0, self.nbatch, plane=4)

    def _summary(self, discard, thin, quantiles, cov, lo, hi, plane=0):
        if plane == 4 and not self.nblobs:
            raise ValueError("the target has no blobs (nblobs = 0): there is no blob plane to summarise")
        q = _summary.check_quantiles(quantiles)
        _, _, nt = self._summary_rows(discard, thin)
        ranks, ilo, ihi, g = _summary.plan_ranks(nt * self.nwalkers, q)
        n, mean, c, order, mx, mlp = self._summary_device(discard, thin, ranks, cov, lo, hi, plane)
        return _summary.BatchSummary(n, mean, c, _summary.interpolate(order, ilo, ihi, g), mx, mlp)

    def _summary_rows(self, discard, thin):
        """-> (start, stop, nt): ``_read``'s selection of stored rows, after the argument checks (no device is touched)."""
        if int(thin) != thin or thin < 1:
            raise ValueError("thin must be an integer >= 1; got %r" % (thin,))
        if int(discard) != discard or discard < 0:
            raise ValueError("discard must be an integer >= 0; got %r" % (discard,))
        if self._h is None or self.iteration <= 0:
            raise ValueError("you must run the sampler with 'store == True' before computing summaries")
        thin, discard, it = int(thin), int(discard), self.iteration
        start = min(discard + thin - 1, it)                 # reference backend.py:53
        nt = len(range(start, it, thin))
        if nt < 1:
            raise ValueError("discard = %d, thin = %d select none of the %d stored steps" % (discard, thin, it))
        return start, it, nt

    def _summary_device(self, discard=0, thin=1, ranks=(), cov=True, lo=0, hi=None, plane=0):
        """-> (n, mean (hi - lo, ndim), cov (hi - lo, ndim, ndim) or None, order statistics (hi - lo, len(ranks), ndim), MAP
        coordinates (hi - lo, ndim), MAP log-probs (hi - lo)): ``emx_summary_batch`` on members [lo, hi), ``order[:, r, d]``
        being the ``ranks[r]``-th smallest (0-based) of the ``n`` selected samples of parameter d.  Arguments are checked
        before any device is touched."""
        hi = self.nbatch if hi is None else int(hi)
        lo = int(lo)
        if not 0 <= lo < hi <= self.nbatch:
            raise ValueError("members [%d, %d) outside a batch of %d" % (lo, hi, self.nbatch))
        ranks = np.ascontiguousarray(ranks, dtype=np.int64).ravel()
        if len(ranks) > 2 * _summary.MAX_QUANTILES:
            raise ValueError("at most %d ranks in one call; got %d" % (2 * _summary.MAX_QUANTILES, len(ranks)))
        start, it, nt = self._summary_rows(discard, thin)
        thin, n = int(thin), nt * self.nwalkers
        if len(ranks) and not (0 <= ranks.min() and ranks.max() < n):
            raise ValueError("ranks must lie in [0, %d)" % n)
        M, D = hi - lo, (self.nblobs if plane == 4 else self.ndim)
        mean, mx, mlp = np.empty((M, D)), np.empty((M, D)), np.empty(M)
        c = np.empty((M, D, D)) if cov else None
        order = np.empty((M, len(ranks), D))
        ptr = (lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(C.c_void_p))
        ns = C.c_int64(0)
        if plane == 0:
            self._ck(self._lib().emx_summary_batch(self._h, lo, hi, start, it, thin, ptr(mean), ptr(c), len(ranks), ptr(ranks), ptr(order),
                                                   ptr(mx), ptr(mlp), C.byref(ns)))
        else:
            self._ck(self._lib().emx_summary_batch_plane(self._h, plane, lo, hi, start, it, thin, ptr(mean), ptr(c), len(ranks), ptr(ranks),
                                                         ptr(order), ptr(mx), ptr(mlp), C.byref(ns)))
        assert ns.value == n
        return n, mean, c, order, mx, mlp

    def get_rhat(self, discard=0, thin=1, chains="walkers", log_prob=False):
        """-> :class:`~emcee_amd.summary.RHat` ``(rhat, within, between, nchains, length)`` over the selected steps
        (``get_chain``'s ``discard`` / ``thin``), computed next to the chain (``emx_rhat_batch``); only these numbers cross to
        the host.  ``chains="walkers"``: every member is its own group, arrays ``(B, ndim)`` -- row ``b`` is ``bt[b].get_rhat()``
        bit for bit.  ``chains="members"``: the replicates are pooled, all ``B nwalkers`` walkers form one group, arrays
        ``(ndim,)`` -- "do my B independent ensembles agree?".  ``log_prob=True`` makes the last axis ``ndim + 1``.

        %s

        :func:`emcee_amd.summary.split_rhat` is the same definition on ``get_chain()``'s array.  A device failure raises
        :class:`emcee_amd._lib.EmxError` (no fallback).  Tuning ``"batch_rhat_members"`` (members per pass) changes no bit."""
        _summary.check_chains(chains, ("walkers", "members"))
        r = self._rhat(discard, thin, 0, self.nbatch, 1 if chains == "members" else 0, log_prob)
        return r if chains == "walkers" else _summary.RHat(r.rhat[0], r.within[0], r.between[0], r.nchains, r.length)

    def _rhat(self, discard, thin, lo, hi, pool, log_prob):
        """-> RHat with arrays (groups, W): ``emx_rhat_batch`` on members [lo, hi); ``pool`` 0: a group a member, P > 0: members
        with equal ``(m - lo) mod P`` pooled into P groups.  Arguments are checked before any device is touched."""
        lo, hi, pool = int(lo), int(hi), int(pool)
        if not 0 <= lo < hi <= self.nbatch:
            raise ValueError("members [%d, %d) outside a batch of %d" % (lo, hi, self.nbatch))
        if pool < 0 or (pool and (hi - lo) % pool):
            raise ValueError("pool = %d: 0, or a divisor of the %d members" % (pool, hi - lo))
        start, it, nt = self._summary_rows(discard, thin)
        h = _summary.check_rhat_length(nt)
        G, W = (pool if pool else hi - lo), self.ndim + (1 if log_prob else 0)
        within, between = np.empty((G, W)), np.empty((G, W))
        ptr = (lambda a: a.ctypes.data_as(C.c_void_p))
        nc, hd = C.c_int64(0), C.c_int64(0)
        self._ck(self._lib().emx_rhat_batch(self._h, lo, hi, pool, start, it, int(thin), int(bool(log_prob)), ptr(within), ptr(between),
                                            C.byref(nc), C.byref(hd)))
        assert hd.value == h
        return _summary.RHat(_summary.rhat_of(within, between, h), within, between, nc.value, h)

    def get_histograms(self, bins=64, range=None, discard=0, thin=1, pairs="all", pair_bins=None):
        """-> :class:`~emcee_amd.summary.BatchHistograms`: for EVERY member the marginal histogram of every parameter and the 2-d
        histogram of every requested parameter pair (a corner plot's panels) over the selected steps (``get_chain``'s
        ``discard`` / ``thin``) and all walkers, counted next to the chain (``emx_chain_minmax_batch``,
        ``emx_histograms_batch``) -- ``np.histogram`` / ``np.histogram2d`` of each member, count for count.  One launch grid
        covers all members; only the integer counts cross to the host.

        The arguments are ``EnsembleSampler.get_histograms``'s: ``bins`` an int (1 ... 1024), one edge array for every column or
        one a column; ``range`` (with an integer ``bins``) None, ``(lo, hi)``, ``(ndim, 2)`` or additionally ``(B, ndim, 2)``: a
        range of its own for every member; ``pairs`` ``"all"``, None or a sequence of ``(i, j)``; ``pair_bins`` as ``bins``, at
        most 128 (None: ``min(bins, 64)`` over the same range, or the edges given as ``bins``).  With ``range=None`` every member
        gets ``np.linspace`` between ITS OWN minimum and maximum of every column, so ``edges[d]`` is ``(B, nb_d + 1)``; a
        non-finite value in such a column raises ``ValueError`` naming the members and columns.  Edges given as arrays are
        shared by all members.  A device failure raises :class:`emcee_amd._lib.EmxError` (no fallback)."""
        return self._histograms(0, bins, range, discard, thin, pairs, pair_bins, 0, self.nbatch)

    def get_blob_histograms(self, bins=64, range=None, discard=0, thin=1, pairs="all", pair_bins=None):
        """-> :class:`~emcee_amd.summary.BatchHistograms` of every member's BLOBS: what :meth:`get_histograms` returns, counted over
        the blob plane by the same kernels with ``nblobs`` in ``ndim``'s place.  ``ValueError`` when the target has no blobs."""
        return self._histograms(4, bins, range, discard, thin, pairs, pair_bins, 0, self.nbatch)

    def _histograms(self, plane, bins, rng, discard, thin, pairs, pair_bins, lo, hi):
        """members [lo, hi) -> BatchHistograms; a 3-d ``rng`` has one entry for every member of the BATCH.  Every argument is
        checked before any device is touched."""
        if int(thin) != thin or thin < 1:
            raise ValueError("thin must be an integer >= 1; got %r" % (thin,))
        if int(discard) != discard or discard < 0:
            raise ValueError("discard must be an integer >= 0; got %r" % (discard,))
        bins = _summary.check_bins(bins, "bins", _summary.MAX_BINS)
        rng = _summary.check_batch_range(rng)
        pairs = _summary.check_pairs(pairs)
        if pair_bins is not None:
            pair_bins = _summary.check_bins(pair_bins, "pair_bins", _summary.MAX_PAIR_BINS)
        elif isinstance(bins, int):
            pair_bins = min(bins, 64)
        if plane == 4 and not self.nblobs:
            raise ValueError("the target has no blobs (nblobs = 0): there is no blob plane to histogram")
        W, M = (self.nblobs if plane == 4 else self.ndim), hi - lo
        _summary.check_batch_columns(bins, rng, self.nbatch, W, "bins")
        _summary.check_columns(pair_bins, None, W, "pair_bins")
        pairs = _summary.column_pairs(pairs, W)
        if pair_bins is None:                               # the edges given as bins serve the panels too
            if len(pairs) and max(len(e) - 1 for e in (bins if isinstance(bins, list) else [bins])) > _summary.MAX_PAIR_BINS:
                raise ValueError("pair panels have at most %d bins a column: pass pair_bins, or pairs=None for the marginals alone"
                                 % _summary.MAX_PAIR_BINS)
            pair_bins = bins
        if not 0 <= lo < hi <= self.nbatch:
            raise ValueError("members [%d, %d) outside a batch of %d" % (lo, hi, self.nbatch))
        start, it, nt = self._summary_rows(discard, thin)
        thin, n = int(thin), nt * self.nwalkers
        if rng is not None and rng.ndim == 3:
            rng = rng[lo:hi]
        minmax = None
        if _summary.needs_minmax(bins, pair_bins, rng):
            mlo, mhi, nf = self._minmax_device(plane, lo, hi, start, it, thin)
            if nf.any():
                bad = np.argwhere(nf > 0)
                named = ", ".join("member %d column %d" % (lo + m, d) for m, d in bad[:8].tolist())
                raise ValueError("autodetected range of %s%s is not finite" % (named, " and %d more" % (len(bad) - 8) if len(bad) > 8 else ""))
            minmax = (mlo, mhi)
        edges = _summary.member_edges(bins, rng, M, W, minmax)
        pedges = _summary.member_edges(pair_bins, rng, M, W, minmax)
        shared = _summary.shared_edges(bins, rng), _summary.shared_edges(pair_bins, rng)
        counts, pc = self._hist_device(plane, lo, hi, start, it, thin, edges, pedges, pairs, shared, n)
        return _summary.BatchHistograms(n, edges, counts, pairs, pedges, pc)

    def _minmax_device(self, plane, lo, hi, start, stop, stride):
        """-> (lo, hi, nonfinite), each (hi - lo, W): ``emx_chain_minmax_batch`` on members [lo, hi)"""
        W = self.nblobs if plane == 4 else self.ndim
        mlo, mhi, nf = np.empty((hi - lo, W)), np.empty((hi - lo, W)), np.zeros((hi - lo, W), dtype=np.int64)
        ptr = (lambda a: a.ctypes.data_as(C.c_void_p))
        self._ck(self._lib().emx_chain_minmax_batch(self._h, plane, lo, hi, start, stop, stride, ptr(mlo), ptr(mhi), ptr(nf)))
        return mlo, mhi, nf

    def _hist_device(self, plane, lo, hi, start, stop, stride, edges, pedges, pairs, shared, n):
        """-> (counts, pair_counts): ``emx_histograms_batch`` on members [lo, hi) with the per-member ``edges`` / ``pedges``
        (W arrays ``(M, nb_d + 1)``; ``shared``: whether all rows of the marginal / the pair edges are one, which then goes to
        the device once)"""
        M, W, P = hi - lo, len(edges), len(pairs)

        def pack(es, one):
            off = np.zeros(W + 1, dtype=np.int64)
            off[1:] = np.cumsum([e.shape[1] for e in es])
            e = np.ascontiguousarray(np.concatenate(es, axis=1), dtype=np.float64)
            return (off, e[0].copy(), 0) if one else (off, e, int(off[-1]))
        ptr = (lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(C.c_void_p))
        off, e, es = pack(edges, shared[0])
        counts = np.empty((M, int(off[-1]) - W), dtype=np.int64)
        pairs32 = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        poff = pe = pair_off = pc = pb = None
        ps = 0
        if P:
            poff, pe, ps = pack(pedges, shared[1])
            pb = np.diff(poff) - 1
            pair_off = np.zeros(P + 1, dtype=np.int64)
            pair_off[1:] = np.cumsum(pb[pairs32[:, 0]] * pb[pairs32[:, 1]])
            pc = np.empty((M, int(pair_off[-1])), dtype=np.int64)
        ns = C.c_int64(0)
        self._ck(self._lib().emx_histograms_batch(self._h, plane, lo, hi, start, stop, stride, ptr(off), ptr(e), es, ptr(counts), ptr(poff),
                                                  ptr(pe), ps, P, ptr(pairs32), ptr(pair_off), ptr(pc), C.byref(ns)))
        assert ns.value == n
        co = off[:-1] - np.arange(W)
        # views of the two buffers the library filled (a panel's last axis is split, which copies nothing): at 1 024 members and
        # ten 64 x 64 panels the counts are a third of a gigabyte
        out = [counts[:, co[d]:co[d] + edges[d].shape[1] - 1] for d in range(W)]
        pout = [pc[:, pair_off[p]:pair_off[p + 1]].reshape(M, pb[pairs32[p, 0]], pb[pairs32[p, 1]]) for p in range(P)]
        return out, pout

    def histogram_launches(self):
        """kernel launches of the last ``get_histograms`` / ``get_blob_histograms`` call's counting (``emx_histograms_batch_info``):
        it does not grow with the number of members of a chunk."""
        n = C.c_int64(0)
        if self._h is not None:
            self._ck(self._lib().emx_histograms_batch_info(self._h, C.byref(n)))
        return n.value

    def get_last_sample(self):
        """:class:`State` with ``(B, nwalkers, ndim)`` coordinates and ``(B, nwalkers)`` log-probs."""
        if self._h is None or not self._ran:
            raise AttributeError("you must run the sampler before accessing the last sample")
        coords = np.empty((self.nbatch, self.nwalkers, self.ndim))
        lp = np.empty((self.nbatch, self.nwalkers))
        self._ck(self._lib().emx_batch_get_state(self._h, coords.ctypes.data_as(C.c_void_p), lp.ctypes.data_as(C.c_void_p)))
        blobs = None
        if self.nblobs:
            blobs = np.empty((self.nbatch, self.nwalkers, self.nblobs))
            self._ck(self._lib().emx_get_blobs_batch(self._h, blobs.ctypes.data_as(C.c_void_p), None))
        return State(coords, log_prob=lp, blobs=blobs)

    def __len__(self):
        return self.nbatch

    def __getitem__(self, b):
        b = int(b)
        if b < 0:
            b += self.nbatch
        if not 0 <= b < self.nbatch:
            raise IndexError("member %d outside a batch of %d" % (b, self.nbatch))
        return _Member(self, b)


def _check_tol(tau, nt, tol, quiet, members, err_tau):
    """integrated_time's ``tol`` rule (autocorr.py:110-121) on ``tau`` (one row per member of ``members``) of ``nt`` samples: a
    member is flagged when ``tol * tau > nt`` for any parameter (NaN never is).  Raise AutocorrError(err_tau, msg) naming the
    flagged members, or only log the message with ``quiet``."""
    flag = tol * tau > nt
    rows = np.flatnonzero(flag.any(axis=1))
    if not len(rows):
        return
    named = [str(members[r]) for r in rows]
    who = ("member " if len(named) == 1 else "members ") + ", ".join(named[:8]) + (
        " and %d more" % (len(named) - 8) if len(named) > 8 else "")
    msg = ("The chain is shorter than {0} times the integrated autocorrelation time for {1} parameter(s) of {2}. "
           "Use this estimate with caution and run a longer chain!\n").format(tol, int(flag.sum()), who)
    msg += "N/{0} = {1:.0f};\ntau: {2}".format(tol, nt / tol, tau[rows[0]] if len(rows) == 1 else tau[rows])
    if not quiet:
        raise autocorr.AutocorrError(err_tau, msg)
    autocorr.logger.warning(msg)


def _split_result(res, nb, rows, nblobs):
    """what a BatchCallable's ``fn`` returned for ``nb`` members x ``rows`` rows -> (log_prob, blobs or None), after the shape
    checks: ``nb * rows`` log-probs and, with ``nblobs > 0``, a pair whose second entry has shape ``(nb, rows, nblobs)``."""
    bl = None
    if nblobs:
        if not (isinstance(res, (tuple, list)) and len(res) == 2):
            raise ValueError("with nblobs = %d the batched log_prob_fn returns (log_prob, blobs); got %s" % (nblobs, type(res).__name__))
        res, bl = res
        got = tuple(bl.shape) if hasattr(bl, "shape") else np.shape(bl)
        if got != (nb, rows, nblobs):
            raise ValueError("the batched log_prob_fn returned blobs of shape %s; expected (members, rows, nblobs) = %s"
                             % (got, (nb, rows, nblobs)))
    got = tuple(res.shape) if hasattr(res, "shape") else np.shape(res)
    if int(np.prod(got, dtype=np.int64)) != nb * rows:
        raise ValueError("the batched log_prob_fn returned %d values for %d members x %d rows" % (int(np.prod(got, dtype=np.int64)), nb, rows))
    return res, bl


def _trampoline(fn, device, box, nblobs=0):
    """emx_batch_log_prob_fn over a BatchCallable's ``fn`` (DeviceEnsemble.set_target_callback's eager form): ``fn`` sees the
    library's block as a ``(B, rows, ndim)`` tensor and runs on the handle's stream; an exception is kept in ``box[0]``."""
    import torch
    from .parallel import _DevView
    streams = {}
    dev = torch.device("cuda", device)

    def tramp(user, q_ptr, nb, rows, ndim, lp_ptr, *rest):
        stream = rest[-1]                 # (emx_batch_log_prob_blobs_fn: nblobs and blobs_dev come before it)
        try:
            s = streams.get(stream)
            if s is None:
                s = streams[stream] = torch.cuda.ExternalStream(stream, device=dev) if stream else torch.cuda.default_stream(dev)
            n = nb * rows
            with torch.cuda.stream(s):
                q = torch.as_tensor(_DevView(q_ptr, n * ndim), device=dev).view(nb, rows, ndim)
                out = torch.as_tensor(_DevView(lp_ptr, n), device=dev)
                res, bl = _split_result(fn(q), nb, rows, nblobs)
                res = torch.as_tensor(res, dtype=torch.float64, device=dev).reshape(-1)
                out.copy_(res)
                if nblobs:
                    bl = torch.as_tensor(bl, dtype=torch.float64, device=dev).reshape(-1)
                    torch.as_tensor(_DevView(rest[1], n * nblobs), device=dev).copy_(bl)
            return 0
        except BaseException as e:  # noqa: BLE001  (handed to the caller by EnsembleBatch._ck)
            box[0] = e
            return -1
    return tramp


class _Member(object):
    """Read-only view of member b: the getters of :class:`~emcee_amd.EnsembleSampler`, on that member's results."""

    def __init__(self, batch, b):
        self._batch, self.index = batch, b
        self.nwalkers, self.ndim = batch.nwalkers, batch.ndim
        self.seed = batch.seeds[b]

    @property
    def iteration(self):
        return self._batch.iteration

    def get_chain(self, discard=0, thin=1, flat=False):
        return self._batch._read(0, self.index, self.index + 1, discard, thin, flat)[0]

    def get_log_prob(self, discard=0, thin=1, flat=False):
        return self._batch._read(1, self.index, self.index + 1, discard, thin, flat)[0]

    def get_blobs(self, discard=0, thin=1, flat=False):
        if not self._batch.nblobs:
            return None
        return self._batch._read(4, self.index, self.index + 1, discard, thin, flat)[0]

    def get_blob_summary(self, discard=0, thin=1, quantiles=(0.16, 0.5, 0.84), cov=True):
        """:meth:`EnsembleBatch.get_blob_summary` of this member alone, without the leading axis."""
        r = self._batch._summary(discard, thin, quantiles, cov, self.index, self.index + 1, plane=4)
        return _summary.BatchSummary(r.nsamples, *[None if a is None else a[0] for a in r[1:]])

    @property
    def acceptance_fraction(self):
        return self._batch.acceptance_fraction[self.index]

    def get_autocorr_time(self, discard=0, thin=1, c=5, tol=50, quiet=False, on_device=False):
        if on_device:
            tau, _, nt = self._batch._autocorr_device(discard, thin, c, self.index, self.index + 1)
            _check_tol(tau, nt, tol, quiet, [self.index], tau[0])
            return thin * tau[0]
        x = self.get_chain(discard=discard, thin=thin)
        return thin * integrated_time(x, c=c, tol=tol, quiet=quiet)

    def get_rhat(self, discard=0, thin=1, chains="walkers", log_prob=False):
        """:meth:`EnsembleBatch.get_rhat` of this member alone, its walkers as chains, without the leading axis: what
        ``EnsembleSampler.get_rhat`` returns.  One ensemble is one group: only ``chains="walkers"`` (``ValueError`` otherwise)."""
        _summary.check_chains(chains, ("walkers",))
        r = self._batch._rhat(discard, thin, self.index, self.index + 1, 0, log_prob)
        return _summary.RHat(r.rhat[0], r.within[0], r.between[0], r.nchains, r.length)

    def get_summary(self, discard=0, thin=1, quantiles=(0.16, 0.5, 0.84), cov=True):
        """:meth:`EnsembleBatch.get_summary` of this member alone, without the leading axis."""
        r = self._batch._summary(discard, thin, quantiles, cov, self.index, self.index + 1)
        return _summary.BatchSummary(r.nsamples, *[None if a is None else a[0] for a in r[1:]])

    def get_histograms(self, bins=64, range=None, discard=0, thin=1, pairs="all", pair_bins=None):
        """:meth:`EnsembleBatch.get_histograms` of this member alone -> a plain :class:`~emcee_amd.summary.Histograms`, what
        ``EnsembleSampler.get_histograms`` returns (``range``: None, ``(lo, hi)`` or ``(ndim, 2)``)."""
        return self._histograms(0, bins, range, discard, thin, pairs, pair_bins)

    def get_blob_histograms(self, bins=64, range=None, discard=0, thin=1, pairs="all", pair_bins=None):
        """:meth:`EnsembleBatch.get_blob_histograms` of this member alone -> a plain :class:`~emcee_amd.summary.Histograms`."""
        return self._histograms(4, bins, range, discard, thin, pairs, pair_bins)

    def _histograms(self, plane, bins, rng, discard, thin, pairs, pair_bins):
        r = self._batch._histograms(plane, bins, _summary.check_range(rng), discard, thin, pairs, pair_bins, self.index, self.index + 1)
        return _summary.Histograms(r.nsamples, [e[0] for e in r.edges], [c[0] for c in r.counts], r.pairs, [e[0] for e in r.pair_edges],
                                   [c[0] for c in r.pair_counts])

    def get_last_sample(self):
        s = self._batch.get_last_sample()
        return State(s.coords[self.index], log_prob=s.log_prob[self.index], blobs=None if s.blobs is None else s.blobs[self.index])


EnsembleBatch.get_rhat.__doc__ = EnsembleBatch.get_rhat.__doc__ % _summary.RHAT_DEFINITION
