"""Device-resident log-probability targets.

Passing one of these as ``log_prob_fn`` lets :class:`emcee_amd.EnsembleSampler` fuse the
batched log-prob evaluation (reference ``ensemble.py:458-553``) into the half-step kernel.
Any other callable still works: proposals and the Metropolis accept stay on the GPU and only
the callable itself runs on the host (split-phase path).

Calling a target object evaluates it ON THE DEVICE (through ``emx_eval_log_prob``); there is
no NumPy twin in the product.  The formulas are restated for the parity tests in
``oracle/sampler_oracle.py`` only.
"""
import ctypes
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np

from . import _lib

__all__ = ["DeviceTarget", "IsoGaussian", "DiagGaussian", "DenseGaussian", "Rosenbrock", "UniformBox", "DeviceCallable", "DeviceKernel",
           "BatchCallable", "BatchKernel", "BatchFused", "BatchFusedLibrary", "compile_fused", "get_include", "PTFused", "PTFusedLibrary",
           "compile_fused_pt", "DeviceFused", "DeviceFusedLibrary", "compile_fused_ensemble", "fused_data_sum"]


class DeviceTarget(object):
    """Base class: subclasses provide ``kind`` and the parameter arrays."""

    kind = _lib.TARGET_HOST
    ndim = None

    def emx_params(self):
        """-> (kind, p0, p1, scale) for emx_set_target."""
        return self.kind, None, None, 0.0

    def bind(self, ens):
        kind, p0, p1, scale = self.emx_params()
        ens.set_target(kind, p0, p1, scale)

    def __call__(self, x):
        from .device import DeviceEnsemble
        x = np.asarray(x, dtype=np.float64)
        single = x.ndim == 1
        rows = np.atleast_2d(x)
        key = rows.shape[1]
        cache = self.__dict__.setdefault("_eval_ctx", {})
        ens = cache.get(key)
        if ens is None:
            ens = DeviceEnsemble(max(1024, 2), key)
            self.bind(ens)
            cache[key] = ens
        out = ens.eval_log_prob(rows)
        return float(out[0]) if single else out

    def __getstate__(self):
        d = dict(self.__dict__)
        d.pop("_eval_ctx", None)
        return d


class IsoGaussian(DeviceTarget):
    """log p = -0.5 sum(x^2)   (reference tests/integration/test_proposal.py:21-22)."""
    kind = _lib.TARGET_ISO


class DiagGaussian(DeviceTarget):
    """log p = -0.5 sum(ivar (x - mean)^2)   (reference docs/index.rst:41-45)."""
    kind = _lib.TARGET_DIAG

    def __init__(self, mean, ivar):
        self.mean = np.ascontiguousarray(mean, dtype=np.float64)
        self.ivar = np.ascontiguousarray(ivar, dtype=np.float64)
        if self.mean.shape != self.ivar.shape or self.mean.ndim != 1:
            raise ValueError("mean and ivar must be 1-d arrays of equal length")
        self.ndim = len(self.mean)

    def emx_params(self):
        return self.kind, self.mean, self.ivar, 0.0


class DenseGaussian(DeviceTarget):
    """log p = -0.5 (x - mean)^T icov (x - mean)   (reference docs/tutorials/quickstart.ipynb:76).

    Evaluated with v_mfma_f64_16x16x4_f64 against the Cholesky factor of ``icov``: LDS-resident and fused into the
    half-step kernel up to ndim 128, streamed through LDS by a log-prob kernel of its own up to ndim 2048."""
    kind = _lib.TARGET_DENSE

    def __init__(self, mean, icov):
        self.mean = np.ascontiguousarray(mean, dtype=np.float64)
        self.icov = np.ascontiguousarray(icov, dtype=np.float64)
        n = len(self.mean)
        if self.icov.shape != (n, n):
            raise ValueError("icov must be (ndim, ndim)")
        self.ndim = n

    def emx_params(self):
        return self.kind, self.mean, self.icov, 0.0


class Rosenbrock(DeviceTarget):
    """log p = -sum_i [100 (x_{i+1} - x_i^2)^2 + (1 - x_i)^2] / scale   (BASELINE config 3)."""
    kind = _lib.TARGET_ROSENBROCK

    def __init__(self, scale=20.0):
        self.scale = float(scale)

    def emx_params(self):
        return self.kind, None, None, self.scale


class UniformBox(DeviceTarget):
    """0 inside [0, 1]^ndim, -inf outside   (reference test_proposal.py:25-28)."""
    kind = _lib.TARGET_BOX


class DeviceCallable(DeviceTarget):
    """A user's vectorised ``log_prob_fn`` that runs on the GPU: ``fn(q)`` receives the ``(n, ndim)`` block of a split's
    proposals as a float64 CUDA tensor -- a zero-copy view of the library's buffer, rows in the order the reference passes them
    (``ensemble.py:486-487``, called at ``red_blue.py:93``) -- and returns their ``n`` log-probabilities as a CUDA tensor.
    Nothing crosses PCIe and nothing synchronises per split: the proposal kernel, ``fn``'s kernels and the accept / commit kernel
    are enqueued on one stream, and ``run_mcmc`` stays one native call.  ``-inf`` is legal; NaN raises the reference's error.
    Blobs are not supported on this path (use an ordinary callable).

        mu_t, icov_t = torch.as_tensor(mu).cuda(), torch.as_tensor(icov).cuda()
        def log_prob(q):                       # q: torch.float64 (n, ndim) on the GPU
            d = q - mu_t
            return -0.5 * ((d @ icov_t) * d).sum(1)
        sampler = EnsembleSampler(nwalkers, ndim, DeviceCallable(log_prob))
    """
    kind = _lib.TARGET_CALLBACK

    def __init__(self, fn, graph=False):
        """``graph=True``: after two eager calls per split shape the kernels ``fn`` launches are captured in a HIP graph and
        replayed (``fn`` must then be a pure function of its argument: same operations, same shapes every call)."""
        if not callable(fn):
            raise TypeError("DeviceCallable needs a callable")
        self.fn = fn
        self.graph = bool(graph)

    def bind(self, ens):
        if getattr(ens, "_cb_owner", None) is not self:
            ens.set_target_callback(self.fn, graph=self.graph)
            ens._cb_owner = self


class DeviceKernel(DeviceTarget):
    """A native log-probability: a C function with the signature ``emx_device_log_prob_fn`` of ``include/emx.h`` (typically one
    that launches the user's own HIP kernel on the stream it is handed) and its opaque ``user`` pointer.  The whole step stays
    three kernel launches per split -- proposal, the user's kernel, accept / commit -- with no Python in between."""
    kind = _lib.TARGET_CALLBACK

    def __init__(self, fn_ptr, user_ptr=None):
        self.fn_ptr, self.user_ptr = fn_ptr, user_ptr

    def bind(self, ens):
        if getattr(ens, "_cb_owner", None) is not self:
            ens.set_target_callback_c(self.fn_ptr, self.user_ptr)
            ens._cb_owner = self


def _check_launcher(fn_ptr, message):
    """a launcher or native callback: a ctypes function or a non-null address (an integer or a ``ctypes.c_void_p``), else TypeError(message)"""
    if not isinstance(fn_ptr, ctypes._CFuncPtr):
        addr = fn_ptr.value if isinstance(fn_ptr, ctypes.c_void_p) else fn_ptr
        if isinstance(addr, bool) or not isinstance(addr, (int, np.integer)) or not addr:
            raise TypeError(message)


def _check_user(who, user, readers="the functor reads"):
    """a fused target's ``user``: None, an integer, a ``ctypes.c_void_p`` or a torch CUDA tensor"""
    if not (user is None or isinstance(user, (int, np.integer, ctypes.c_void_p)) or hasattr(user, "data_ptr")) or isinstance(user, bool):
        raise TypeError("%s's user is a device pointer: None, an integer, a ctypes.c_void_p or a torch CUDA tensor" % who)
    if hasattr(user, "data_ptr") and not getattr(user, "is_cuda", False):
        raise TypeError("%s's user tensor must live on the GPU (%s it on the device)" % (who, readers))


class _FusedUser(object):
    """the ``user`` of the fused targets"""

    def user_address(self):
        """-> the device address handed to the functor (None: a null pointer)"""
        u = self.user
        if u is None:
            return None
        if hasattr(u, "data_ptr"):
            return int(u.data_ptr())
        return u.value if isinstance(u, ctypes.c_void_p) else int(u)


class DeviceFused(_FusedUser, DeviceTarget):
    """The user's per-row ``__device__`` log-probability compiled INTO the half-step kernel of :class:`~emcee_amd.EnsembleSampler`:
    ``fn_ptr`` is the launcher that ``EMX_FUSED_ENSEMBLE_TARGET(name, Functor, ndim)`` of ``emx_fused_ensemble.hpp`` emits in the
    user's own translation unit (an ``emx_fused_ensemble_fn`` of ``include/emx.h``: a ctypes function or a non-null address),
    ``ndim`` the dimension it was compiled for (1 ... 256), ``user`` the device pointer the functor receives with every row -- None,
    an integer, a ``ctypes.c_void_p``, or a torch CUDA tensor (kept alive; its ``data_ptr()`` is passed).

    A half-step is then ONE kernel launch -- proposal, the user's function on the row staged in LDS, accept / commit -- where a
    :class:`DeviceKernel` takes three and sends the proposal block through memory; the run is bit for bit the :class:`DeviceKernel`
    run of the same function, with every move that path runs, in both rng modes.  The functor contract is :class:`BatchFused`'s
    (``member`` is always 0), so one model source serves both; :func:`compile_fused_ensemble` builds the launcher from source.
    One GPU only (``distributed=True`` is refused).  Not a target of :class:`~emcee_amd.EnsembleBatch` or
    :class:`~emcee_amd.PTSampler`, and not callable outside a sampler.

    ``nblobs = K > 0``: the launcher was emitted by ``EMX_FUSED_ENSEMBLE_TARGET_BLOBS(name, Functor, ndim, K)`` around the functor's
    five-argument form ``(x, ndim, member, user, double* blobs)``, which writes K float64 derived quantities a row in the call
    that returns the log-probability.  They stay on the device next to the chain -- ``get_blobs``, ``get_last_sample().blobs``,
    ``compute_log_prob(x)[1]`` and the returned state's ``.blobs`` read them from there, ``(nsteps, nwalkers, K)``, or ``(nsteps,
    nwalkers)`` for ``K == 1`` -- and the run stays one launch per half-step, the samples those of the blob-free functor.  A
    launcher compiled for another count is refused when the target is bound; ``WalkMove`` / ``KDEMove`` are refused with blobs.

    ``small_fn``: the launcher that ``EMX_FUSED_ENSEMBLE_SMALL_TARGET(name, Functor, ndim)`` (``..._SMALL_TARGET_BLOBS`` with blobs)
    emits next to ``fn_ptr`` in the same translation unit (:func:`compile_fused_ensemble` does by default).  An ensemble that fits
    one workgroup's LDS -- the common 32 to a few hundred walkers at 5 to 20 parameters; ``emx_small_fused_check`` of
    ``include/emx.h`` has the rule -- then runs whole ``run_mcmc`` calls inside one workgroup, one launch per chunk of steps, in both
    rng modes, with or without blobs, to the same bits -- where that was measured faster (``emx_small_fused_pays``: ndim <= 16 under
    ``rng="mt19937"``, ndim <= 10 and nwalkers x ndim <= 1 024 under ``rng="philox"``).  Larger ensembles, ``WalkMove`` / ``KDEMove``
    schedules, a ``GaussianMove`` under ``rng="mt19937"`` and ``sample()`` driven step by step keep the launch per half-step.  None:
    always that path.

    ``ndata`` (an integer, ``0 <= ndata < 2**31``): the log-probability sums over data, ``base(x) + sum_k term(x; datum k)``, and
    ``fn_ptr`` is the launcher that ``EMX_FUSED_ENSEMBLE_DATA_TARGET(name, Model, ndim)`` of ``emx_fused_ensemble_data.hpp`` emits
    around a model with ``base`` and ``term`` members.  The half-step then gives every row a WAVE for the data sum -- one lane calls
    ``base``, 64 lanes stride over the data, a fixed pairwise tree adds the lane partials -- where the plain functor would loop over
    the data in one lane, and a mid-size ensemble is spread over the chip in small tiles.  The value of a row is defined by the
    header and reproduced on the host by :func:`fused_data_sum`; the run is bit for bit the :class:`DeviceKernel` run of a kernel
    that sums in that order.  ``ndata`` is a run-time value: one launcher serves every data set.  No blobs and no ``small_fn``
    with ``ndata`` (``ValueError``); such a target always runs one launch a half-step.  Where it pays, measured on the
    straight-line fit against the one-lane functor of the same model (``profiles/ensemble_fused_data.md``): at 1 024 and 4 096
    walkers from the smallest count measured, 64 data (3 to 4 times the speed; 17 to 25 times at 1 024 data, 35 to 48 times at
    16 384); at 65 536 walkers the crossover lies between 64 data (0.89 times the speed of a plain one-accumulator loop, 1.95 times
    that of the loop in the data target's order) and 1 024 data (3.9 and 9.6 times), with 6.6 and 16 times at 16 384."""
    kind = _lib.TARGET_FUSED_ENSEMBLE

    def __init__(self, fn_ptr, ndim, user=None, nblobs=0, small_fn=None, ndata=None):
        _check_launcher(fn_ptr, "DeviceFused needs an emx_fused_ensemble_fn: a ctypes function or a non-null address")
        if isinstance(ndim, bool) or not isinstance(ndim, (int, np.integer)) or not 1 <= ndim <= 256:
            raise TypeError("DeviceFused needs the ndim its launcher was compiled for, an integer in [1, 256]; got %r" % (ndim,))
        _check_user("DeviceFused", user)
        if small_fn is not None:
            _check_launcher(small_fn, "DeviceFused's small_fn is an EMX_FUSED_ENSEMBLE_SMALL_TARGET launcher: a ctypes function, a non-null address or None")
        self.fn_ptr, self.ndim, self.user, self.small_fn = fn_ptr, int(ndim), user, small_fn
        self.nblobs = _check_nblobs("DeviceFused", nblobs)
        self.ndata = _check_ndata("DeviceFused", ndata)
        if self.ndata is not None and self.nblobs > 0:
            raise ValueError("DeviceFused: a target that sums over data (ndata) carries no blobs; nblobs=%d is refused" % self.nblobs)
        if self.ndata is not None and small_fn is not None:
            raise ValueError("DeviceFused: a target that sums over data (ndata) has no one-workgroup form; small_fn is refused")

    def bind(self, ens):
        if ens.ndim != self.ndim:
            raise ValueError("the DeviceFused target was compiled for ndim %d; the sampler has ndim %d" % (self.ndim, ens.ndim))
        if getattr(ens, "_cb_owner", None) is not self or ens._target_kind != self.kind:
            if self.ndata is not None:
                ens.set_target_fused(self.fn_ptr, self.user_address(), ndata=self.ndata)
            else:
                ens.set_target_fused(self.fn_ptr, self.user_address(), self.nblobs, small_fn=self.small_fn)
            ens._cb_owner = self

    def __call__(self, x):
        raise TypeError("DeviceFused is evaluated inside EnsembleSampler's kernels on the device (sampler.compute_log_prob(x) evaluates rows)")


def _check_nblobs(who, nblobs):
    if isinstance(nblobs, bool) or not isinstance(nblobs, (int, np.integer)) or not 0 <= nblobs <= _lib.MAX_BLOBS:
        raise ValueError("%s: nblobs is an integer in [0, %d] (float64 blobs a sample); got %r" % (who, _lib.MAX_BLOBS, nblobs))
    return int(nblobs)


def _check_ndata(who, ndata):
    if ndata is None:
        return None
    if isinstance(ndata, bool) or not isinstance(ndata, (int, np.integer)) or not 0 <= ndata < 2 ** 31:
        raise ValueError("%s: ndata is an integer in [0, 2**31) (the data the target's term runs over), or None; got %r" % (who, ndata))
    return int(ndata)


def _check_member_ndata(who, ndata):
    """one count for every member (_check_ndata), or a sequence / array with one a member -> None, an int or a tuple of ints"""
    if ndata is None or isinstance(ndata, (bool, int, float, np.generic)):
        return _check_ndata(who, ndata)
    return tuple(_check_ndata(who, n) for n in (ndata.tolist() if isinstance(ndata, np.ndarray) and ndata.dtype == object else list(ndata)))


def fused_data_sum(terms):
    """Sum a 1-d float64 array in the order a data target's kernel sums its terms (``emx_fused_ensemble_data.hpp``): lane partial
    ``p[l]``, ``l = 0 ... 63``, starts at +0.0 and adds ``terms[k]`` for ``k = l, l + 64, l + 128, ...`` in ascending ``k``; the
    result is the balanced pairwise tree over ``p[0] ... p[63]``, adjacent pairs level by level.  With it the host reproduces a
    device log-probability bit for bit: ``base + fused_data_sum(terms)``.  An empty array gives 0.0."""
    t = np.asarray(terms, dtype=np.float64)
    if t.ndim != 1:
        raise ValueError("fused_data_sum: a 1-d array of terms; got shape %r" % (t.shape,))
    n = t.shape[0]
    pad = np.zeros(((n + 63) // 64) * 64, dtype=np.float64)
    pad[:n] = t
    p = np.zeros(64, dtype=np.float64)
    for row in pad.reshape(-1, 64)[:n // 64]:        # whole strides: every lane adds
        p = p + row
    if n % 64:
        p[:n % 64] = p[:n % 64] + pad[n - n % 64:n]  # the last, partial stride: the lanes past the end add nothing
    while p.shape[0] > 1:
        p = p[0::2] + p[1::2]
    return float(p[0])


class BatchTarget(DeviceTarget):
    """Base of the batched callback targets of :class:`~emcee_amd.EnsembleBatch` (``emx_set_batch_target_callback``): one call
    evaluates the proposals of every member of a batch.  They are not targets of a single ensemble."""
    kind = _lib.TARGET_CALLBACK
    nblobs = 0                            # blobs a sample (EnsembleBatch.get_blobs); the built-in targets have none

    def bind(self, ens):
        raise TypeError("%s is a target of EnsembleBatch, not of a single ensemble (use DeviceCallable with EnsembleSampler)"
                        % type(self).__name__)

    def __call__(self, x):
        raise TypeError("%s is evaluated by EnsembleBatch on the device" % type(self).__name__)


class BatchCallable(BatchTarget):
    """A user's log-probability over every member of an :class:`~emcee_amd.EnsembleBatch` at once: ``fn(q)`` receives a float64
    CUDA tensor ``(B, n, ndim)`` -- a zero-copy view of the library's proposal block, ``q[b]`` member b's rows -- and returns
    ``(B, n)`` (or ``B * n``) log-probabilities, anything ``torch.as_tensor`` takes on the device.  Per-member data (catalogue
    rows, per-object parameters) lives in ``fn``'s closure as ``(B, ...)`` tensors.  ``-inf`` is legal; NaN raises the
    reference's error naming the member; an exception raised by ``fn`` comes out of ``run_mcmc`` as itself.  Every row must be
    computed on its own, independently of the block's shape: rows past a member's split size are padding (copies of its current
    walkers) whose values are ignored.

        mu_t, ivar_t = torch.as_tensor(mu).cuda()[:, None, :], torch.as_tensor(ivar).cuda()[:, None, :]    # (B, 1, ndim)
        def log_prob(q):                       # q: torch.float64 (B, n, ndim) on the GPU
            d = q - mu_t
            return -0.5 * (ivar_t * d * d).sum(-1)
        batch = EnsembleBatch(B, nwalkers, ndim, BatchCallable(log_prob), seeds=seeds)

    ``nblobs = K > 0``: ``fn(q)`` returns ``(lp, blobs)`` with ``blobs`` of shape ``(B, n, K)``, K float64 derived quantities
    a row, kept with every sample (``EnsembleBatch.get_blobs``).
    """

    def __init__(self, fn, nblobs=0):
        if not callable(fn):
            raise TypeError("BatchCallable needs a callable")
        self.fn, self.nblobs = fn, _check_nblobs("BatchCallable", nblobs)


class BatchKernel(BatchTarget):
    """A native batched log-probability: a C function with the signature ``emx_batch_log_prob_fn`` of ``include/emx.h``
    (typically one that launches the user's own HIP kernel on the stream it is handed) and its opaque ``user`` pointer.  A
    proposal step is then library launches and calls of that function alone, with no Python in between.  With ``nblobs = K > 0``
    the function has the signature ``emx_batch_log_prob_blobs_fn`` and also writes a ``(nbatch, rows, K)`` block of blobs."""

    def __init__(self, fn_ptr, user_ptr=None, nblobs=0):
        _check_launcher(fn_ptr, "BatchKernel needs an emx_batch_log_prob_fn: a ctypes function or a non-null address")
        self.fn_ptr, self.user_ptr, self.nblobs = fn_ptr, user_ptr, _check_nblobs("BatchKernel", nblobs)


class BatchFused(_FusedUser, BatchTarget):
    """The user's per-row ``__device__`` log-probability compiled INTO the batch kernel: ``fn_ptr`` is the launcher that
    ``EMX_FUSED_BATCH_TARGET(name, Functor, ndim)`` of ``emx_fused_target.hpp`` emits in the user's own translation unit (an
    ``emx_fused_batch_fn`` of ``include/emx.h``: a ctypes function or a non-null address), ``ndim`` the dimension it was compiled
    for, ``user`` the device pointer the functor receives with every row -- an integer, a ``ctypes.c_void_p``, or a torch CUDA
    tensor (kept alive; its ``data_ptr()`` is passed) -- holding the per-member data the functor indexes by ``member``.

    :class:`~emcee_amd.EnsembleBatch` then runs as it does for a built-in target: one launch per ``run_mcmc`` chunk, no callback,
    no proposal block in global memory, bit for bit the :class:`BatchKernel` run of the same function.
    :func:`compile_fused` builds such a launcher from source.  Not a likelihood of :class:`~emcee_amd.PTSampler` (its launcher
    carries the untempered kernel): the tempered form is :class:`PTFused`.

    ``nblobs = K > 0``: the launcher was emitted by ``EMX_FUSED_BATCH_TARGET_BLOBS(name, Functor, ndim, K)`` around the functor's
    five-argument form, which writes K doubles a row (``EnsembleBatch.get_blobs``); a launcher compiled for another count is
    refused when the target is bound.

    ``ndata`` (an integer for every member, or a sequence / array of ``nbatch`` integers, each ``0 <= ndata < 2**31``): the
    log-probability sums over per-member data, ``base(x) + sum_k term(x; datum k)``, and ``fn_ptr`` is the launcher that
    ``EMX_FUSED_BATCH_DATA_TARGET(name, Model, ndim)`` of ``emx_fused_target_data.hpp`` emits around a model with ``base(x, ndim,
    member, user)`` and ``term(x, ndim, member, k, user)`` members (an ``emx_fused_batch_data_fn``).  The kernel then gives every
    proposal a WAVE for the data sum -- one lane calls ``base``, 64 lanes stride over the member's ``ndata[member]`` data, a fixed
    pairwise tree adds the lane partials, the wave commits the row -- where the plain functor loops over the data in one of the
    few lanes a small ensemble keeps busy.  The counts are run-time values and may differ from member to member (a catalogue's
    objects have different numbers of points): one launcher serves them all.  The value of a row is defined by the header and
    reproduced on the host by :func:`fused_data_sum`; member b is bit for bit the :class:`~emcee_amd.EnsembleSampler` run of the
    same model as a :class:`DeviceFused` with ``ndata[b]`` under ``rng="philox"``.  Everything else of the batch -- one launch per
    chunk, ``get_summary``, ``get_histograms``, the device autocorrelation times, thinning, ``store=False`` -- is unchanged.  No
    blobs with ``ndata`` (``ValueError``); a length other than ``nbatch`` is refused when the batch takes the target.  Where it pays,
    measured on a straight-line fit against the one-lane, one-accumulator functor of the same model
    (``profiles/batch_fused_data.md``): at 64 members of 32 x 5 from the smallest count measured (1.17 times the speed at 16 data,
    12 times at 1 024); at 1 024 members, which share CUs, from 256 data (0.34 times at 16, 1.9 times at 256, 3.6 times at 1 024)."""
    kind = _lib.TARGET_FUSED_USER

    def __init__(self, fn_ptr, ndim, user=None, nblobs=0, ndata=None):
        _check_launcher(fn_ptr, "BatchFused needs an emx_fused_batch_fn: a ctypes function or a non-null address")
        if isinstance(ndim, bool) or not isinstance(ndim, (int, np.integer)) or ndim < 1:
            raise TypeError("BatchFused needs the ndim its launcher was compiled for, an integer >= 1; got %r" % (ndim,))
        _check_user("BatchFused", user)
        self.fn_ptr, self.ndim, self.user = fn_ptr, int(ndim), user
        self.nblobs = _check_nblobs("BatchFused", nblobs)
        self.ndata = _check_member_ndata("BatchFused", ndata)
        if self.ndata is not None and self.nblobs > 0:
            raise ValueError("BatchFused: a target that sums over data (ndata) carries no blobs; nblobs=%d is refused" % self.nblobs)

class PTFused(_FusedUser, BatchTarget):
    """The user's per-row ``__device__`` log-likelihood (and, optionally, log-prior) compiled INTO the tempered kernel of
    :class:`~emcee_amd.PTSampler`: ``fn_ptr`` is the launcher that ``EMX_FUSED_PT_TARGET(name, LikeFunctor, PriorFunctor, ndim)`` of
    ``emx_pt_fused.hpp`` emits in the user's own translation unit (an ``emx_pt_fused_fn`` of ``include/emx.h``), ``ndim`` the
    dimension it was compiled for, ``user`` the device pointer both functors receive with every row (as :class:`BatchFused`'s); the
    functors' ``member`` is ``object * ntemps + rung``.  ``has_prior``: whether the launcher carries a prior functor (None: not
    known before the launcher is probed at the first run).

    One workgroup then runs one object -- all its rungs, the swap pass and the ladder adaptation -- in LDS: one launch per
    ``run_mcmc`` chunk, bit for bit the :class:`BatchKernel` run of the same functions.  :func:`compile_fused_pt` builds such a
    launcher from source.  A likelihood of :class:`~emcee_amd.PTSampler` only.

    ``ndata`` (an integer for every object, or a sequence / array of ``nbatch`` integers, one count an object, each ``0 <= ndata <
    2**31``; None: the plain target above): the log-likelihood sums over the object's data, ``base(x) + sum_k term(x; datum k)``, and
    ``fn_ptr`` is the launcher that ``EMX_FUSED_PT_DATA_TARGET(name, Model, PriorFunctor, ndim)`` of ``emx_pt_fused_data.hpp`` emits
    around a model with ``base(x, ndim, member, user)`` and ``term(x, ndim, member, k, user)`` members (:class:`BatchFused`'s data
    contract).  Every rung of an object sees the object's data.  The tempered kernel then gives every proposal a WAVE for the data sum
    -- one lane evaluates the prior and ``base``, 64 lanes stride over the data, a fixed pairwise tree adds the lane partials, the
    wave commits the row -- where the plain functor loops over the data in one of the ``ntemps x rows`` lanes the second pass keeps
    busy.  The value of a row is the one ``emx_fused_target_data.hpp`` defines, reproduced on the host by :func:`fused_data_sum`; a
    row outside the prior does not reach the model; the run is bit for bit the plain :class:`PTFused` run of a one-lane functor that
    computes the same value.  A length other than ``nbatch`` is refused when the sampler takes the target.  Nothing chooses between
    the two forms for the user.  Where it pays, measured on a straight-line fit against the one-lane, one-accumulator functor
    (``profiles/pt_fused_data.md``): at 8 rungs of 32 x 5 from about 1 024 data an object (2.0 times the speed there, 2.6 to 2.8
    times at 4 096; 3.4 times SLOWER at 16 data, 12 to 15 % slower at 256); at 8 rungs of 64 x 16 only at 4 096 (1.5 times).

    ``nblobs = K > 0``: the launcher was emitted by ``EMX_FUSED_PT_TARGET_BLOBS(name, LikeFunctor, PriorFunctor, ndim, K)`` around the
    likelihood's five-argument form ``(x, ndim, member, user, double* blobs)``, which writes K float64 derived quantities a row
    (``PTSampler.get_blobs``; the semantics are in the ``pt`` module's docstring).  A launcher compiled for another count is refused
    when the target is bound.  No blobs with ``ndata`` (``ValueError``)."""

    def __init__(self, fn_ptr, ndim, user=None, nblobs=0, has_prior=None, ndata=None):
        _check_launcher(fn_ptr, "PTFused needs an emx_pt_fused_fn: a ctypes function or a non-null address")
        if isinstance(ndim, bool) or not isinstance(ndim, (int, np.integer)) or ndim < 1:
            raise TypeError("PTFused needs the ndim its launcher was compiled for, an integer >= 1; got %r" % (ndim,))
        _check_user("PTFused", user, "the functors read")
        self.fn_ptr, self.ndim, self.user = fn_ptr, int(ndim), user
        self.has_prior = None if has_prior is None else bool(has_prior)
        self.ndata = _check_member_ndata("PTFused", ndata)
        self.nblobs = _check_nblobs("PTFused", nblobs)
        if self.ndata is not None and self.nblobs > 0:
            raise ValueError("PTFused: a target that sums over data (ndata) carries no blobs; nblobs=%d is refused" % self.nblobs)


def get_include():
    """-> [``include/``, ``emcee_amd/csrc/``]: the directories a build of the user's own fused target needs on its include path
    (``emx.h`` and ``emx_fused_target.hpp``)."""
    here = os.path.dirname(os.path.abspath(__file__))
    return [os.path.join(os.path.dirname(here), "include"), os.path.join(here, "csrc")]


class _FusedLibrary(object):
    """Base of what the three compile functions build: ``path``, ``lib`` (the ``ctypes.CDLL``), ``name`` and ``launcher``, ``ndim``,
    ``data``, and the refusals of :meth:`target`'s ``ndata`` in the words of the class (``_who``, ``_compiler``, ``_counts``)."""

    def __init__(self, path, name, ndim, data):
        self.path, self.name, self.ndim = path, name, int(ndim)
        self.data = bool(data)            # the launcher is a data-target one: target() takes the data counts
        _lib.load()                       # one HIP runtime per process: the library's (torch's) first
        self.lib = ctypes.CDLL(path)
        self.launcher = getattr(self.lib, name)

    def _check_target_ndata(self, ndata):
        if self.data and ndata is None:
            raise ValueError("%s.target: the library was built with data=True; give ndata, %s" % (self._who, self._counts))
        if not self.data and ndata is not None:
            raise ValueError("%s.target: ndata is for a library built with %s(..., data=True)" % (self._who, self._compiler))


class BatchFusedLibrary(_FusedLibrary):
    """What :func:`compile_fused` built: ``path`` of the shared library, ``lib`` (its ``ctypes.CDLL``: the user's own ``extern
    "C"`` setup functions of ``source`` are there), ``name`` of the launcher, ``ndim``, ``nblobs``, ``data`` (the launcher is an
    ``EMX_FUSED_BATCH_DATA_TARGET`` one) and :meth:`target`."""

    _who, _compiler, _counts = "BatchFusedLibrary", "compile_fused", "the members' numbers of data"

    def __init__(self, path, name, ndim, nblobs=0, data=False):
        self.nblobs = int(nblobs)
        _FusedLibrary.__init__(self, path, name, ndim, data)

    def target(self, user=None, ndata=None):
        """-> :class:`BatchFused` of the compiled functor with the device pointer ``user``; a library built with ``data=True``
        needs ``ndata`` -- the data every member's ``term`` runs over, an integer or ``nbatch`` of them -- and any other refuses it"""
        self._check_target_ndata(ndata)
        t = BatchFused(self.launcher, self.ndim, user, nblobs=self.nblobs, ndata=ndata)
        t._library = self                 # the launcher's code lives as long as the target
        return t


FUSED_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC"]


def _compile_cached(what, header, source, tail, key_parts, name, flags, cache_dir):
    """the shared build of compile_fused, compile_fused_ensemble and compile_fused_pt: cache key, translation unit, hipcc, diagnostics -> path of the library"""
    from . import _build
    h = hashlib.sha256(repr(key_parts + (FUSED_FLAGS + flags,)).encode())
    for d in _build.DEPS:
        if d.endswith((".hpp", ".h")):
            with open(d, "rb") as f:
                h.update(f.read())
    key = h.hexdigest()[:24]
    cache_dir = cache_dir or os.environ.get("EMCEE_AMD_CACHE") or os.path.join(os.path.expanduser("~"), ".cache", "emcee_amd")
    work = os.path.join(str(cache_dir), key)
    so = os.path.join(work, "lib%s.so" % name)
    if not os.path.exists(so):
        os.makedirs(work, exist_ok=True)
        src = os.path.join(work, "%s.hip" % name)
        with open(src, "w") as f:
            f.write("#include <%s>\n\n%s\n\n%s\n" % (header, source, tail))
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        tmp = "%s.%d.tmp" % (so, os.getpid())
        cmd = [hipcc] + FUSED_FLAGS + flags + ["-I" + d for d in get_include()] + [src, "-o", tmp]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            if os.path.exists(tmp):
                os.remove(tmp)
            raise RuntimeError("%s: hipcc failed (%s):\n%s" % (what, src, (r.stderr or r.stdout)[-4000:]))
        os.replace(tmp, so)
    return so


def _compile_ndim(who, ndim):
    ndim = int(ndim)
    if ndim < 1 or ndim > 256:
        raise ValueError("%s: 1 <= ndim <= 256; got %d" % (who, ndim))
    return ndim


def _compile_nblobs(who, nblobs, data):
    nblobs = _check_nblobs(who, nblobs)
    if data and nblobs:
        raise ValueError("%s: a data target (data=True) carries no blobs; nblobs=%d is refused" % (who, nblobs))
    return nblobs


def _compile_names(who, prefix, ndim, idents, name, flags):
    """the identifier check of the functor types (``idents``: (what, identifier) pairs, the first one required) and of ``name``, the
    default launcher name, the flags as strings -> (name, flags)"""
    for what, ident in idents + (("name", name),):
        if (ident is not None or what == idents[0][0]) and not (isinstance(ident, str) and re.match(r"^[A-Za-z_][A-Za-z0-9_:]*$", ident)):
            raise ValueError("%s: %s must be a C++ identifier; got %r" % (who, what, ident))
    return name or "%s_%s_%d" % (prefix, idents[0][1].replace(":", "_"), ndim), [str(f) for f in flags]


def _compile_form(who, header, source, tail, data_tail, key, name, flags, cache_dir, data):
    """the plain translation unit, or with ``data`` the data header's and its tail under the key + ("data target",) -> path of the
    library.  (A plain build keeps the key, and with it the cached library, it always had.)"""
    if data:
        return _compile_cached(who, header.replace(".hpp", "_data.hpp"), source, data_tail, key + ("data target",), name, flags, cache_dir)
    return _compile_cached(who, header, source, tail, key, name, flags, cache_dir)


class DeviceFusedLibrary(_FusedLibrary):
    """What :func:`compile_fused_ensemble` built: ``path`` of the shared library, ``lib`` (its ``ctypes.CDLL``: the user's own
    ``extern "C"`` setup functions of ``source`` are there), ``name`` of the launcher, ``ndim``, ``nblobs``, ``small_name`` /
    ``small_launcher`` (the one-workgroup launcher, None when it was built with ``small=False``) and :meth:`target`."""

    _who, _compiler, _counts = "DeviceFusedLibrary", "compile_fused_ensemble", "the number of data"

    def __init__(self, path, name, ndim, nblobs=0, small_name=None, data=False):
        self.nblobs = _check_nblobs("DeviceFusedLibrary", nblobs)
        _FusedLibrary.__init__(self, path, name, ndim, data)
        self.small_name = small_name
        self.small_launcher = getattr(self.lib, small_name) if small_name else None

    def target(self, user=None, ndata=None):
        """-> :class:`DeviceFused` of the compiled functor with the device pointer ``user``; a library built with ``data=True``
        needs ``ndata``, the number of data its ``term`` runs over, and any other refuses it"""
        self._check_target_ndata(ndata)
        if self.data:
            t = DeviceFused(self.launcher, self.ndim, user, ndata=ndata)
        else:
            t = DeviceFused(self.launcher, self.ndim, user, nblobs=self.nblobs, small_fn=self.small_launcher)
        t._library = self                 # the launcher's code lives as long as the target
        return t


def compile_fused_ensemble(source, functor, ndim, name=None, flags=(), cache_dir=None, nblobs=0, small=True, data=False):
    """Compile the user's model into the single sampler's half-step kernel -> :class:`DeviceFusedLibrary`.

    ``source``: HIP C++ that defines the functor type ``functor`` -- ``__device__ double operator()(const double* x, int ndim, int
    member, const void* user) const``, the contract of :func:`compile_fused` (``member`` is 0 here) -- and whatever ``extern "C"``
    helpers the user wants in the same library.  The translation unit is ``#include <emx_fused_ensemble.hpp>``, ``source`` and
    ``EMX_FUSED_ENSEMBLE_TARGET(name, functor, ndim)``, compiled and cached as :func:`compile_fused` does (the same flags; the key is
    the hash of source, functor, ndim, name, flags and every header of the library, ``emx_fused_ensemble.hpp`` among them); a
    compiler failure raises ``RuntimeError`` with the compiler's last lines.

    ``nblobs = K > 0``: the functor has the five-argument form ``(x, ndim, member, user, double* blobs)`` and the translation unit
    ends in ``EMX_FUSED_ENSEMBLE_TARGET_BLOBS(name, functor, ndim, K)`` -- the source :func:`compile_fused` takes with ``nblobs``.

    ``small`` (default True): the translation unit also ends in ``EMX_FUSED_ENSEMBLE_SMALL_TARGET[_BLOBS](name_small, functor, ndim[,
    K])``, the one-workgroup launcher of ensembles that fit one workgroup's LDS (:class:`DeviceFused`'s ``small_fn``; four more
    kernels to compile, about 2 s more).  ``small=False`` builds the library without it: the translation unit it always was.

    ``data=True``: ``functor`` is a model with ``base(x, ndim, user)`` and ``term(x, ndim, k, user)`` members whose log-probability
    sums over data (:class:`DeviceFused`'s ``ndata``).  The translation unit is ``#include <emx_fused_ensemble_data.hpp>``,
    ``source`` and ``EMX_FUSED_ENSEMBLE_DATA_TARGET(name, functor, ndim)``; no one-workgroup launcher is emitted and ``nblobs``
    is refused.  ``data=False`` keeps the translation unit and the cache key it always had."""
    nblobs = _compile_nblobs("compile_fused_ensemble", nblobs, data)
    ndim = _compile_ndim("compile_fused_ensemble", ndim)
    name, flags = _compile_names("compile_fused_ensemble", "emx_fused_ensemble", ndim, (("functor", functor),), name, flags)
    tail = "EMX_FUSED_ENSEMBLE_TARGET(%s, %s, %d)" % (name, functor, ndim)
    key = ("ensemble", source, functor, ndim, name)
    if nblobs:                            # (a blob-free build keeps the key, and with it the cached library, it always had)
        tail = "EMX_FUSED_ENSEMBLE_TARGET_BLOBS(%s, %s, %d, %d)" % (name, functor, ndim, nblobs)
        key += ("nblobs", nblobs)
    small_name = name + "_small" if small and not data else None
    if small_name:
        tail += ("\nEMX_FUSED_ENSEMBLE_SMALL_TARGET_BLOBS(%s, %s, %d, %d)" % (small_name, functor, ndim, nblobs) if nblobs else
                 "\nEMX_FUSED_ENSEMBLE_SMALL_TARGET(%s, %s, %d)" % (small_name, functor, ndim))
    elif not data:                        # (the default build keeps the form of key it always had; the headers are part of its hash)
        key += ("half-step launcher only",)
    so = _compile_form("compile_fused_ensemble", "emx_fused_ensemble.hpp", source, tail,
                       "EMX_FUSED_ENSEMBLE_DATA_TARGET(%s, %s, %d)" % (name, functor, ndim), key, name, flags, cache_dir, data)
    return DeviceFusedLibrary(so, name, ndim, nblobs, small_name, data=data)


class PTFusedLibrary(_FusedLibrary):
    """What :func:`compile_fused_pt` built: ``path``, ``lib`` (its ``ctypes.CDLL``), ``name`` of the launcher, ``ndim``,
    ``has_prior``, ``data`` (the launcher is an ``EMX_FUSED_PT_DATA_TARGET`` one), ``nblobs`` and :meth:`target`."""

    _who, _compiler, _counts = "PTFusedLibrary", "compile_fused_pt", "the objects' numbers of data"
    nblobs = 0                            # (an instance attribute only of a library built with blobs)

    def __init__(self, path, name, ndim, has_prior, data=False, nblobs=0):
        self.has_prior = bool(has_prior)
        if _compile_nblobs("PTFusedLibrary", nblobs, data):
            self.nblobs = int(nblobs)
        _FusedLibrary.__init__(self, path, name, ndim, data)

    def target(self, user=None, ndata=None):
        """-> :class:`PTFused` of the compiled functors with the device pointer ``user``; a library built with ``data=True``
        needs ``ndata`` -- the data every object's ``term`` runs over, an integer or ``nbatch`` of them -- and any other refuses it"""
        self._check_target_ndata(ndata)
        t = PTFused(self.launcher, self.ndim, user, nblobs=self.nblobs, has_prior=self.has_prior, ndata=ndata)
        t._library = self                 # the launcher's code lives as long as the target
        return t


def compile_fused_pt(source, likelihood, ndim, prior=None, name=None, flags=(), cache_dir=None, data=False, nblobs=0):
    """Compile the user's model into the tempered kernel -> :class:`PTFusedLibrary`.

    ``source``: HIP C++ that defines the functor type ``likelihood`` and, unless ``prior`` is None, the functor type ``prior`` (both
    ``__device__ double operator()(const double* x, int ndim, int member, const void* user) const``).  The translation unit is
    ``#include <emx_pt_fused.hpp>``, ``source`` and ``EMX_FUSED_PT_TARGET(name, likelihood, prior or emx::NoFusedPrior, ndim)``,
    compiled and cached as :func:`compile_fused` does (the same flags; the key is the hash of source, both names, ndim, name, flags
    and every header of the library); a compiler failure raises ``RuntimeError`` with the compiler's last lines.

    ``data=True``: ``likelihood`` is a model with ``base(x, ndim, member, user)`` and ``term(x, ndim, member, k, user)`` members whose
    log-likelihood sums over the object's data (:class:`PTFused`'s ``ndata``); ``prior`` is what it is above.  The translation unit
    is ``#include <emx_pt_fused_data.hpp>``, ``source`` and ``EMX_FUSED_PT_DATA_TARGET(name, likelihood, prior or emx::NoFusedPrior,
    ndim)``.  ``data=False`` keeps the translation unit and the cache key it always had.

    ``nblobs = K > 0``: ``likelihood`` has the five-argument form ``(x, ndim, member, user, double* blobs)`` (the prior keeps four) and
    the translation unit ends in ``EMX_FUSED_PT_TARGET_BLOBS(name, likelihood, prior or emx::NoFusedPrior, ndim, K)``; K joins the
    cache key only then, so a blob-free build keeps the key and the cached library it always had.  Refused with ``data=True``: the
    data form carries no blobs."""
    nblobs = _compile_nblobs("compile_fused_pt", nblobs, data)
    ndim = _compile_ndim("compile_fused_pt", ndim)
    name, flags = _compile_names("compile_fused_pt", "emx_pt_fused", ndim, (("likelihood", likelihood), ("prior", prior)), name, flags)
    args = (name, likelihood, prior or "emx::NoFusedPrior", ndim)
    tail, key = "EMX_FUSED_PT_TARGET(%s, %s, %s, %d)" % args, ("pt", source, likelihood, prior, ndim, name)
    if nblobs:
        tail, key = "EMX_FUSED_PT_TARGET_BLOBS(%s, %s, %s, %d, %d)" % (args + (nblobs,)), key + ("nblobs", nblobs)
    so = _compile_form("compile_fused_pt", "emx_pt_fused.hpp", source, tail, "EMX_FUSED_PT_DATA_TARGET(%s, %s, %s, %d)" % args, key, name, flags,
                       cache_dir, data)
    return PTFusedLibrary(so, name, ndim, prior is not None, data=data, nblobs=nblobs)


def compile_fused(source, functor, ndim, nblobs=0, name=None, flags=(), cache_dir=None, data=False):
    """Compile the user's model into the batch kernel -> :class:`BatchFusedLibrary`.

    ``source``: HIP C++ that defines the functor type ``functor`` -- ``__device__ double operator()(const double* x, int ndim,
    int member, const void* user) const`` -- and whatever ``extern "C"`` helpers the user wants in the same library.  The
    translation unit is ``#include <emx_fused_target.hpp>``, ``source`` and ``EMX_FUSED_BATCH_TARGET(name, functor, ndim)``,
    compiled with ``hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -shared -fPIC`` (+ ``flags``) and
    :func:`get_include`.  The output is cached in ``cache_dir`` (default ``$EMCEE_AMD_CACHE`` or ``~/.cache/emcee_amd``) under
    the hash of source, functor, ndim, name, flags and every header of the library: a second call with the same inputs compiles
    nothing.  A compiler failure raises ``RuntimeError`` with the compiler's last lines.

    ``nblobs = K > 0``: the functor has the five-argument form ``(const double* x, int ndim, int member, const void* user, double*
    blobs)`` and writes ``blobs[0 ... K)``; the translation unit ends with ``EMX_FUSED_BATCH_TARGET_BLOBS(name, functor, ndim, K)``
    and K is part of the cache key.

    ``data=True``: ``functor`` is a model with ``base(x, ndim, member, user)`` and ``term(x, ndim, member, k, user)`` members whose
    log-probability sums over per-member data (:class:`BatchFused`'s ``ndata``).  The translation unit is ``#include
    <emx_fused_target_data.hpp>``, ``source`` and ``EMX_FUSED_BATCH_DATA_TARGET(name, functor, ndim)``; ``nblobs`` is refused.
    ``data=False`` keeps the translation unit and the cache key it always had."""
    ndim = _compile_ndim("compile_fused", ndim)
    nblobs = _compile_nblobs("compile_fused", nblobs, data)
    name, flags = _compile_names("compile_fused", "emx_fused", ndim, (("functor", functor),), name, flags)
    tail = ("EMX_FUSED_BATCH_TARGET_BLOBS(%s, %s, %d, %d)" % (name, functor, ndim, nblobs) if nblobs else
            "EMX_FUSED_BATCH_TARGET(%s, %s, %d)" % (name, functor, ndim))
    # (nblobs joins the key only when there are blobs: a blob-free build does not depend on how the count is spelt)
    key = ("batch", source, functor, ndim, name) + (("nblobs", nblobs) if nblobs else ())
    so = _compile_form("compile_fused", "emx_fused_target.hpp", source, tail, "EMX_FUSED_BATCH_DATA_TARGET(%s, %s, %d)" % (name, functor, ndim), key,
                       name, flags, cache_dir, data)
    return BatchFusedLibrary(so, name, ndim, nblobs, data=data)
