"""Fused user targets of the single sampler on the GPU: a DeviceFused run equals the DeviceKernel run of the same function BIT FOR
BIT -- chain, log-probs, accept counts, last state, the generator afterwards -- for every move that path runs, both rng modes,
thinning, unstored and continued runs; -inf and NaN behave as they do there; what the library refuses is refused by message.

tests/c/user_ensemble_fused.hip defines each model once and wraps it both ways.  DeviceKernel itself is pinned to the reference by
tests/test_gpu_device_callable.py, which makes it an oracle that is not the code under test.  No tolerance anywhere."""
import ctypes as C
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import emcee_amd
from emcee_amd import _lib, moves, targets
from emcee_amd.targets import get_include

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "user_ensemble_fused.hip")
K = 20
_LIBS = {}


def _user_lib(ndim):
    """the models compiled for `ndim`, cached under build/ by the hash of the source and of every header it includes"""
    if ndim in _LIBS:
        return _LIBS[ndim]
    from emcee_amd import _build
    h = hashlib.sha256(open(SRC, "rb").read() + str(ndim).encode())
    for d in _build.DEPS:
        if d.endswith((".hpp", ".h")):
            h.update(open(d, "rb").read())
    work = os.path.join(ROOT, "build", "test_user_ensemble")
    so = os.path.join(work, "libuser_%d_%s.so" % (ndim, h.hexdigest()[:16]))
    if not os.path.exists(so):
        os.makedirs(work, exist_ok=True)
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        tmp = "%s.%d.tmp" % (so, os.getpid())
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DUSER_NDIM=%d" % ndim] +
                       ["-I" + d for d in get_include()] + [SRC, "-o", tmp], check=True, timeout=900, capture_output=True)
        os.replace(tmp, so)
    _lib.load()                                      # one HIP runtime per process: the library's (torch's) first
    user = C.CDLL(so)
    user.user_setup.restype = C.c_void_p
    user.user_setup.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double]
    user.user_device_pointer.restype = C.c_void_p
    user.user_device_pointer.argtypes = [C.c_void_p]
    user.user_teardown.argtypes = [C.c_void_p]
    _LIBS[ndim] = user
    return user


class Model(object):
    """one model of the test library in both wrappings"""

    def __init__(self, ndim, which="a", box=2.5, nan_above=1e300, seed=11):
        self.user, self.ndim, self.which = _user_lib(ndim), ndim, which
        rs = np.random.RandomState(seed)
        self.mu = np.ascontiguousarray(0.3 * rs.randn(ndim))
        self.ivar = np.ascontiguousarray(1.0 / (0.5 + rs.rand(ndim)) ** 2)
        t = np.linspace(-1.0, 1.0, K)
        yerr = 0.1 + 0.1 * rs.rand(K)
        self.data = np.ascontiguousarray(np.stack([t, 0.2 + 0.5 * t + yerr * rs.randn(K), yerr]))
        self.h = self.user.user_setup(self.mu.ctypes.data, self.ivar.ctypes.data, self.data.ctypes.data, ndim, float(box), float(nan_above))
        assert self.h

    def kernel(self):
        return targets.DeviceKernel(getattr(self.user, "user_rows_" + self.which), self.h)

    def fused(self):
        return targets.DeviceFused(getattr(self.user, "user_fused_" + self.which), self.ndim, user=self.user.user_device_pointer(self.h))

    def close(self):
        self.user.user_teardown(self.h)


def _start(N, D, seed=5, scale=1.0):
    return scale * np.random.RandomState(seed).randn(N, D)


def _run(target, N, D, p0, mv, rng, calls=((6, {}),), seed=1234):
    """-> everything a run leaves behind: chain, log-probs, accept counts, last state, generator"""
    s = emcee_amd.EnsembleSampler(N, D, target, moves=mv, rng=rng)
    s._random.seed(seed)
    st = p0
    for nsteps, kw in calls:
        st = s.run_mcmc(st, nsteps, skip_initial_state_check=True, **kw)
    out = dict(coords=np.array(st.coords), lp=np.array(st.log_prob), accepted=np.array(s.backend.accepted), iteration=s.iteration)
    if s.iteration > 0:
        out["chain"] = s.get_chain()
        out["chain_lp"] = s.get_log_prob()
    rstate = s.random_state
    out["mt"] = (np.array(rstate[1]), rstate[2], rstate[3], rstate[4])
    out["philox_step"] = s._philox_step
    ens = s._ens
    out["launch_kind"] = ens._target_kind
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k == "launch_kind":
            continue
        if k == "mt":
            assert np.array_equal(a[k][0], b[k][0]) and a[k][1:] == b[k][1:], "generator state differs"
        else:
            assert np.array_equal(a[k], b[k], equal_nan=False) if not isinstance(a[k], int) else a[k] == b[k], "%s differs" % k
    assert a["launch_kind"] == _lib.TARGET_CALLBACK and b["launch_kind"] == _lib.TARGET_FUSED_ENSEMBLE


def _pair(m, N, D, mv_factory, rng, calls=((6, {}),), p0=None):
    p0 = _start(N, D) if p0 is None else p0
    ref = _run(m.kernel(), N, D, p0, mv_factory(), rng, calls)
    got = _run(m.fused(), N, D, p0, mv_factory(), rng, calls)
    _same(ref, got)
    return ref


LIVE = dict(live_dangerously=True)       # 64 walkers at ndim > 32: the comparison is of arithmetic, not of sampling quality
MOVES = {
    "stretch": lambda: moves.StretchMove(**LIVE),
    "stretch3": lambda: moves.StretchMove(nsplits=3, **LIVE),
    "de": lambda: moves.DEMove(**LIVE),
    "snooker": lambda: moves.DESnookerMove(**LIVE),
    "de+snooker": lambda: [(moves.DEMove(**LIVE), 0.6), (moves.DESnookerMove(**LIVE), 0.4)],
    "gauss_vector": lambda: moves.GaussianMove(0.05, mode="vector"),
    "gauss_sequential": lambda: moves.GaussianMove(0.3, mode="sequential"),
}
NDIMS = (1, 2, 5, 16, 33, 64, 130)


@pytest.mark.parametrize("ndim", NDIMS)
def test_every_walker_count_at_every_ndim(ndim):
    """64, 1 000 (an odd half) and 4 096 walkers, stretch move, Philox plans; the accept rate is a rate, not 0 or 1"""
    m = Model(ndim)
    try:
        for N in (64, 1000, 4096):
            ref = _pair(m, N, ndim, MOVES["stretch"], "philox")
            if N >= 1000:
                assert 0 < ref["accepted"].sum() < 6 * N
    finally:
        m.close()


def test_the_headline_shape():
    m = Model(64)
    try:
        ref = _pair(m, 65536, 64, MOVES["stretch"], "philox", calls=((4, {}),))
        assert 0 < ref["accepted"].sum() < 4 * 65536
    finally:
        m.close()


@pytest.mark.parametrize("rng", ["philox", "mt19937"])
@pytest.mark.parametrize("move", sorted(MOVES))
def test_every_move_in_both_rng_modes(move, rng):
    """each move at an odd ndim with 1 000 walkers (one coordinate a lane) and an even one with 4 096 (two a lane); ndim 130 with 64"""
    for N, ndim in ((1000, 5), (4096, 16), (64, 130)):
        m = Model(ndim)
        try:
            _pair(m, N, ndim, MOVES[move], rng)
        finally:
            m.close()


@pytest.mark.parametrize("rng", ["philox", "mt19937"])
def test_thinning_unstored_and_continued_runs(rng):
    N, ndim = 1000, 33
    m = Model(ndim)
    try:
        _pair(m, N, ndim, MOVES["stretch"], rng, calls=((4, dict(thin_by=3)),))
        _pair(m, N, ndim, MOVES["de"], rng, calls=((7, dict(store=False)),))
        # two consecutive calls, the second from the device State of the first, against one call of the same length
        two = _pair(m, N, ndim, MOVES["stretch"], rng, calls=((5, {}), (6, {})))
        one = _pair(m, N, ndim, MOVES["stretch"], rng, calls=((11, {}),))
        for k in ("chain", "chain_lp", "coords", "lp", "accepted"):
            assert np.array_equal(two[k], one[k]), k
    finally:
        m.close()


@pytest.mark.parametrize("move", ["walk", "kde"])
def test_walk_and_kde_moves_take_the_fused_evaluation(move):
    N, ndim = 1000, 5
    m = Model(ndim)
    try:
        _pair(m, N, ndim, (lambda: moves.WalkMove()) if move == "walk" else (lambda: moves.KDEMove()), "philox", calls=((4, {}),))
    finally:
        m.close()


@pytest.mark.parametrize("ndim", [2, 16])
def test_a_box_that_cuts_the_start_cloud(ndim):
    """model (b): -inf outside the box -- proposals that leave it are rejected, walkers that start outside accept anything finite"""
    N = 1000
    m = Model(ndim, which="b", box=1.0)
    try:
        p0 = _start(N, ndim, scale=0.8)
        assert 0 < (np.abs(p0) > 1.0).any(axis=1).sum() < N
        ref = _pair(m, N, ndim, MOVES["stretch"], "philox", p0=p0, calls=((8, {}),))
        assert np.isinf(ref["chain_lp"]).any() and np.isfinite(ref["chain_lp"]).any()
    finally:
        m.close()


def test_nan_raises_the_same_error():
    N, ndim = 1000, 5
    m = Model(ndim, which="n", nan_above=0.9)
    try:
        p0 = np.clip(_start(N, ndim, scale=0.4), -0.85, 0.85)      # the start is clean: only proposals reach the NaN region
        errs = []
        for t in (m.kernel(), m.fused()):
            with pytest.raises(ValueError) as e:
                _run(t, N, ndim, p0, MOVES["stretch"](), "philox", calls=((20, {}),))
            errs.append(str(e.value))
        assert errs[0] == errs[1] == "Probability function returned NaN"
    finally:
        m.close()


def test_a_non_finite_proposal_ends_as_it_does_there():
    """a walker at 1e308 stretches past the largest double: the proposal is rejected, the status bit raised, the reference's error"""
    N, ndim = 64, 2
    m = Model(ndim)
    try:
        p0 = _start(N, ndim)
        p0[::2] = np.where(p0[::2] >= 0.0, 1.5e308, -1.5e308)
        errs = []
        for t in (m.kernel(), m.fused()):
            with pytest.raises(ValueError) as e:
                _run(t, N, ndim, p0, MOVES["stretch"](), "philox", calls=((10, {}),))
            errs.append(str(e.value))
        assert errs[0] == errs[1] == "At least one parameter value was infinite or NaN"
    finally:
        m.close()


def test_refusals_on_the_device():
    from emcee_amd.device import DeviceEnsemble
    from emcee_amd._lib import EmxError
    m5, m6 = Model(5), Model(6)
    try:
        with pytest.raises(ValueError) as e:
            emcee_amd.EnsembleSampler(64, 5, m5.fused(), distributed=True)
        assert "distributed" in str(e.value)
        ens = DeviceEnsemble(64, 5)
        try:
            # a launcher compiled for another ndim: the probe answers, nothing is launched
            with pytest.raises(EmxError) as e:
                ens.set_target_fused(m6.user.user_fused_a, None)
            assert "another ndim" in str(e.value) and "ndim 5" in str(e.value)
            # a BatchFused launcher: another descriptor type, refused on its constant
            from emcee_amd.targets import compile_fused
            src = "struct Z { __device__ double operator()(const double*, int, int, const void*) const { return 0.0; } };"
            batch = compile_fused(src, "Z", 5, cache_dir=os.path.join(ROOT, "build", "test_user_ensemble", "cache"))
            with pytest.raises(EmxError) as e:
                ens.set_target_fused(batch.launcher, None)
            assert "another version of emx_fused_ensemble.hpp" in str(e.value)
            assert ens._target_kind == _lib.TARGET_HOST and ens.status() == 0
            # ... and the right one is taken; sharding such a context is refused
            ens.set_target_fused(m5.user.user_fused_a, m5.user.user_device_pointer(m5.h))
            with pytest.raises(EmxError) as e:
                ens._ck(ens.lib.emx_set_shard(ens.ctx, 0, 2))
            assert "one replica" in str(e.value)
        finally:
            ens.close()
    finally:
        m5.close()
        m6.close()
