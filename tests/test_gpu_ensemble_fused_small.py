"""Small ensembles of a DeviceFused target on the GPU: with a one-workgroup launcher bound (DeviceFused's small_fn), an ensemble that
fits one workgroup's LDS runs run_mcmc inside k_small_run -- and every such run equals, FIELD FOR FIELD AND BIT FOR BIT,
  1. the same DeviceFused with the tuning key small_kernel = 0 (the launch per half-step it ran before), and
  2. the DeviceKernel run of the same function (pinned to the reference by tests/test_gpu_device_callable.py):
chain, log-probs, accept counts, last state, the MT19937 generator afterwards, the Philox step, blobs.  DeviceEnsemble.small_info()
says which kernel ran, independently of any timing.  No tolerance anywhere.

tests/c/user_ensemble_fused_small.hip defines each model once and wraps it three ways.  Shapes are the smallest at which the kernel
takes another path: 32 x 5 (the quickstart shape), splits of two rows, uneven splits, one coordinate a lane in four chunks, ndim 130,
the LDS boundary and its neighbour, more than one plan pass, more than one launch."""
import ctypes as C
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import emcee_amd
from emcee_amd import _lib, moves, targets
from emcee_amd.state import State
from emcee_amd.targets import get_include

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "user_ensemble_fused_small.hip")
# (ndim, models b and n too, blobs): every library the tests below load, compiled side by side by the first that needs one
BUILDS = [(1, False, 0), (2, False, 0), (5, True, 0), (16, False, 0), (33, False, 0), (130, False, 0), (5, False, 1), (5, False, 3)]
_LIBS = {}


def _paths():
    from emcee_amd import _build
    out = {}
    for ndim, extra, K in BUILDS:
        h = hashlib.sha256(open(SRC, "rb").read() + ("%d,%d,%d" % (ndim, extra, K)).encode())
        for d in _build.DEPS:
            if d.endswith((".hpp", ".h")):
                h.update(open(d, "rb").read())
        out[(ndim, extra, K)] = os.path.join(ROOT, "build", "test_user_ensemble_small", "libuser_%d_%d_%d_%s.so" % (ndim, extra, K, h.hexdigest()[:16]))
    return out


def _user_lib(ndim, K=0):
    """the models compiled for `ndim` (with K blobs), cached under build/ by the hash of the source and of every header it includes"""
    key = [b for b in BUILDS if b[0] == ndim and b[2] == K][0]
    if key in _LIBS:
        return _LIBS[key]
    paths = _paths()
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    running = []
    for (nd, ex, k), so in paths.items():           # whatever is missing, at once: eight compilers beside each other
        if os.path.exists(so):
            continue
        os.makedirs(os.path.dirname(so), exist_ok=True)
        tmp = "%s.%d.tmp" % (so, os.getpid())
        flags = ["-DUSER_NDIM=%d" % nd] + (["-DUSER_EXTRA"] if ex else []) + (["-DUSER_NBLOBS=%d" % k] if k else [])
        p = subprocess.Popen([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC"] + flags +
                             ["-I" + d for d in get_include()] + [SRC, "-o", tmp], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        running.append((p, tmp, so))
    for p, tmp, so in running:
        log = p.communicate(timeout=900)[0]
        assert p.returncode == 0, log.decode()[-4000:]
        os.replace(tmp, so)
    _lib.load()                                      # one HIP runtime per process: the library's (torch's) first
    user = C.CDLL(paths[key])
    user.user_setup.restype = C.c_void_p
    user.user_setup.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double]
    user.user_device_pointer.restype = C.c_void_p
    user.user_device_pointer.argtypes = [C.c_void_p]
    user.user_teardown.argtypes = [C.c_void_p]
    _LIBS[key] = user
    return user


class Model(object):
    """one model of the test library in its three wrappings"""

    def __init__(self, ndim, which="a", box=2.5, nan_above=1e300, K=0, seed=11):
        self.user, self.ndim, self.which, self.K = _user_lib(ndim, K), ndim, which, K
        rs = np.random.RandomState(seed)
        self.mu = np.ascontiguousarray(0.3 * rs.randn(ndim))
        self.ivar = np.ascontiguousarray(1.0 / (0.5 + rs.rand(ndim)) ** 2)
        self.h = self.user.user_setup(self.mu.ctypes.data, self.ivar.ctypes.data, ndim, float(box), float(nan_above))
        assert self.h
        self.dev = self.user.user_device_pointer(self.h)

    def kernel(self):
        return targets.DeviceKernel(getattr(self.user, "user_rows_" + self.which), self.h)

    def fused(self, small=True):
        return targets.DeviceFused(getattr(self.user, "user_fused_" + self.which), self.ndim, user=self.dev,
                                   small_fn=getattr(self.user, "user_small_" + self.which) if small else None)

    def blobs(self, small=True):
        return targets.DeviceFused(self.user.user_fused_blobs, self.ndim, user=self.dev, nblobs=self.K,
                                   small_fn=self.user.user_small_blobs if small else None)

    def g(self, x, lp):
        """the blobs of rows x (..., ndim) with log-probs lp (...), as the functor computes them: one rounding each"""
        D, K = self.ndim, self.K
        cols = [x[..., 0], x[..., D - 1] + x[..., 0], lp] + [x[..., k % D] * float(k + 1) for k in range(3, K)]
        b = np.stack(cols[:K], axis=-1)
        return b[..., 0] if K == 1 else b

    def close(self):
        self.user.user_teardown(self.h)


@pytest.fixture(scope="module")
def models():
    made = {}

    def get(ndim, **kw):
        key = (ndim,) + tuple(sorted(kw.items()))
        if key not in made:
            made[key] = Model(ndim, **kw)
        return made[key]
    yield get
    for m in made.values():
        m.close()


def _start(N, D, seed=5, scale=1.0):
    return scale * np.random.RandomState(seed).randn(N, D)


def _run(target, N, D, p0, mv, rng, calls=((6, {}),), seed=1234, small_kernel=1, keep=None):
    """-> everything a run leaves behind: chain, log-probs, accept counts, last state, generator, blobs, the one-workgroup launches.
    calls: (nsteps, run_mcmc keywords[, "none": continue with run_mcmc(None, ...)]) one after the other, each from the state the
    previous one returned"""
    s = emcee_amd.EnsembleSampler(N, D, target, moves=mv, rng=rng)
    s._random.seed(seed)
    s._device_ensemble().set_tuning("small_kernel", small_kernel)
    if keep is not None:
        keep.append(s)
    st = p0
    for call in calls:
        st = s.run_mcmc(None if len(call) > 2 and call[2] == "none" else st, call[0], skip_initial_state_check=True, **call[1])
        assert type(st) is State or hasattr(st, "coords")
    out = dict(coords=np.array(st.coords), lp=np.array(st.log_prob), accepted=np.array(s.backend.accepted), iteration=s.iteration)
    if s.iteration > 0:
        out["chain"] = s.get_chain()
        out["chain_lp"] = s.get_log_prob()
    rstate = s.random_state
    out["mt"] = (np.array(rstate[1]), rstate[2], rstate[3], rstate[4])
    out["philox_step"] = s._philox_step
    if getattr(target, "nblobs", 0):
        out["state_blobs"] = np.array(st.blobs)
        if s.iteration > 0:
            out["last_blobs"] = np.array(s.get_last_sample().blobs)
            out["blobs"] = s.get_blobs()
    info = s._ens.small_info()
    out["small"] = (info["launches"], info["steps"])
    return out


def _same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        if k == "small":
            continue
        if k == "mt":
            assert np.array_equal(a[k][0], b[k][0]) and a[k][1:] == b[k][1:], "generator state differs " + what
        else:
            assert np.array_equal(a[k], b[k], equal_nan=False) if not isinstance(a[k], int) else a[k] == b[k], "%s differs %s" % (k, what)


def _triple(m, N, D, mv_factory, rng, calls=((6, {}),), p0=None, expect_small=True, blobs=False, small_kernel=2):
    """the small run against its two references; -> the small run.  small_kernel 2: the one-workgroup kernel wherever the ensemble
    fits (the shapes below are chosen where the kernel can go wrong, not where it is fast); 1: the default, where it also pays"""
    p0 = _start(N, D) if p0 is None else p0
    target = m.blobs if blobs else m.fused
    got = _run(target(), N, D, p0, mv_factory(), rng, calls, small_kernel=small_kernel)
    general = _run(target(), N, D, p0, mv_factory(), rng, calls, small_kernel=0)
    nsteps = sum(c[0] * c[1].get("thin_by", 1) for c in calls)
    assert general["small"] == (0, 0), "small_kernel = 0 forces the launch per half-step"
    if expect_small:
        assert got["small"][0] > 0 and got["small"][1] == nsteps, "the one-workgroup kernel ran every step: %r" % (got["small"],)
    else:
        assert got["small"] == (0, 0), "this configuration stays on the launch per half-step"
    _same(general, got, "(small kernel off / on)")
    if not blobs:                                     # a DeviceKernel carries no blobs: the blob tests have an oracle of their own
        _same(_run(m.kernel(), N, D, p0, mv_factory(), rng, calls), got, "(DeviceKernel / small kernel)")
    return got


LIVE = dict(live_dangerously=True)       # fewer walkers than 2 ndim: the comparison is of arithmetic, not of sampling quality
MOVES = {
    "stretch": lambda: moves.StretchMove(**LIVE),
    "stretch3": lambda: moves.StretchMove(nsplits=3, **LIVE),
    "de": lambda: moves.DEMove(**LIVE),
    "snooker": lambda: moves.DESnookerMove(**LIVE),
    "de+snooker": lambda: [(moves.DEMove(**LIVE), 0.6), (moves.DESnookerMove(**LIVE), 0.4)],
    "gauss_vector": lambda: moves.GaussianMove(0.05, mode="vector"),
    "gauss_sequential": lambda: moves.GaussianMove(0.3, mode="sequential"),
}
RNGS = ["philox", "mt19937"]


@pytest.mark.parametrize("rng", RNGS)
@pytest.mark.parametrize("move", sorted(MOVES))
def test_the_quickstart_shape_every_move_in_both_rng_modes(models, move, rng):
    """32 x 5.  A GaussianMove under MT19937 takes N x ndim host normals a step: the launch per half-step, the same bits"""
    got = _triple(models(5), 32, 5, MOVES[move], rng, calls=((12, {}),), expect_small=not (move.startswith("gauss") and rng == "mt19937"),
                  small_kernel=1)
    assert 0 < got["accepted"].sum() < 12 * 32


@pytest.mark.parametrize("rng", RNGS)
@pytest.mark.parametrize("N,ndim,move", [(4, 1, lambda: moves.StretchMove(nsplits=2, **LIVE)),          # splits of two rows
                                         (33, 2, lambda: moves.StretchMove(nsplits=3, **LIVE)),         # uneven splits, stage_rows = 11
                                         (33, 2, lambda: moves.DEMove(nsplits=3, **LIVE)),
                                         (64, 33, lambda: moves.StretchMove(**LIVE)),                   # one coordinate a lane, four chunks
                                         (64, 130, lambda: moves.StretchMove(**LIVE))])
def test_shapes_where_the_kernel_takes_another_path(models, N, ndim, move, rng):
    _triple(models(ndim), N, ndim, move, rng, calls=((8, {}),))


def _largest_admitted(ndim, nblobs):
    arr = (_lib.MoveDesc * 1)(_lib.MoveDesc(kind=0, nsplits=2))
    lib = _lib.load()
    fits = [N for N in range(4, 4097) if lib.emx_small_fused_check(N, ndim, 1, arr, _lib.RNG_PHILOX, nblobs, None, 0) == 0]
    return max(fits)


@pytest.mark.parametrize("nblobs", [0, 3])
def test_the_lds_boundary(models, nblobs):
    """the largest nwalkers emx_small_fused_check admits at ndim 5 takes the one-workgroup kernel, its neighbour does not"""
    m = models(5, K=nblobs) if nblobs else models(5)
    N = _largest_admitted(5, nblobs)
    assert 1000 < N < 2000 and _largest_admitted(5, 0) > _largest_admitted(5, 3)
    for rng in RNGS:
        _triple(m, N, 5, MOVES["stretch"], rng, blobs=bool(nblobs))
        _triple(m, N + 1, 5, MOVES["stretch"], rng, expect_small=False, blobs=bool(nblobs))


@pytest.mark.parametrize("rng", RNGS)
def test_more_than_one_plan_pass_and_more_than_one_launch(models, rng):
    m = models(5)
    _triple(m, 32, 5, MOVES["stretch"], rng, calls=((70, {}),))                      # small_batch(32) = 32 steps a pass
    got = _triple(m, 32, 5, MOVES["de+snooker"], rng, calls=((4100, dict(store=False)),))     # a launch takes 4 096 steps at most
    assert got["small"][0] >= 2


@pytest.mark.parametrize("rng", RNGS)
def test_thinning_unstored_and_continued_runs(models, rng):
    m = models(5)
    N, ndim = 32, 5
    _triple(m, N, ndim, MOVES["stretch"], rng, calls=((5, dict(thin_by=3)),))
    _triple(m, N, ndim, MOVES["de"], rng, calls=((9, dict(store=False)),))
    # two consecutive calls -- the second from the State the first returned, or from None -- against one call of the same length
    one = _triple(m, N, ndim, MOVES["stretch"], rng, calls=((11, {}),))
    for how in ("state", "none"):
        two = _triple(m, N, ndim, MOVES["stretch"], rng, calls=((5, {}), (6, {}, how)))
        for k in ("chain", "chain_lp", "coords", "lp", "accepted", "philox_step"):
            assert np.array_equal(two[k], one[k]), (how, k)
        assert np.array_equal(two["mt"][0], one["mt"][0])


@pytest.mark.parametrize("rng", RNGS)
@pytest.mark.parametrize("K", [1, 3])
def test_blobs_follow_the_walker(models, K, rng):
    """get_blobs, get_last_sample().blobs and the state's blobs equal the launch per half-step's; the samples equal the blob-free
    functor's; and every blob is the functor's map of its stored row"""
    N, ndim = 32, 5
    m = models(ndim, K=K)
    p0 = m.mu + _start(N, ndim) / np.sqrt(m.ivar)
    for name in ("stretch", "de+snooker", "stretch3"):
        for calls in (((20, {}),), ((6, dict(thin_by=3)),), ((5, {}), (5, {}, "none"))):
            got = _triple(m, N, ndim, MOVES[name], rng, calls=calls, p0=p0, blobs=True)
            plain = _triple(m, N, ndim, MOVES[name], rng, calls=calls, p0=p0)
            for k in plain:
                if k not in ("small",):
                    assert np.array_equal(plain[k], got[k]) if k != "mt" else np.array_equal(plain[k][0], got[k][0]), k
            frac = got["accepted"].sum() / float(N * got["iteration"])
            assert 0.05 < frac < 0.95, "both branches of the blob commit must run: %s accepts %.3f" % (name, frac)
            assert got["blobs"].shape == got["chain_lp"].shape + (() if K == 1 else (K,))
            assert np.array_equal(got["blobs"], m.g(got["chain"], got["chain_lp"]))
            assert np.array_equal(got["state_blobs"], m.g(got["coords"], got["lp"]))
            assert np.array_equal(got["last_blobs"], got["blobs"][-1])
    _triple(m, N, ndim, MOVES["stretch"], rng, calls=((9, dict(store=False)),), p0=p0, blobs=True)


def test_a_box_that_cuts_the_start_cloud(models):
    """model (b): -inf outside the box -- proposals that leave it are rejected, walkers that start outside accept anything finite"""
    N, ndim = 32, 5
    m = models(ndim, which="b", box=1.0)
    p0 = _start(N, ndim, scale=0.8)
    assert 0 < (np.abs(p0) > 1.0).any(axis=1).sum() < N
    for rng in RNGS:
        got = _triple(m, N, ndim, MOVES["stretch"], rng, p0=p0, calls=((10, {}),))
        assert np.isinf(got["chain_lp"]).any() and np.isfinite(got["chain_lp"]).any()


def _errors(m, N, ndim, p0, nsteps):
    """-> the message each of the three runs ends with, and the one-workgroup launches of the third"""
    errs, keep = [], []
    for t, small in ((m.kernel(), 1), (m.fused(), 0), (m.fused(), 1)):
        with pytest.raises(ValueError) as e:
            _run(t, N, ndim, p0, MOVES["stretch"](), "philox", calls=((nsteps, {}),), small_kernel=small, keep=keep)
        errs.append(str(e.value))
    assert keep[1]._ens.small_info()["launches"] == 0 and keep[2]._ens.small_info()["launches"] > 0
    return errs


def test_nan_raises_the_same_error(models):
    N, ndim = 32, 5
    m = models(ndim, which="n", nan_above=0.3)
    p0 = np.clip(_start(N, ndim, scale=0.4), -0.85, 0.25)      # the start is clean: only proposals reach the NaN region
    errs = _errors(m, N, ndim, p0, 40)
    assert errs[0] == errs[1] == errs[2] == "Probability function returned NaN"


def test_a_non_finite_proposal_ends_as_it_does_there(models):
    """a walker at 1.5e308 stretches past the largest double: the proposal is rejected, the status bit raised, the reference's error"""
    N, ndim = 32, 5
    m = models(ndim, which="b")
    p0 = _start(N, ndim)
    p0[::2] = np.where(p0[::2] >= 0.0, 1.5e308, -1.5e308)
    errs = _errors(m, N, ndim, p0, 10)
    assert errs[0] == errs[1] == errs[2] == "At least one parameter value was infinite or NaN"


def test_what_does_not_fit_and_what_did_not_opt_in_run_as_before(models):
    _triple(models(16), 4096, 16, MOVES["stretch"], "philox", expect_small=False)
    m = models(5)
    p0 = _start(32, 5)
    for rng in RNGS:
        ref = _run(m.kernel(), 32, 5, p0, MOVES["stretch"](), rng)
        got = _run(m.fused(small=False), 32, 5, p0, MOVES["stretch"](), rng)      # no small_fn: no one-workgroup launch
        assert got["small"] == (0, 0)
        _same(ref, got)


def test_by_default_the_kernel_runs_where_it_pays(models):
    """emx_small_fused_pays (profiles/ensemble_fused_small.md): Philox plans up to ndim 10 and nwalkers x ndim 1 024, the host's plans up
    to ndim 16; elsewhere the default keeps the launch per half-step and small_kernel = 2 still reaches the kernel"""
    pays = _lib.load().emx_small_fused_pays
    ph, mt = _lib.RNG_PHILOX, _lib.RNG_MT19937
    assert [pays(32, 5, ph), pays(100, 10, ph), pays(512, 2, ph), pays(103, 10, ph), pays(64, 16, ph), pays(1000, 5, ph)] == [1, 1, 1, 0, 0, 0]
    assert [pays(32, 5, mt), pays(606, 16, mt), pays(1000, 5, mt), pays(64, 33, mt)] == [1, 1, 1, 0]
    for rng in RNGS:
        _triple(models(33), 64, 33, MOVES["stretch"], rng, expect_small=False, small_kernel=1)
    _triple(models(16), 256, 16, MOVES["stretch"], "mt19937", small_kernel=1)
    _triple(models(16), 256, 16, MOVES["stretch"], "philox", expect_small=False, small_kernel=1)


def test_sample_driven_step_by_step_stays_on_the_launch_per_half_step(models):
    m = models(5)
    p0 = _start(32, 5)
    one = _run(m.fused(), 32, 5, p0, MOVES["stretch"](), "mt19937", calls=((5, {}),))
    s = emcee_amd.EnsembleSampler(32, 5, m.fused(), moves=MOVES["stretch"](), rng="mt19937")
    s._random.seed(1234)
    for _ in s.sample(p0, iterations=5, skip_initial_state_check=True):
        pass
    assert s._ens.small_info()["launches"] == 0 and one["small"][0] > 0
    assert np.array_equal(s.get_chain(), one["chain"]) and np.array_equal(s.get_log_prob(), one["chain_lp"])


def test_refusals_at_bind_time(models):
    from emcee_amd._lib import EmxError
    from emcee_amd.device import DeviceEnsemble
    m5, m2, mb = models(5), models(2), models(5, K=3)
    ens = DeviceEnsemble(32, 5)
    try:
        with pytest.raises(EmxError) as e:            # before any fused target is bound
            ens._ck(ens.lib.emx_set_target_fused_small(ens.ctx, C.cast(m5.user.user_small_a, _lib.FUSED_BATCH_FN)))
        assert "emx_set_target_fused" in str(e.value)
        with pytest.raises(EmxError) as e:            # a small launcher compiled for another ndim
            ens.set_target_fused(m5.user.user_fused_a, m5.dev, small_fn=m2.user.user_small_a)
        assert "another ndim" in str(e.value) and "ndim 5" in str(e.value)
        with pytest.raises(EmxError) as e:            # ... for another blob count
            ens.set_target_fused(m5.user.user_fused_a, m5.dev, small_fn=mb.user.user_small_blobs)
        assert "another number of blobs" in str(e.value)
        with pytest.raises(EmxError) as e:            # the half-step launcher in the small launcher's place: another descriptor type
            ens.set_target_fused(m5.user.user_fused_a, m5.dev, small_fn=m5.user.user_fused_a)
        assert "another version of emx_fused_ensemble.hpp" in str(e.value)
        assert ens.status() == 0 and ens.small_info() == {"launches": 0, "steps": 0}
        ens.set_target_fused(m5.user.user_fused_a, m5.dev, small_fn=m5.user.user_small_a)
    finally:
        ens.close()
