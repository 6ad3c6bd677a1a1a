"""Blobs of a DeviceFused target on the GPU (EMX_FUSED_ENSEMBLE_TARGET_BLOBS, k_halfstep_user with NB > 0).

The oracle is the blob-free functor through the blob-free DeviceFused (tests/test_gpu_ensemble_fused.py pins that one to
DeviceKernel): the blob run samples the same chain BIT FOR BIT, and every blob is reproducible in NumPy from the stored row with one
rounding (tests/c/user_ensemble_fused_blobs.hip: the map g below), so blobs are compared exactly, at every stored step and walker.
Rejected proposals are exercised because every run's acceptance fraction is asserted to lie in (0.1, 0.9).  No tolerance anywhere.

Shapes: the smallest that reach every row layout and tile rule -- ndim 1 (half an ensemble of 70 is less than one tile), 5 x 3 blobs
(two tiles and a part), 64 x 32 (the top of the blob range at the widest 64-row tile), 65 (tile 32, odd) and 129 (tile 16)."""
import ctypes as C
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import emcee_amd
from emcee_amd import _lib, moves, targets
from emcee_amd._lib import EmxError
from emcee_amd.state import State
from emcee_amd.targets import get_include

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "user_ensemble_fused_blobs.hip")
SHAPES = [(1, 1, 70), (5, 3, 300), (64, 32, 300), (65, 4, 300), (129, 4, 520)]       # ndim, K, nwalkers
NO_BLOBS = "If you start sampling with a given log_prob, you also need to provide the current list of blobs at that position."
_LIBS = {}


def _user_lib(ndim, K):
    """the model compiled for (ndim, K), cached under build/ by the hash of the source and of every header it includes"""
    if (ndim, K) in _LIBS:
        return _LIBS[(ndim, K)]
    from emcee_amd import _build
    h = hashlib.sha256(open(SRC, "rb").read() + ("%d,%d" % (ndim, K)).encode())
    for d in _build.DEPS:
        if d.endswith((".hpp", ".h")):
            h.update(open(d, "rb").read())
    work = os.path.join(ROOT, "build", "test_user_ensemble_blobs")
    so = os.path.join(work, "libuser_%d_%d_%s.so" % (ndim, K, h.hexdigest()[:16]))
    if not os.path.exists(so):
        os.makedirs(work, exist_ok=True)
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        tmp = "%s.%d.tmp" % (so, os.getpid())
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DUSER_NDIM=%d" % ndim,
                        "-DUSER_NBLOBS=%d" % K] + ["-I" + d for d in get_include()] + [SRC, "-o", tmp], check=True, timeout=900, capture_output=True)
        os.replace(tmp, so)
    _lib.load()                                      # one HIP runtime per process: the library's (torch's) first
    user = C.CDLL(so)
    user.user_setup.restype = C.c_void_p
    user.user_setup.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double]
    user.user_device_pointer.restype = C.c_void_p
    user.user_device_pointer.argtypes = [C.c_void_p]
    user.user_teardown.argtypes = [C.c_void_p]
    _LIBS[(ndim, K)] = user
    return user


class Model(object):
    """the diagonal Gaussian of the test library: blob-free and with K blobs, open or cut by a box"""

    def __init__(self, ndim, K, box=None, seed=11):
        self.user, self.ndim, self.K, self.box = _user_lib(ndim, K), ndim, K, box
        rs = np.random.RandomState(seed)
        self.mu = np.ascontiguousarray(0.3 * rs.randn(ndim))
        self.ivar = np.ascontiguousarray(1.0 / (0.5 + rs.rand(ndim)) ** 2)
        self.h = self.user.user_setup(self.mu.ctypes.data, self.ivar.ctypes.data, ndim, float(box if box is not None else 0.0))
        assert self.h
        self.dev = self.user.user_device_pointer(self.h)

    def plain(self):
        return targets.DeviceFused(getattr(self.user, "user_plain_box" if self.box is not None else "user_plain"), self.ndim, user=self.dev)

    def blobs(self, nblobs=None):
        return targets.DeviceFused(getattr(self.user, "user_blobs_box" if self.box is not None else "user_blobs"), self.ndim, user=self.dev,
                                   nblobs=self.K if nblobs is None else nblobs)

    def start(self, N, seed=5, scale=1.0):
        """a draw from the target itself (scale 1): the acceptance rates are the stationary ones from the first step"""
        return self.mu + scale * np.random.RandomState(seed).randn(N, self.ndim) / np.sqrt(self.ivar)

    def g(self, x, lp):
        """the blobs of rows x (..., ndim) with log-probs lp (...), as the functor computes them: one rounding each"""
        D, K = self.ndim, self.K
        with np.errstate(over="ignore", invalid="ignore"):
            cols = [x[..., 0], x[..., D - 1] + x[..., 0], lp] + [x[..., k % D] * float(k + 1) for k in range(3, K)]
        b = np.stack(cols[:K], axis=-1)
        return b[..., 0] if K == 1 else b

    def close(self):
        self.user.user_teardown(self.h)


def _moves(ndim):
    """every move the fused half-step runs, scaled so that a stationary ensemble accepts between a tenth and nine tenths"""
    a = 1.0 + 2.0 / np.sqrt(ndim) if ndim > 5 else 2.0
    snook = 1.7 if ndim <= 5 else 4.0 / np.sqrt(ndim)
    return {
        "stretch": lambda: moves.StretchMove(a=a),
        "stretch3": lambda: moves.StretchMove(a=a, nsplits=3),
        "de": lambda: moves.DEMove(),
        "snooker": lambda: moves.DESnookerMove(gammas=snook),
        "stretch+de": lambda: [(moves.StretchMove(a=a), 0.6), (moves.DEMove(), 0.4)],
        "gauss": lambda: moves.GaussianMove(0.5 / ndim, mode="vector"),
    }


def _run(target, N, D, p0, mv, rng, calls=((30, {}),), seed=1234):
    s = emcee_amd.EnsembleSampler(N, D, target, moves=mv, rng=rng)
    s._random.seed(seed)
    st = p0
    for nsteps, kw in calls:
        st = s.run_mcmc(st, nsteps, skip_initial_state_check=True, **kw)
    assert s._ens._target_kind == _lib.TARGET_FUSED_ENSEMBLE
    rstate = s.random_state
    out = dict(coords=np.array(st.coords), lp=np.array(st.log_prob), accepted=np.array(s.backend.accepted), iteration=s.iteration,
               chain=s.get_chain(), chain_lp=s.get_log_prob(), mt_key=np.array(rstate[1]), mt_rest=tuple(rstate[2:]), philox_step=s._philox_step)
    return s, st, out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        same = a[k] == b[k] if isinstance(a[k], (int, tuple)) else np.array_equal(a[k], b[k])
        assert same, "%s differs" % k


@pytest.fixture(scope="module")
def models():
    made = {}

    def get(ndim, K, box=None):
        key = (ndim, K, box)
        if key not in made:
            made[key] = Model(ndim, K, box)
        return made[key]
    yield get
    for m in made.values():
        m.close()


# ------------------------------------------------------------------------------------------ 1, 2: the same samples; blobs follow
@pytest.mark.parametrize("rng", ["philox", "mt19937"])
@pytest.mark.parametrize("ndim,K,N", SHAPES)
def test_sampling_is_unchanged_and_blobs_follow_the_walker(models, ndim, K, N, rng):
    m = models(ndim, K)
    p0 = m.start(N)
    for name, mv in sorted(_moves(ndim).items()):
        for thin_by in (1, 3):
            calls = ((30 // thin_by, dict(thin_by=thin_by)),)
            _, _, ref = _run(m.plain(), N, ndim, p0, mv(), rng, calls)
            s, st, got = _run(m.blobs(), N, ndim, p0, mv(), rng, calls)
            frac = ref["accepted"].sum() / float(N * ref["iteration"])
            print("ndim %d K %d N %d %s %s thin_by %d: acceptance fraction %.3f" % (ndim, K, N, rng, name, thin_by, frac))
            _same(ref, got)
            assert 0.1 < frac < 0.9, "both branches of the blob commit must run: %s accepts %.3f" % (name, frac)
            blobs = s.get_blobs()
            assert blobs.shape == ((30 // thin_by, N) if K == 1 else (30 // thin_by, N, K))
            assert np.array_equal(blobs, m.g(got["chain"], got["chain_lp"])), name
            if K >= 3:
                assert np.array_equal(blobs[..., 2], s.get_log_prob())
            assert np.array_equal(st.blobs, m.g(got["coords"], got["lp"]))
            assert np.array_equal(s.get_last_sample().blobs, blobs[-1])


# ------------------------------------------------------------------------------------------ 3: rows that keep their previous blobs
@pytest.mark.parametrize("ndim,K,N", [(5, 3, 300), (64, 32, 300)])
def test_a_box_that_cuts_the_start_cloud(models, ndim, K, N):
    """-inf outside the box: walkers that start outside carry lp = -inf and its blobs until they accept, proposals that leave the box
    are rejected and the row keeps its previous blobs"""
    m = models(ndim, K, box=1.2 if ndim == 5 else 3.2)
    p0 = m.start(N)
    outside = (np.abs(p0) > m.box).any(axis=1).sum()
    assert 0 < outside < N
    mv = _moves(ndim)["stretch"]
    _, _, ref = _run(m.plain(), N, ndim, p0, mv(), "philox")
    s, st, got = _run(m.blobs(), N, ndim, p0, mv(), "philox")
    _same(ref, got)
    frac = ref["accepted"].sum() / float(N * ref["iteration"])
    print("box, ndim %d: %d walkers start outside, acceptance fraction %.3f" % (ndim, outside, frac))
    assert 0.1 < frac < 0.9
    assert np.isinf(got["chain_lp"]).any() and np.isfinite(got["chain_lp"]).any()
    assert np.array_equal(s.get_blobs(), m.g(got["chain"], got["chain_lp"]))
    assert np.array_equal(st.blobs, m.g(got["coords"], got["lp"]))


def test_a_non_finite_proposal_ends_as_it_does_today(models):
    """walkers at 1.5e308 stretch past the largest double: rejected without the call, the same error, and the rows stored before the
    error left still carry the blobs of their coordinates"""
    ndim, K, N = 5, 3, 300
    m = models(ndim, K)
    p0 = m.start(N)
    p0[::2] = np.where(p0[::2] >= 0.0, 1.5e308, -1.5e308)
    runs = []
    for t in (m.plain(), m.blobs()):
        s = emcee_amd.EnsembleSampler(N, ndim, t, moves=moves.StretchMove(), rng="philox")
        s._random.seed(1234)
        with pytest.raises(ValueError) as e:
            s.run_mcmc(p0, 10, skip_initial_state_check=True)
        assert str(e.value) == "At least one parameter value was infinite or NaN"
        runs.append(s)
    plain, blob = runs
    assert plain.iteration == blob.iteration > 0
    chain, lp = blob.get_chain(), blob.get_log_prob()
    assert np.array_equal(chain, plain.get_chain()) and np.array_equal(lp, plain.get_log_prob())
    assert np.array_equal(blob.get_blobs(), m.g(chain, lp))


# ------------------------------------------------------------------------------------------ 4: state plumbing
def test_state_plumbing(models):
    ndim, K, N, n = 5, 3, 300, 20
    m = models(ndim, K)
    p0 = m.start(N)
    mv = _moves(ndim)["stretch"]
    # the initial blobs are evaluated on the device; compute_log_prob returns them
    s = emcee_amd.EnsembleSampler(N, ndim, m.blobs(), moves=mv(), rng="philox")
    s._random.seed(99)
    lp0, b0 = s.compute_log_prob(p0)
    assert np.array_equal(b0, m.g(p0, lp0)) and np.isfinite(lp0).all()
    st1 = s.run_mcmc(p0, n, skip_initial_state_check=True)
    assert s.backend.has_blobs() and np.array_equal(s.backend.blobs, s.get_blobs())
    first = s.get_blobs()
    # one run of 2n against two of n: continued with None, with the returned state, and with the last sample brought to the host
    one = emcee_amd.EnsembleSampler(N, ndim, m.blobs(), moves=mv(), rng="philox")
    one._random.seed(99)
    one.run_mcmc(p0, 2 * n, skip_initial_state_check=True)
    for how in ("none", "state", "host"):
        two = emcee_amd.EnsembleSampler(N, ndim, m.blobs(), moves=mv(), rng="philox")
        two._random.seed(99)
        st = two.run_mcmc(p0, n, skip_initial_state_check=True)
        if how == "host":
            st = two.get_last_sample()
            assert type(st) is State and np.array_equal(st.blobs, m.g(st.coords, st.log_prob))
        end = two.run_mcmc(None if how == "none" else st, n, skip_initial_state_check=True)
        for name in ("get_chain", "get_log_prob", "get_blobs"):
            assert np.array_equal(getattr(two, name)(), getattr(one, name)()), (how, name)
        assert np.array_equal(end.blobs, one.get_blobs()[-1]) and np.array_equal(two.backend.accepted, one.backend.accepted)
    # a state held across a later run keeps its blobs (the snapshot carries them); the grown chain keeps its earlier rows
    st2 = s.run_mcmc(None, n, skip_initial_state_check=True)
    assert np.array_equal(s.get_blobs()[:n], first) and np.array_equal(s.get_blobs(), one.get_blobs())
    assert np.array_equal(st1.blobs, first[-1]) and np.array_equal(st1.blobs, m.g(st1.coords, st1.log_prob))
    assert np.array_equal(st2.blobs, s.get_blobs()[-1])
    # a given log_prob without blobs: the reference's message, on both paths
    with pytest.raises(ValueError) as e:
        s.run_mcmc(State(p0, log_prob=lp0), 2, skip_initial_state_check=True)
    assert str(e.value) == NO_BLOBS
    with pytest.raises(ValueError) as e:
        next(s.sample(State(p0, log_prob=lp0), iterations=1, skip_initial_state_check=True))
    assert str(e.value) == NO_BLOBS
    # the generator path yields the same blobs as the one-call path
    gen = emcee_amd.EnsembleSampler(N, ndim, m.blobs(), moves=mv(), rng="philox")
    gen._random.seed(99)
    for i, st in enumerate(gen.sample(p0, iterations=3, skip_initial_state_check=True)):
        assert np.array_equal(st.blobs, one.get_blobs()[i])
    assert np.array_equal(gen.get_blobs(), one.get_blobs()[:3])
    # reset empties them
    s.reset()
    assert s.iteration == 0
    with pytest.raises(AttributeError):
        s.get_blobs()
    s.run_mcmc(p0, 3, skip_initial_state_check=True)
    assert s.get_blobs().shape == (3, N, K)


# ------------------------------------------------------------------------------------------ 5: shapes
@pytest.mark.parametrize("ndim,K,N", [(1, 1, 70), (5, 3, 300)])
def test_shapes_and_slices(models, ndim, K, N):
    m = models(ndim, K)
    s, st, _ = _run(m.blobs(), N, ndim, m.start(N), _moves(ndim)["stretch"](), "philox", calls=((30, {}),))
    tail = () if K == 1 else (K,)
    full = s.get_blobs()
    assert full.shape == (30, N) + tail and full.dtype == np.float64
    assert st.blobs.shape == (N,) + tail and s.get_last_sample().blobs.shape == (N,) + tail
    assert s.compute_log_prob(m.start(7, seed=3))[1].shape == (7,) + tail
    for discard, thin in ((0, 1), (7, 1), (0, 4), (5, 3), (29, 1)):
        want = full[discard + thin - 1::thin]
        assert np.array_equal(s.get_blobs(discard=discard, thin=thin), want)
        assert np.array_equal(s.get_blobs(discard=discard, thin=thin, flat=True), want.reshape((-1,) + tail))
    assert np.array_equal(s.backend.get_blobs(), full) and s.backend.has_blobs()


# ------------------------------------------------------------------------------------------ 6: refusals
def test_refusals_launch_nothing(models):
    from emcee_amd.device import DeviceEnsemble
    ndim, K, N = 5, 3, 300
    m = models(ndim, K)
    ens = DeviceEnsemble(N, ndim)
    try:
        for wrong in (2, 4):                          # a launcher of another blob count: the probe answers at bind time
            with pytest.raises(EmxError) as e:
                m.blobs(nblobs=wrong).bind(ens)
            assert "another number of blobs" in str(e.value)
        with pytest.raises(EmxError) as e:            # the blob launcher as a blob-free target, and the other way round
            ens.set_target_fused(m.user.user_blobs, m.dev)
        assert "another version of emx_fused_ensemble.hpp" in str(e.value)
        with pytest.raises(EmxError) as e:
            ens.set_target_fused(m.user.user_plain, m.dev, nblobs=K)
        assert "another version of emx_fused_ensemble.hpp" in str(e.value)
        assert ens._target_kind == _lib.TARGET_HOST and ens.nblobs() == 0 and ens.status() == 0
    finally:
        ens.close()
    for name, mv in (("WalkMove", moves.WalkMove()), ("KDEMove", moves.KDEMove())):
        s = emcee_amd.EnsembleSampler(N, ndim, m.blobs(), moves=mv, rng="philox")
        with pytest.raises(EmxError) as e:
            s.run_mcmc(m.start(N), 2, skip_initial_state_check=True)
        assert name in str(e.value) and "blobs" in str(e.value)
        assert s._ens.iteration() == (0, 0) and s._ens.status() == 0
