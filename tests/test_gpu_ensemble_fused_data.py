"""Fused user targets that sum over data (targets.DeviceFused(..., ndata=); emx_fused_ensemble_data.hpp) on the GPU: the run equals
the DeviceKernel run of a kernel that sums in the defined order BIT FOR BIT -- chain, log-probs, accept counts, last state, generator
state and Philox step -- for every count of data around the lane stride, every row layout, every move, both rng modes, thinned,
unstored and continued runs, and whatever rows a workgroup takes.  The value itself is pinned by NumPy (targets.fused_data_sum).

tests/c/user_ensemble_fused_data.hip defines each model's base and term once and wraps them both ways.  DeviceKernel is pinned to the
reference by tests/test_gpu_device_callable.py and runs none of the new kernel, which makes it the oracle.  No tolerance anywhere.
Every compared run has an acceptance fraction strictly between 0.05 and 0.95 (checked on the oracle run), so equality is not vacuous."""
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
SRC = os.path.join(ROOT, "tests", "c", "user_ensemble_fused_data.hip")
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
    work = os.path.join(ROOT, "build", "test_user_ensemble_data")
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
    user.user_setup.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_double, C.c_double]
    user.user_device_pointer.restype = C.c_void_p
    user.user_device_pointer.argtypes = [C.c_void_p]
    user.user_teardown.argtypes = [C.c_void_p]
    _LIBS[ndim] = user
    return user


class Model(object):
    """one model of the test library in both wrappings.  The noise grows with sqrt(ndata), so that a proposal made from a start cloud
    of scale 0.1 changes the log-probability by about one whatever the count of data: a rate of acceptance, not 0 or 1."""

    def __init__(self, ndim, which="b", ndata=200, box=2.5, nan_above=1e300, noise=1.5, seed=11):
        self.user, self.ndim, self.which, self.ndata = _user_lib(ndim), ndim, which, ndata
        rs = np.random.RandomState(seed)
        t = np.linspace(-1.0, 1.0, max(ndata, 2))[:ndata]
        sigma = noise * np.sqrt(max(ndata, 16) / 200.0) * (1.0 + 0.5 * rs.rand(ndata))
        self.data = np.ascontiguousarray(np.stack([t, 0.2 + 0.5 * t + sigma * rs.randn(ndata), sigma]))
        self.box = float(box)
        self.h = self.user.user_setup(self.data.ctypes.data, ndata, ndim, self.box, float(nan_above))
        assert self.h

    def kernel(self):
        return targets.DeviceKernel(getattr(self.user, "user_rows_" + self.which), self.h)

    def fused(self, fn=None):
        return targets.DeviceFused(fn or getattr(self.user, "user_data_" + self.which), self.ndim, user=self.user.user_device_pointer(self.h),
                                   ndata=self.ndata)

    def close(self):
        self.user.user_teardown(self.h)


def _start(N, D, seed=5, scale=0.1):
    return scale * np.random.RandomState(seed).randn(N, D)


def _run(target, N, D, p0, mv, rng, calls=((6, {}),), seed=1234, rows=None):
    """-> everything a run leaves behind: chain, log-probs, accept counts, last state, generator"""
    s = emcee_amd.EnsembleSampler(N, D, target, moves=mv, rng=rng)
    s._random.seed(seed)
    if rows is not None:
        s._device_ensemble().set_tuning("fused_data_rows", rows)
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
    out["small"] = ens.small_info()["launches"]
    return out


def _same(a, b, kinds=(_lib.TARGET_CALLBACK, _lib.TARGET_FUSED_ENSEMBLE)):
    assert a.keys() == b.keys()
    for k in a:
        if k in ("launch_kind", "small"):
            continue
        if k == "mt":
            assert np.array_equal(a[k][0], b[k][0]) and a[k][1:] == b[k][1:], "generator state differs"
        else:
            assert np.array_equal(a[k], b[k], equal_nan=False) if not isinstance(a[k], int) else a[k] == b[k], "%s differs" % k
    assert (a["launch_kind"], b["launch_kind"]) == kinds and b["small"] == 0


def _rate(out, N, what=""):
    """the acceptance fraction of a stored run, printed, and strictly inside (0.05, 0.95)"""
    assert out["iteration"] > 0
    f = out["accepted"].sum() / float(out["iteration"] * N)
    print("acceptance %s: %.3f" % (what, f))
    assert 0.05 < f < 0.95, "acceptance fraction %.3f of %s: the comparison would be vacuous" % (f, what)
    return f


def _pair(m, N, D, mv_factory, rng, calls=((6, {}),), p0=None, what="", rows=None):
    p0 = _start(N, D) if p0 is None else p0
    ref = _run(m.kernel(), N, D, p0, mv_factory(), rng, calls)
    got = _run(m.fused(), N, D, p0, mv_factory(), rng, calls, rows=rows)
    _same(ref, got)
    if ref["iteration"] > 0:
        _rate(ref, N, what or "%s %dx%d ndata %d %s" % (m.which, N, D, m.ndata, rng))
    return ref


LIVE = dict(live_dangerously=True)       # 64 walkers at ndim > 32: the comparison is of arithmetic, not of sampling quality
MOVES = {
    "stretch": lambda: moves.StretchMove(**LIVE),
    "stretch3": lambda: moves.StretchMove(nsplits=3, **LIVE),
    "de": lambda: moves.DEMove(**LIVE),
    "snooker": lambda: moves.DESnookerMove(**LIVE),
    "de+snooker": lambda: [(moves.DEMove(**LIVE), 0.6), (moves.DESnookerMove(**LIVE), 0.4)],
    "gauss_vector": lambda: moves.GaussianMove(0.002, mode="vector"),
    "gauss_sequential": lambda: moves.GaussianMove(0.05, mode="sequential"),
    "walk": lambda: moves.WalkMove(),
}


@pytest.mark.parametrize("ndata", [0, 1, 63, 64, 65, 200, 4097])
def test_ndata_around_the_lane_stride(ndata):
    """no datum, one, a partial stride, a whole one, one more, several, and 64 whole strides and one (64 x 5, stretch, Philox)"""
    m = Model(5, ndata=ndata)
    try:
        _pair(m, 64, 5, MOVES["stretch"], "philox")
    finally:
        m.close()


@pytest.mark.parametrize("ndim", [1, 5, 16, 33, 130])
def test_every_walker_count_at_every_ndim(ndim):
    """64, 1 000 (an odd half and a partial last tile) and 4 096 walkers; ndim 130 has the 16-row tile"""
    m = Model(ndim)
    try:
        for N in (64, 1000, 4096):
            _pair(m, N, ndim, MOVES["stretch"], "philox", calls=((4, {}),))
    finally:
        m.close()


# (WalkMove proposes on the device in Philox mode only)
@pytest.mark.parametrize("move,rng", [(mv, rng) for mv in sorted(MOVES) for rng in ("philox", "mt19937") if mv != "walk" or rng == "philox"])
def test_every_move_in_both_rng_modes(move, rng):
    m = Model(5)
    try:
        _pair(m, 256, 5, MOVES[move], rng, what="%s %s" % (move, rng))
    finally:
        m.close()


@pytest.mark.parametrize("rng", ["philox", "mt19937"])
def test_thinning_unstored_and_continued_runs(rng):
    N, ndim = 256, 5
    m = Model(ndim)
    try:
        _pair(m, N, ndim, MOVES["stretch"], rng, calls=((4, dict(thin_by=3)),))
        # an unstored run counts no acceptances: its decisions are those of the stored run of the same configuration, whose rate is checked
        _pair(m, N, ndim, MOVES["de"], rng, calls=((7, dict(store=False)),))
        _pair(m, N, ndim, MOVES["de"], rng, calls=((7, {}),), what="the stored twin of the unstored run, %s" % rng)
        # two consecutive calls, the second from the device State of the first, against one call of the same length
        two = _pair(m, N, ndim, MOVES["stretch"], rng, calls=((5, {}), (6, {})))
        one = _pair(m, N, ndim, MOVES["stretch"], rng, calls=((11, {}),))
        for k in ("chain", "chain_lp", "coords", "lp", "accepted"):
            assert np.array_equal(two[k], one[k]), k
    finally:
        m.close()


@pytest.mark.parametrize("N,ndim", [(1000, 5), (4096, 16)])
def test_results_do_not_depend_on_the_rows_a_workgroup(N, ndim):
    m = Model(ndim)
    try:
        p0 = _start(N, ndim)
        ref = _run(m.kernel(), N, ndim, p0, MOVES["stretch"](), "philox", calls=((4, {}),))
        _rate(ref, N, "rows a workgroup, %dx%d" % (N, ndim))
        for rows in (4, 8, 16, 0):
            _same(ref, _run(m.fused(), N, ndim, p0, MOVES["stretch"](), "philox", calls=((4, {}),), rows=rows))
    finally:
        m.close()


def test_numpy_reproduces_the_log_probability():
    """model (a): base + targets.fused_data_sum(terms) in NumPy equals compute_log_prob bit for bit; -inf outside the box.  An oracle
    that shares no device code."""
    N, ndim, ndata = 300, 5, 200
    m = Model(ndim, which="a", ndata=ndata, box=0.2)
    try:
        x = _start(N, ndim, seed=9)
        inside = (np.abs(x) <= m.box).all(axis=1)
        assert 20 < inside.sum() < N - 20
        s = emcee_amd.EnsembleSampler(N, ndim, m.fused())
        lp, blobs = s.compute_log_prob(x)
        assert blobs is None and s._ens._target_kind == _lib.TARGET_FUSED_ENSEMBLE
        t, y, sig = m.data
        want = np.full(N, -np.inf)
        for i in np.nonzero(inside)[0]:
            r = ((y - x[i, 0] * t) - x[i, 1]) / sig
            want[i] = 0.0 + targets.fused_data_sum(-0.5 * (r * r))
        assert np.array_equal(lp, want)
        assert np.isfinite(lp[inside]).all() and len(np.unique(lp[inside])) > inside.sum() // 2
    finally:
        m.close()


def test_nan_terms_behind_an_infinite_base_are_never_evaluated():
    """model (c): term is NaN outside the box, where base is -inf.  Proposals leave the box; nothing is raised; the oracle agrees"""
    N, ndim = 256, 5
    m = Model(ndim, which="c", box=0.2)
    try:
        p0 = np.clip(_start(N, ndim), -0.19, 0.19)
        ref = _pair(m, N, ndim, MOVES["stretch"], "philox", p0=p0, calls=((8, {}),), what="model (c)")
        assert np.isfinite(ref["chain_lp"]).all()          # every walker started inside, and -inf is never accepted
        # ... and proposals did leave the box: rows evaluated there give -inf
        s = emcee_amd.EnsembleSampler(N, ndim, m.fused())
        lp, _ = s.compute_log_prob(3.0 * p0)
        assert np.isneginf(lp).any() and np.isfinite(lp).any()
    finally:
        m.close()


def test_a_nan_term_raises_the_same_error():
    """model (d): term is NaN above a threshold inside the box"""
    N, ndim = 256, 5
    m = Model(ndim, which="d", nan_above=0.25)
    try:
        p0 = np.clip(_start(N, ndim), -0.2, 0.2)           # the start is clean: only proposals reach the NaN region
        errs = []
        for t in (m.kernel(), m.fused()):
            with pytest.raises(ValueError) as e:
                _run(t, N, ndim, p0, MOVES["stretch"](), "philox", calls=((20, {}),))
            errs.append(str(e.value))
        assert errs[0] == errs[1] == "Probability function returned NaN"
    finally:
        m.close()


def test_one_launcher_call_a_half_step():
    """the launcher is wrapped by a counting one: a probe, the initial log-probs, then exactly one call a half-step, each with the
    bound count of data and rows a workgroup inside the rule's range; neither the one-workgroup nor the persistent kernel ran"""
    N, ndim, nsteps = 1000, 5, 5
    m = Model(ndim)
    try:
        real = getattr(m.user, "user_data_b")
        real.restype, real.argtypes = C.c_int, [C.c_void_p]
        calls = []

        @_lib.FUSED_ENSEMBLE_DATA_FN
        def counting(p):
            d = _lib.FusedEnsembleDataLaunch.from_address(p)
            calls.append((d.move, d.grid, d.rows, d.ndata))
            return real(p)

        got = _run(m.fused(counting), N, ndim, _start(N, ndim), MOVES["stretch"](), "philox", calls=((nsteps, {}),))
        assert got["launch_kind"] == _lib.TARGET_FUSED_ENSEMBLE and got["small"] == 0
        probes = [c for c in calls if c[1] == 0]
        evals = [c for c in calls if c[1] != 0 and c[0] == 4]
        steps = [c for c in calls if c[1] != 0 and c[0] != 4]
        assert len(probes) == 1 and len(evals) == 1 and len(steps) == 2 * nsteps
        assert all(c[0] == _lib.MOVE_STRETCH and c[3] == m.ndata and 4 <= c[2] <= 64 and c[1] == (N // 2 + c[2] - 1) // c[2] for c in steps)
        ref = _run(m.kernel(), N, ndim, _start(N, ndim), MOVES["stretch"](), "philox", calls=((nsteps, {}),))
        _same(ref, got)
        _rate(ref, N, "launch count")
    finally:
        m.close()


def test_refusals_on_the_device():
    from emcee_amd.device import DeviceEnsemble
    from emcee_amd._lib import EmxError
    m5, m16 = Model(5), Model(16)
    try:
        ens = DeviceEnsemble(64, 5)
        try:
            with pytest.raises(EmxError) as e:        # a launcher compiled for another ndim: the probe answers, nothing is launched
                ens.set_target_fused(m16.user.user_data_b, None, ndata=10)
            assert "another ndim" in str(e.value) and "ndim 5" in str(e.value)
            with pytest.raises(EmxError) as e:        # a data-free launcher bound as a data one, and the other way round
                ens.set_target_fused(m5.user.user_serial_a, None, ndata=10)
            assert "another version of emx_fused_ensemble.hpp" in str(e.value)
            with pytest.raises(EmxError) as e:
                ens.set_target_fused(m5.user.user_data_b, None)
            assert "another version of emx_fused_ensemble.hpp" in str(e.value)
            with pytest.raises(EmxError) as e:
                ens.set_target_fused(m5.user.user_data_b, None, ndata=2 ** 31)
            assert "ndata" in str(e.value)
            assert ens._target_kind == _lib.TARGET_HOST and ens.status() == 0
            ens.set_target_fused(m5.user.user_data_b, m5.user.user_device_pointer(m5.h), ndata=m5.ndata)
            with pytest.raises(EmxError) as e:
                ens._ck(ens.lib.emx_set_shard(ens.ctx, 0, 2))
            assert "one replica" in str(e.value)
            for bad in (-1, 1, 3, 257):
                with pytest.raises(EmxError) as e:        # the library's own check (DeviceEnsemble.set_tuning refuses before it)
                    ens._ck(ens.lib.emx_set_tuning(ens.ctx, b"fused_data_rows", bad))
                assert "fused_data_rows" in str(e.value)
        finally:
            ens.close()
    finally:
        m5.close()
        m16.close()
