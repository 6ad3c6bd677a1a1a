"""EnsembleBatch with a fused user target (targets.BatchFused): the user's per-row __device__ function compiled into the
one-workgroup kernel.  The oracle is the callback path: tests/c/user_fused_logprob.hip defines each model once and wraps it as a
BatchKernel callback and as a fused functor, and the fused run must equal the BatchKernel run of the same function bit for bit
(a BatchKernel member is itself pinned to the single Philox-mode sampler by tests/test_gpu_batch_callback.py).  No tolerance."""
import ctypes as C
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from emcee_amd import EnsembleBatch, PTSampler, _lib, moves  # noqa: E402
from emcee_amd.targets import BatchFused, BatchKernel, compile_fused, get_include  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
K = 20                       # USER_K of the model file
NDIMS = (2, 5, 8, 10, 32)


# ---------------------------------------------------------------------------------------------------------------- the models
def _compile_cmd(ndim, so, extra=()):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return ([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DUSER_NDIM=%d" % ndim] +
            list(extra) + ["-I" + d for d in get_include()] + [os.path.join(HERE, "c", "user_fused_logprob.hip"), "-o", so])


def _load(so):
    _lib.load()                                  # one HIP runtime per process: the library's (torch's) first
    user = C.CDLL(so)
    user.user_setup.restype = C.c_void_p
    user.user_setup.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double]
    user.user_device_pointer.restype = C.c_void_p
    user.user_device_pointer.argtypes = [C.c_void_p]
    user.user_teardown.argtypes = [C.c_void_p]
    return user


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    """every (model, ndim) compiled ONCE a session: one library per ndim (both models, both wrappings), built side by side"""
    d = tmp_path_factory.mktemp("user_fused")
    t0 = time.time()
    procs = {}
    for n in NDIMS:
        so = str(d / ("libuser_fused_%d.so" % n))
        procs[n] = (so, subprocess.Popen(_compile_cmd(n, so, ["-DUSER_WITH_NAN"] if n == 5 else []), stdout=subprocess.PIPE,
                                         stderr=subprocess.PIPE, text=True))
    out = {}
    for n, (so, p) in procs.items():
        _, err = p.communicate(timeout=1200)
        assert p.returncode == 0, err[-4000:]
        out[n] = _load(so)
    print("user_fused_logprob.hip at ndim %s: %.1f s" % (list(NDIMS), time.time() - t0))
    return out


class Model(object):
    """the data of B members on the device; .kernel(m) / .fused(m): model m ('a', 'b', 'n') as BatchKernel / BatchFused"""

    def __init__(self, user, B, D, seed, nan_member=-1, nan_above=0.0):
        rs = np.random.RandomState(seed)
        self.user, self.B, self.D = user, B, D
        self.mu = np.ascontiguousarray(0.1 * rs.randn(B, D))
        self.ivar = np.ascontiguousarray(1.0 / (0.2 + rs.rand(B, D)))
        t = np.sort(rs.uniform(-1.0, 1.0, size=(B, K)), axis=1)
        yerr = 0.05 + 0.1 * rs.rand(B, K)
        y = 0.3 * t + 0.1 + yerr * rs.randn(B, K)
        self.data = np.ascontiguousarray(np.stack([t, y, yerr], axis=1))
        self.h = user.user_setup(self.mu.ctypes.data, self.ivar.ctypes.data, self.data.ctypes.data, B, D, nan_member, nan_above)
        assert self.h

    def kernel(self, m):
        return BatchKernel(getattr(self.user, "user_block_" + m), self.h)

    def fused(self, m):
        return BatchFused(getattr(self.user, "user_fused_" + m), self.D, user=self.user.user_device_pointer(self.h))

    def close(self):
        self.user.user_teardown(self.h)


def outputs(batch):
    last = batch.get_last_sample()
    return dict(chain=batch.get_chain(), log_prob=batch.get_log_prob(), accepted=batch._accepted(), coords=last.coords,
                last_log_prob=last.log_prob, step=np.array(batch._step))


def assert_equal_runs(x, y):
    assert sorted(x) == sorted(y)
    for k in x:
        assert x[k].shape == y[k].shape and np.array_equal(x[k], y[k]), k


def start(rs, B, N, D, model):
    """an initial state: a cloud that model (b)'s box |x| <= 2.5 cuts (some walkers start at -inf, some proposals leave it)"""
    return (1.2 if model == "b" else 1.0) * rs.randn(B, N, D)


stretch = lambda: moves.StretchMove()  # noqa: E731
SHAPES = {
    # name: (nwalkers, ndim, moves, batch sizes)
    "stretch_32x5": (32, 5, stretch, (1, 7, 300)),
    "de_snooker_100x10": (100, 10, lambda: [(moves.DEMove(), 0.8), (moves.DESnookerMove(), 0.2)], (1, 7, 300)),
    "stretch3_45x2": (45, 2, lambda: moves.StretchMove(nsplits=3), (1, 7, 300)),
    "gauss_vector_64x8": (64, 8, lambda: moves.GaussianMove(0.3), (1, 7, 300)),
    "gauss_sequential_64x8": (64, 8, lambda: moves.GaussianMove(0.5, mode="sequential"), (1, 7, 300)),
    "stretch_256x32": (256, 32, stretch, (1, 7)),
}
CASES = [(name, B, model, thin) for name in sorted(SHAPES) for B in SHAPES[name][3] for model in "ab" for thin in (1, 3)]


# ---------------------------------------------------------------------------------------------------------------- 1. bit equality
@pytest.mark.parametrize("name,B,model,thin_by", CASES, ids=["%s-B%d-%s-thin%d" % c for c in CASES])
def test_fused_equals_the_callback_path(libs, name, B, model, thin_by):
    N, D, mf, _ = SHAPES[name]
    nsteps = 60
    seed = sum(map(ord, name)) + 1000 * B + 7 * thin_by + (model == "b")
    rs = np.random.RandomState(seed)
    mdl = Model(libs[D], B, D, seed + 1)
    p0 = start(rs, B, N, D, model)
    seeds = [int(s) for s in rs.randint(1, 2 ** 31, size=B)]
    fb = EnsembleBatch(B, N, D, mdl.fused(model), moves=mf(), seeds=seeds)
    fb.run_mcmc(p0, nsteps, thin_by=thin_by)
    kb = EnsembleBatch(B, N, D, mdl.kernel(model), moves=mf(), seeds=seeds)
    kb.run_mcmc(p0, nsteps, thin_by=thin_by)
    x, y = outputs(fb), outputs(kb)
    assert x["chain"].shape == (B, nsteps, N, D) and x["step"] == nsteps * thin_by
    assert_equal_runs(x, y)
    assert 0 < x["accepted"].sum() < x["accepted"].size * nsteps          # the chains move, and not every proposal is taken
    fb.close()
    kb.close()
    mdl.close()


# ---------------------------------------------------------------------------------------------------------------- 2. eval0
def test_initial_log_probs_equal_a_numpy_transcription(libs):
    B, N, D = 7, 32, 5
    rs = np.random.RandomState(2)
    mdl = Model(libs[D], B, D, 3)
    p0 = rs.randn(B, N, D)
    fb = EnsembleBatch(B, N, D, mdl.fused("a"), seeds=list(range(B)))
    st = fb.run_mcmc(p0, 0)
    acc = np.zeros((B, N))
    for d in range(D):                                # model (a)'s operation order: r = x - mu; acc = acc + ((ivar * r) * r)
        r = p0[:, :, d] - mdl.mu[:, None, d]
        acc = acc + mdl.ivar[:, None, d] * r * r
    assert np.array_equal(st.log_prob, -0.5 * acc)
    assert np.array_equal(st.coords, p0)
    assert fb.launch_info()["launches"] == 1
    fb.close()
    mdl.close()


# ---------------------------------------------------------------------------------------------------------------- 3. resume
@pytest.mark.parametrize("model", ["a", "b"])
def test_a_run_in_two_calls_equals_one(libs, model):
    B, N, D = 7, 100, 10
    mf = SHAPES["de_snooker_100x10"][2]
    rs = np.random.RandomState(31)
    mdl = Model(libs[D], B, D, 32)
    p0 = start(rs, B, N, D, model)
    seeds = list(range(70, 70 + B))
    one = EnsembleBatch(B, N, D, mdl.fused(model), moves=mf(), seeds=seeds)
    one.run_mcmc(p0, 100)
    if model == "b":                                  # the box cuts the initial cloud: -inf is a legal log-prob, and such walkers move
        probe = EnsembleBatch(B, N, D, mdl.fused(model), moves=mf(), seeds=seeds)
        first = probe.run_mcmc(p0, 0).log_prob
        assert np.isneginf(first).any() and np.isfinite(first).any()
        assert np.isfinite(one.get_last_sample().log_prob).mean() > np.isfinite(first).mean()
        probe.close()
    two = EnsembleBatch(B, N, D, mdl.fused(model), moves=mf(), seeds=seeds)
    two.run_mcmc(p0, 40)
    two.run_mcmc(None, 60)
    assert_equal_runs(outputs(one), outputs(two))
    one.close()
    two.close()
    mdl.close()


# ---------------------------------------------------------------------------------------------------------------- 4. launches
def test_one_launch_per_chunk(libs):
    B, N, D = 16, 32, 5
    rs = np.random.RandomState(4)
    mdl = Model(libs[D], B, D, 5)
    fb = EnsembleBatch(B, N, D, mdl.fused("a"), seeds=list(range(B)))
    fb.run_mcmc(rs.randn(B, N, D), 500)
    assert fb.launch_info()["launches"] == 2          # the initial evaluation + one chunk of up to 4 096 steps, as a built-in target
    fb.run_mcmc(None, 5000, store=False)
    assert fb.launch_info()["launches"] == 4          # 4 096 + 904
    fb.close()
    mdl.close()


# ---------------------------------------------------------------------------------------------------------------- 5. tuning
@pytest.mark.parametrize("name", ["de_snooker_100x10", "stretch_256x32"])
def test_launch_shape_changes_no_bit(libs, name):
    N, D, mf, _ = SHAPES[name]
    B = 5
    rs = np.random.RandomState(6)
    mdl = Model(libs[D], B, D, 7)
    p0 = start(rs, B, N, D, "b")
    seeds = list(range(B))

    def run(tuning):
        fb = EnsembleBatch(B, N, D, mdl.fused("b"), moves=mf(), seeds=seeds)
        for k, v in tuning.items():
            fb.set_tuning(k, v)
        fb.run_mcmc(p0, 30)
        out, info = outputs(fb), fb.launch_info()
        fb.close()
        return out, info
    ref, info0 = run({})
    for key, field, values in (("batch_threads", "threads", (64, 640)), ("batch_plan_steps", "plan_steps", (1, 3))):
        for v in values:
            out, info = run({key: v})
            assert info[field] == v and info0[field] != v
            assert_equal_runs(ref, out)
    mdl.close()


# ---------------------------------------------------------------------------------------------------------------- 6. NaN
def test_nan_raises_the_reference_error_naming_the_member(libs):
    B, N, D, k = 6, 32, 5, 4
    rs = np.random.RandomState(8)
    p0 = 0.05 * rs.randn(B, N, D)
    mdl = Model(libs[D], B, D, 9, nan_member=k, nan_above=0.3)         # no walker starts above 0.3; proposals get there
    fb = EnsembleBatch(B, N, D, mdl.fused("n"), seeds=list(range(B)))
    with pytest.raises(ValueError) as e:
        fb.run_mcmc(p0, 200)
    assert str(e.value).startswith("member %d: Probability function returned NaN" % k)
    fb.close()
    mdl.close()
    mdl = Model(libs[D], B, D, 9, nan_member=k, nan_above=-1e300)      # every row of member k, the initial ones included
    fb = EnsembleBatch(B, N, D, mdl.fused("n"), seeds=list(range(B)))
    with pytest.raises(ValueError) as e:
        fb.run_mcmc(p0, 10)
    assert str(e.value).startswith("member %d: The initial log_prob was NaN" % k)
    fb.close()
    # model (n) carries the single-StretchMove kernel alone: another schedule is refused by its launcher, by name
    fb = EnsembleBatch(B, N, D, mdl.fused("n"), moves=moves.DEMove(), seeds=list(range(B)))
    with pytest.raises(_lib.EmxError) as e:
        fb.run_mcmc(p0, 10)
    assert "EMX_FUSED_MOVES_ANY" in str(e.value)
    fb.close()
    mdl.close()


# ---------------------------------------------------------------------------------------------------------------- 7. what hangs off the handle
def test_summary_and_autocorr_on_the_fused_handle(libs):
    B, N, D, nsteps = 7, 32, 5, 400
    rs = np.random.RandomState(10)
    mdl = Model(libs[D], B, D, 11)
    p0 = rs.randn(B, N, D)
    seeds = list(range(B))
    fb = EnsembleBatch(B, N, D, mdl.fused("a"), seeds=seeds)
    fb.run_mcmc(p0, nsteps)
    kb = EnsembleBatch(B, N, D, mdl.kernel("a"), seeds=seeds)
    kb.run_mcmc(p0, nsteps)
    sf, sk = fb.get_summary(discard=50), kb.get_summary(discard=50)
    assert sf.nsamples == sk.nsamples
    for u, v in zip(sf[1:], sk[1:]):
        assert np.array_equal(u, v)
    tf = fb.get_autocorr_time(discard=50, on_device=True, quiet=True)
    tk = kb.get_autocorr_time(discard=50, on_device=True, quiet=True)
    assert tf.shape == (B, D) and np.array_equal(tf, tk, equal_nan=True)
    fb.close()
    kb.close()
    mdl.close()


# ---------------------------------------------------------------------------------------------------------------- 8. the ABI guard
def test_a_launcher_of_another_header_version_is_refused_at_bind_time(libs, tmp_path):
    so = str(tmp_path / "libuser_fused_wrong.so")
    subprocess.run(_compile_cmd(5, so, ["-DEMX_FUSED_ABI=4242u"]), check=True, timeout=900, capture_output=True)
    wrong = _load(so)
    B, N, D = 3, 32, 5
    mdl = Model(wrong, B, D, 12)
    fb = EnsembleBatch(B, N, D, mdl.fused("a"), seeds=list(range(B)))
    with pytest.raises(_lib.EmxError) as e:
        fb.run_mcmc(np.random.RandomState(0).randn(B, N, D), 10)
    assert "another version of emx_fused_target.hpp" in str(e.value)
    assert fb.launch_info()["launches"] == 0
    fb.close()
    mdl.close()
    # a hand-written launcher that answers non-zero to the probe: refused, nothing launched
    refuse = _lib.FUSED_BATCH_FN(lambda launch: 1)
    fb = EnsembleBatch(B, N, D, BatchFused(refuse, D), seeds=list(range(B)))
    with pytest.raises(_lib.EmxError) as e:
        fb.run_mcmc(np.random.RandomState(0).randn(B, N, D), 10)
    assert "another version" in str(e.value) and fb.launch_info()["launches"] == 0
    fb.close()


# ---------------------------------------------------------------------------------------------------------------- 9. PT
def test_ptsampler_and_tempering_refuse_a_fused_target(libs):
    B, N, D = 4, 32, 5
    mdl = Model(libs[D], B, D, 13)
    with pytest.raises(TypeError) as e:
        PTSampler(2, N, D, mdl.fused("a"), nbatch=2)
    assert "BatchCallable" in str(e.value) and "BatchKernel" in str(e.value)
    fb = EnsembleBatch(B, N, D, mdl.fused("a"), seeds=list(range(B)))
    h = fb._handle()
    rc = _lib.load().emx_pt_set_tempering(h, 2, np.array([1.0, 0.5]), None, None)
    assert rc != 0 and b"fused user target" in _lib.load().emx_batch_last_error(h)
    fb.close()
    mdl.close()


# ---------------------------------------------------------------------------------------------------------------- compile_fused
def test_compile_fused_end_to_end(tmp_path):
    """the Python route: source -> compile_fused -> BatchFused with a torch tensor as the user's data; against the built-in
    DiagGaussian's statistics (another arithmetic, so not its bits): the sample mean of a long run"""
    src = r"""
    struct Shifted {
        __device__ double operator()(const double* x, int ndim, int member, const void* user) const {
            const double* mu = (const double*)user + (long long)member * ndim;
            double acc = 0.0;
            for (int d = 0; d < ndim; ++d) acc = acc + (x[d] - mu[d]) * (x[d] - mu[d]);
            return -0.5 * acc;
        }
    };
    """
    B, N, D = 4, 32, 3
    lib = compile_fused(src, "Shifted", D, cache_dir=str(tmp_path))
    mu = torch.arange(B * D, dtype=torch.float64, device="cuda").reshape(B, D)
    rs = np.random.RandomState(14)
    p0 = mu.cpu().numpy()[:, None, :] + rs.randn(B, N, D)
    fb = EnsembleBatch(B, N, D, lib.target(user=mu), seeds=list(range(B)))
    st = fb.run_mcmc(p0, 0)
    r = p0 - mu.cpu().numpy()[:, None, :]
    acc = np.zeros((B, N))
    for d in range(D):
        acc = acc + r[:, :, d] * r[:, :, d]
    assert np.array_equal(st.log_prob, -0.5 * acc)
    fb.run_mcmc(None, 2000)
    mean = fb.get_chain(discard=500).mean(axis=(1, 2))
    assert np.all(np.abs(mean - mu.cpu().numpy()) < 0.15)          # sigma / sqrt(n_eff) ~ 1 / sqrt(48 000 / ~30) = 0.025: 6 sigma
    fb.close()
