"""PTSampler with a fused tempered likelihood (targets.PTFused): the user's per-row __device__ likelihood and prior compiled into
k_pt_run, one workgroup an object.  The oracle is the callback path: tests/c/user_pt_fused.hip defines each function once and wraps
it as a BatchKernel and as a fused functor, and the fused run must equal the BatchKernel run bit for bit (that run is itself pinned
to a NumPy swap oracle, the host ladder twin and EnsembleBatch by tests/test_gpu_pt.py and tests/test_gpu_pt_adapt.py).  No
tolerance.  No proposal of these runs has a non-finite coordinate."""
import ctypes as C
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from emcee_amd import PTSampler, _lib, moves  # noqa: E402
from emcee_amd.pt import thermodynamic_integration_log_evidence  # noqa: E402
from emcee_amd.targets import BatchKernel, PTFused, compile_fused_pt, get_include  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NDIMS = (3, 5, 7, 16)


def _compile_cmd(ndim, so, extra=()):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return ([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DUSER_NDIM=%d" % ndim] +
            list(extra) + ["-I" + d for d in get_include()] + [os.path.join(HERE, "c", "user_pt_fused.hip"), "-o", so])


def _load(so):
    _lib.load()                                  # one HIP runtime per process: the library's (torch's) first
    user = C.CDLL(so)
    user.user_setup.restype = C.c_void_p
    user.user_setup.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double]
    user.user_device_pointer.restype = C.c_void_p
    user.user_device_pointer.argtypes = [C.c_void_p]
    user.user_teardown.argtypes = [C.c_void_p]
    return user


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    """one library per ndim (every model, both wrappings), built side by side"""
    d = tmp_path_factory.mktemp("user_pt_fused")
    t0 = time.time()
    procs = {}
    for n in NDIMS:
        so = str(d / ("libuser_pt_fused_%d.so" % n))
        procs[n] = (so, subprocess.Popen(_compile_cmd(n, so, ["-DUSER_WITH_NAN"] if n == 5 else []), stdout=subprocess.PIPE,
                                         stderr=subprocess.PIPE, text=True))
    out = {}
    for n, (so, p) in procs.items():
        _, err = p.communicate(timeout=1200)
        assert p.returncode == 0, err[-4000:]
        out[n] = _load(so)
    print("user_pt_fused.hip at ndim %s: %.1f s" % (list(NDIMS), time.time() - t0))
    return out


class Model(object):
    """the data of `members` = nbatch * ntemps members on the device; .kernel(m) / .fused(m): function m as BatchKernel / PTFused"""

    def __init__(self, user, members, D, seed, nan_member=-1, nan_above=0.0, bound=3.0):
        rs = np.random.RandomState(seed)
        self.user, self.D = user, D
        self.mu = np.ascontiguousarray(0.1 * rs.randn(members, D))
        self.ivar = np.ascontiguousarray(1.0 / (0.2 + rs.rand(members, D)))
        self.h = user.user_setup(self.mu.ctypes.data, self.ivar.ctypes.data, members, D, nan_member, nan_above, bound)
        assert self.h

    def kernel(self, m):
        return BatchKernel(getattr(self.user, "user_block_" + m), self.h)

    def fused(self, m):
        return PTFused(getattr(self.user, "pt_fused_" + m), self.D, user=self.user.user_device_pointer(self.h))

    def close(self):
        self.user.user_teardown(self.h)


def outputs(pt, stored=True):
    last = pt.get_last_sample()
    L, P = pt._pt_state()
    att, acc = pt._swap_counts()
    out = dict(coords=last.coords, last_log_prob=last.log_prob, L=L, P=P, ladder=pt.ladder, updates=np.array(pt.adaptation_updates),
               accepted=pt._b._accepted().reshape(L.shape), attempts=att, swaps=acc, step=np.array(pt._b._step))      # (counts: stored steps only)
    if stored:
        out.update(chain=pt.get_chain(), log_prob=pt.get_log_prob(), log_like=pt.get_log_likelihood(), betas=pt.get_betas())
    return out


def assert_equal_runs(x, y):
    assert sorted(x) == sorted(y)
    for k in x:
        assert x[k].shape == y[k].shape and np.array_equal(x[k], y[k]), k


MOVES = {
    "stretch": lambda: moves.StretchMove(),
    "de_snooker": lambda: [(moves.DEMove(), 0.8), (moves.DESnookerMove(), 0.2)],
    "gauss": lambda: moves.GaussianMove(0.3),
}
SHAPES = [(3, 4, 32, 3), (5, 16, 32, 5), (2, 8, 64, 16), (2, 3, 33, 7)]
# prior: "box" (the handle's), "functor" (pt_fused_ap against a BatchKernel prior), "none"
CASES = []
for i, shape in enumerate(SHAPES):
    for j, mv in enumerate(sorted(MOVES)):
        for every in (0, 1, 3):
            k = i + j + every
            CASES.append((shape, mv, every, (1, 3)[k % 2], ("box", "functor", "none")[k % 3]))


def pair(libs, shape, mv, prior, seed, like="a", **kw):
    """-> (fused sampler, BatchKernel sampler, model) of one configuration"""
    G, T, N, D = shape
    mdl = Model(libs[D], G * T, D, seed + 1)
    box = (-3.0 * np.ones(D), 3.0 * np.ones(D))
    common = dict(nbatch=G, moves=None, seeds=[seed + 10 * g for g in range(G)])
    common.update(kw)
    mk = (lambda: MOVES[mv]()) if isinstance(mv, str) else mv
    if prior == "functor":
        f = PTSampler(T, N, D, mdl.fused(like + "p"), **dict(common, moves=mk()))
        k = PTSampler(T, N, D, mdl.kernel(like), log_prior=mdl.kernel("p"), **dict(common, moves=mk()))
    else:
        lp = box if prior == "box" else None
        f = PTSampler(T, N, D, mdl.fused(like), log_prior=lp, **dict(common, moves=mk()))
        k = PTSampler(T, N, D, mdl.kernel(like), log_prior=lp, **dict(common, moves=mk()))
    return f, k, mdl


# ---------------------------------------------------------------------------------------------------------------- 1. bit equality
@pytest.mark.parametrize("shape,mv,every,thin_by,prior", CASES, ids=["%s-%s-swap%d-thin%d-%s" % ("x".join(map(str, c[0])), c[1], c[2], c[3], c[4])
                                                                      for c in CASES])
def test_fused_equals_the_callback_path(libs, shape, mv, every, thin_by, prior):
    G, T, N, D = shape
    seed = 100 * G + 7 * T + N + D + every + thin_by
    f, k, mdl = pair(libs, shape, mv, prior, seed, swap_every=every)
    p0 = 0.8 * np.random.RandomState(seed).randn(G, T, N, D)
    nsteps = 25
    f.run_mcmc(p0, nsteps, thin_by=thin_by)
    k.run_mcmc(p0, nsteps, thin_by=thin_by)
    x, y = outputs(f), outputs(k)
    assert x["chain"].shape == (G, T, nsteps, N, D) and x["step"] == nsteps * thin_by
    assert_equal_runs(x, y)
    assert 0 < x["accepted"].sum() < x["accepted"].size * nsteps and np.array_equal(f.acceptance_fraction, k.acceptance_fraction)
    if every and T > 1:
        assert x["attempts"].sum() > 0 and x["swaps"].sum() > 0
    f.close()
    k.close()
    mdl.close()


def test_a_ladder_down_to_beta_zero_with_walkers_outside_the_box(libs):
    shape = G, T, N, D = 3, 4, 32, 3
    f, k, mdl = pair(libs, shape, "stretch", "box", 5, swap_every=1, betas=np.array([1.0, 0.3, 0.05, 0.0]))
    p0 = 2.0 * np.random.RandomState(6).randn(G, T, N, D)          # the box is |x| <= 3: some walkers start outside (P = -inf)
    f.run_mcmc(p0, 0)
    assert np.isneginf(f._pt_state()[1]).any()
    f.run_mcmc(None, 40)
    k.run_mcmc(p0, 40)
    assert_equal_runs(outputs(f), outputs(k))
    f.close()
    k.close()
    mdl.close()


# ---------------------------------------------------------------------------------------------------------------- 2. adaptation
def test_adaptive_ladder_then_frozen(libs):
    shape = G, T, N, D = 5, 16, 32, 5
    f, k, mdl = pair(libs, shape, "stretch", "box", 11, swap_every=1, adaptive=True, adaptation_lag=20, adaptation_time=2)
    p0 = 0.8 * np.random.RandomState(12).randn(G, T, N, D)
    for s in (f, k):
        s.run_mcmc(p0, 40)
    assert f.adaptation_updates == 40 and not np.array_equal(f.ladder, np.tile(f.betas, (G, 1)))      # the ladder visibly moved
    assert_equal_runs(outputs(f), outputs(k))
    for s in (f, k):
        s.adaptive = False
        s.run_mcmc(None, 20)
    x, y = outputs(f), outputs(k)
    assert_equal_runs(x, y)
    assert x["updates"] == 40 and np.array_equal(x["betas"][:, 40:], np.broadcast_to(x["ladder"][:, None, :], x["betas"][:, 40:].shape))
    f.close()
    k.close()
    mdl.close()


# ---------------------------------------------------------------------------------------------------------------- 3. composition
def test_a_run_in_three_calls_equals_one_and_unstored_runs_leave_the_same_state(libs):
    shape = G, T, N, D = 3, 4, 32, 3
    p0 = 0.8 * np.random.RandomState(21).randn(G, T, N, D)
    one, k, mdl = pair(libs, shape, "de_snooker", "functor", 22, swap_every=3)
    one.run_mcmc(p0, 30)
    k.run_mcmc(p0, 30)
    assert_equal_runs(outputs(one), outputs(k))
    three, k2, mdl2 = pair(libs, shape, "de_snooker", "functor", 22, swap_every=3)
    three.run_mcmc(p0, 10)
    three.run_mcmc(None, 10)
    three.run_mcmc(None, 10)
    assert_equal_runs(outputs(one), outputs(three))
    k2.run_mcmc(p0, 30, store=False)
    blind, k3, mdl3 = pair(libs, shape, "de_snooker", "functor", 22, swap_every=3)
    blind.run_mcmc(p0, 30, store=False)
    assert_equal_runs(outputs(blind, stored=False), outputs(k2, stored=False))
    assert np.array_equal(blind.get_last_sample().coords, one.get_last_sample().coords)
    for s in (one, k, three, k2, blind, k3):
        s.close()
    for m in (mdl, mdl2, mdl3):
        m.close()


# ---------------------------------------------------------------------------------------------------------------- 4. launch shape
def test_launch_shape_changes_no_bit(libs):
    shape = G, T, N, D = 5, 16, 32, 5
    p0 = 0.8 * np.random.RandomState(31).randn(G, T, N, D)

    def run(tuning):
        f, k, mdl = pair(libs, shape, "de_snooker", "box", 32, swap_every=1)
        for key, v in tuning.items():
            f.set_tuning(key, v)
        f.run_mcmc(p0, 20)
        out, info = outputs(f), f.launch_info()
        f.close()
        k.close()
        mdl.close()
        return out, info
    ref, info0 = run({})
    for tuning in (dict(batch_threads=64, batch_plan_steps=3), dict(batch_threads=256, batch_plan_steps=2)):
        out, info = run(tuning)
        assert info["threads"] == tuning["batch_threads"] != info0["threads"] and info["plan_steps"] == tuning["batch_plan_steps"]
        assert_equal_runs(ref, out)


# ---------------------------------------------------------------------------------------------------------------- 5. launches
def test_one_launch_per_chunk(libs):
    """a chunk is up to 4 096 proposal steps; both runs below stay under it"""
    shape = G, T, N, D = 3, 4, 32, 3
    f, k, mdl = pair(libs, shape, "stretch", "box", 41, swap_every=1)
    p0 = 0.8 * np.random.RandomState(42).randn(G, T, N, D)
    grew = {}
    for name, s in (("fused", f), ("kernel", k)):
        s.run_mcmc(p0, 1, store=False)
        for n in (10, 100):
            n0 = s.launch_info()["launches"]
            s.run_mcmc(None, n, store=False)
            grew[name, n] = s.launch_info()["launches"] - n0
    assert grew["fused", 10] == grew["fused", 100] == 1
    assert grew["kernel", 100] > grew["kernel", 10] >= 10 * 3
    f.close()
    k.close()
    mdl.close()


# ---------------------------------------------------------------------------------------------------------------- 6. NaN, ABI, state
def test_nan_raises_the_reference_error_naming_object_and_rung(libs):
    G, T, N, D, bad = 3, 4, 32, 5, 6
    p0 = 0.05 * np.random.RandomState(51).randn(G, T, N, D)
    mdl = Model(libs[D], G * T, D, 52, nan_member=bad, nan_above=0.3)         # no walker starts above 0.3; proposals get there
    f = PTSampler(T, N, D, mdl.fused("n"), nbatch=G, seeds=[1, 2, 3])
    with pytest.raises(ValueError) as e:
        f.run_mcmc(p0, 200)
    assert str(e.value).startswith("(object %d, rung %d): Probability function returned NaN" % divmod(bad, T))
    f.close()
    mdl.close()
    mdl = Model(libs[D], G * T, D, 52, nan_member=bad, nan_above=-1e300)
    f = PTSampler(T, N, D, mdl.fused("n"), nbatch=G, seeds=[1, 2, 3])
    with pytest.raises(ValueError) as e:
        f.run_mcmc(p0, 10)
    assert str(e.value).startswith("(object %d, rung %d): The initial log_prob was NaN" % divmod(bad, T))
    f.close()
    mdl.close()


def test_a_launcher_of_another_header_version_is_refused_at_bind_time(libs, tmp_path):
    so = str(tmp_path / "libuser_pt_fused_wrong.so")
    subprocess.run(_compile_cmd(3, so, ["-DEMX_FUSED_PT_ABI=4242u"]), check=True, timeout=900, capture_output=True)
    wrong = _load(so)
    G, T, N, D = 2, 4, 32, 3
    mdl = Model(wrong, G * T, D, 61)
    f = PTSampler(T, N, D, mdl.fused("a"), nbatch=G, seeds=[1, 2])
    with pytest.raises(_lib.EmxError) as e:
        f.run_mcmc(np.random.RandomState(0).randn(G, T, N, D), 10)
    assert "another version of emx_pt_fused.hpp" in str(e.value)
    assert f.launch_info()["launches"] == 0
    f.close()
    mdl.close()


def test_state_and_swap_after_a_fused_run(libs):
    shape = G, T, N, D = 3, 4, 32, 3
    f, k, mdl = pair(libs, shape, "stretch", "box", 71, swap_every=0)
    p0 = 0.8 * np.random.RandomState(72).randn(G, T, N, D)
    for s in (f, k):
        s.run_mcmc(p0, 15)
        s._swap()                                     # k_pt_swap on the state the fused kernel left
    assert_equal_runs(outputs(f), outputs(k))
    assert outputs(f)["swaps"].sum() > 0
    s1, s2 = f.get_summary(), k.get_summary()
    for u, v in zip(s1[1:], s2[1:]):
        assert np.array_equal(u, v)
    assert np.array_equal(f.mean_log_likelihood(5), k.mean_log_likelihood(5))
    f.close()
    k.close()
    mdl.close()


# ---------------------------------------------------------------------------------------------------------------- 7. compile_fused_pt
def exact_mean_loglike(beta, a=10.0, D=2):
    from math import erf
    if beta == 0:
        return -D / 2 * np.log(2 * np.pi) - 0.5 * D * a * a / 3
    s = 1 / np.sqrt(beta)
    z = a / s
    phi = np.exp(-z * z / 2) / np.sqrt(2 * np.pi)
    ex2 = s * s * (1 - 2 * z * phi / erf(z / np.sqrt(2)))
    return -D / 2 * np.log(2 * np.pi) - 0.5 * D * ex2


def test_evidence_end_to_end_through_compile_fused_pt(tmp_path):
    """tests/test_gpu_pt.py's evidence test (the same model, shape, seeds and thresholds) with the likelihood compiled by
    compile_fused_pt and a torch tensor as the functor's `user` (it holds the normalisation constant)"""
    src = r"""
    struct Gauss {
        __device__ double operator()(const double* x, int ndim, int member, const void* user) const {
            double acc = 0.0;
            for (int d = 0; d < ndim; ++d) acc = acc + x[d] * x[d];
            return -0.5 * acc - *(const double*)user;
        }
    };
    """
    G, T, N, D, nsteps = 4, 40, 32, 2, 2000
    lib = compile_fused_pt(src, "Gauss", D, cache_dir=str(tmp_path))
    norm = torch.full((1,), float(np.log(2 * np.pi)), dtype=torch.float64, device="cuda")
    pt = PTSampler(T, N, D, lib.target(user=norm), log_prior=(-10 * np.ones(D), 10 * np.ones(D)), Tmax=1e4, nbatch=G,
                   seeds=[31, 32, 33, 34])
    rs = np.random.RandomState(9)
    pt.run_mcmc(rs.uniform(-1, 1, size=(G, T, N, D)), nsteps)
    assert pt.launch_info()["launches"] == 2          # the initial evaluation and one chunk
    logz, dlogz = pt.log_evidence_estimate()
    exact, _ = thermodynamic_integration_log_evidence(pt.betas, np.array([exact_mean_loglike(b) for b in pt.betas]))
    mc = np.std(logz)
    assert np.all(np.abs(logz - exact) < max(0.05, 4 * mc)), (logz, exact, mc)
    assert np.all(np.abs(logz - (-2 * np.log(20))) < 0.2), logz
    dev = pt.mean_log_likelihood(int(0.1 * pt.iteration))
    host = pt.get_log_likelihood(discard=int(0.1 * pt.iteration)).mean(axis=(2, 3))
    assert np.allclose(dev, host, rtol=1e-12, atol=0)
    pt.close()
