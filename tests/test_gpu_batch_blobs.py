"""Blobs of EnsembleBatch on the GPU: derived quantities produced with every log-probability, committed with it and stored in a
blob plane next to the chain.  tests/c/user_blobs_logprob.hip defines each model once and wraps it as a fused functor with blobs,
as the same functor without blobs, and as a BatchKernel callback with blobs.

The blobs are {lp itself, x[0] + x[1], x[0] * x[1], (double)member}: single correctly rounded operations on stored coordinates
(the model file is compiled with -ffp-contract=off), so every comparison with NumPy on get_chain() / get_log_prob() is exact.
The summary's mean and covariance are held to the bounds tests/test_gpu_batch_summary.py derives for coordinates (the same
kernels run on the blob plane); order statistics and the MAP blob are exact."""
import ctypes as C
import math
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from emcee_amd import EnsembleBatch, State, _lib, moves, summary  # noqa: E402
from emcee_amd.targets import BatchCallable, BatchFused, BatchKernel, get_include  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
K = 4                        # USER_NBLOBS of the model file
NDIMS = (5, 8)               # odd and even: the two row layouts (V = 1, V = 2)
NWALKERS = {5: 32, 8: 64}
U = 2.0 ** -53


# ---------------------------------------------------------------------------------------------------------------- the models
def _compile_cmd(ndim, so):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return ([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DUSER_NDIM=%d" % ndim] +
            ["-I" + d for d in get_include()] + [os.path.join(HERE, "c", "user_blobs_logprob.hip"), "-o", so])


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    """one library per ndim (both models, all three wrappings), built side by side; each compile is bounded"""
    d = tmp_path_factory.mktemp("user_blobs")
    t0 = time.time()
    procs = {}
    for n in NDIMS:
        so = str(d / ("libuser_blobs_%d.so" % n))
        procs[n] = (so, subprocess.Popen(_compile_cmd(n, so), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    out = {}
    _lib.load()                                      # one HIP runtime per process: the library's (torch's) first
    for n, (so, p) in procs.items():
        _, err = p.communicate(timeout=1200)
        assert p.returncode == 0, err[-4000:]
        user = C.CDLL(so)
        user.user_setup.restype = C.c_void_p
        user.user_setup.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double]
        user.user_device_pointer.restype = C.c_void_p
        user.user_device_pointer.argtypes = [C.c_void_p]
        user.user_ninf.restype = C.c_longlong
        user.user_ninf.argtypes = [C.c_void_p]
        user.user_teardown.argtypes = [C.c_void_p]
        out[n] = user
    print("user_blobs_logprob.hip at ndim %s: %.1f s" % (list(NDIMS), time.time() - t0))
    return out


class Model(object):
    """the data of B members on the device; model 'g' (diagonal Gaussian) or 'x' (the same inside the box |x| <= half)"""

    def __init__(self, user, B, D, seed, half=1.5):
        rs = np.random.RandomState(seed)
        self.user, self.B, self.D, self.half = user, B, D, half
        self.mu = np.ascontiguousarray(0.1 * rs.randn(B, D))
        self.ivar = np.ascontiguousarray(1.0 / (0.2 + rs.rand(B, D)))
        self.h = user.user_setup(self.mu.ctypes.data, self.ivar.ctypes.data, B, D, half)
        assert self.h

    def fused(self, m):                               # with blobs
        return BatchFused(getattr(self.user, "user_fused_%s_blobs" % m), self.D, user=self.user.user_device_pointer(self.h), nblobs=K)

    def plain(self, m):                               # the same functor without blobs
        return BatchFused(getattr(self.user, "user_fused_" + m), self.D, user=self.user.user_device_pointer(self.h))

    def kernel(self, m):                              # the batched callback with blobs
        return BatchKernel(getattr(self.user, "user_block_%s_blobs" % m), self.h, nblobs=K)

    def torch_fn(self, m):
        """the model in torch, operation for operation (separate multiplies and adds, ascending d), returning (lp, blobs)"""
        mu = torch.as_tensor(self.mu, device="cuda")
        iv = torch.as_tensor(self.ivar, device="cuda")
        member = torch.arange(self.B, dtype=torch.float64, device="cuda")[:, None]
        half, D = self.half, self.D

        def fn(q):
            acc = torch.zeros(q.shape[:2], dtype=torch.float64, device=q.device)
            for d in range(D):
                r = q[:, :, d] - mu[:, None, d]
                acc = acc + iv[:, None, d] * r * r
            lp = -0.5 * acc
            if m == "x":
                inside = ((q >= -half) & (q <= half)).all(-1)
                lp = torch.where(inside, lp, torch.full_like(lp, -math.inf))
            blobs = torch.stack([lp, q[:, :, 0] + q[:, :, 1], q[:, :, 0] * q[:, :, 1], member.expand_as(lp)], dim=-1)
            return lp, blobs
        return fn

    def ninf(self):
        return self.user.user_ninf(self.h)

    def close(self):
        self.user.user_teardown(self.h)


def start(rs, B, N, D, model, half=1.5):
    """model (x): every walker starts inside the box, close enough to its walls for proposals to leave it"""
    return rs.uniform(-0.95 * half, 0.95 * half, size=(B, N, D)) if model == "x" else rs.randn(B, N, D)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def outputs(batch):
    last = batch.get_last_sample()
    return dict(chain=batch.get_chain(), log_prob=batch.get_log_prob(), accepted=batch._accepted(), coords=last.coords,
                last_log_prob=last.log_prob, step=np.array(batch._step, dtype=np.float64))


def assert_equal_runs(x, y):
    assert sorted(x) == sorted(y)
    for k in x:
        assert same_bits(x[k], y[k]), k


def assert_blobs_follow_the_chain(blobs, chain, lp):
    """blobs (B, T, N, 4) against the same NumPy expressions on the stored chain (B, T, N, D) and log-probs: bit for bit"""
    B = chain.shape[0]
    assert blobs.shape == chain.shape[:3] + (K,)
    assert same_bits(blobs[..., 0], lp)
    assert same_bits(blobs[..., 1], chain[..., 0] + chain[..., 1])
    assert same_bits(blobs[..., 2], chain[..., 0] * chain[..., 1])
    assert same_bits(blobs[..., 3], np.broadcast_to(np.arange(B, dtype=np.float64)[:, None, None], lp.shape))


MOVES = {
    "stretch": lambda: moves.StretchMove(),
    "de": lambda: moves.DEMove(),
    "snooker": lambda: moves.DESnookerMove(),
    "gauss": lambda: moves.GaussianMove(0.3),
    "mix": lambda: [(moves.StretchMove(), 0.5), (moves.DEMove(), 0.3), (moves.DESnookerMove(), 0.2)],
}
CASES = [(mv, D, thin, model) for mv in sorted(MOVES) for D in NDIMS for thin in (1, 3) for model in "gx"]


# ---------------------------------------------------------------------------------------------------------------- 1. consistency
@pytest.mark.parametrize("mv,D,thin_by,model", CASES, ids=["%s-D%d-thin%d-%s" % c for c in CASES])
def test_blobs_follow_the_chain_and_sampling_is_unchanged(libs, mv, D, thin_by, model):
    """get_blobs() against NumPy on get_chain() / get_log_prob(), exactly; and chain, log-prob and accept counts equal to the run of
    the same functor compiled without blobs, bit for bit.  Model (x): the -inf region is hit, and a rejected walker keeps its blobs."""
    B, N, nsteps = 7, NWALKERS[D], 40
    seed = sum(map(ord, mv)) + 100 * D + 7 * thin_by + (model == "x")
    rs = np.random.RandomState(seed)
    mdl = Model(libs[D], B, D, seed + 1)
    p0 = start(rs, B, N, D, model)
    seeds = [int(s) for s in rs.randint(1, 2 ** 31, size=B)]
    fb = EnsembleBatch(B, N, D, mdl.fused(model), moves=MOVES[mv](), seeds=seeds)
    fb.run_mcmc(p0, nsteps, thin_by=thin_by)
    ninf = mdl.ninf()
    x = outputs(fb)
    blobs = fb.get_blobs()
    assert x["chain"].shape == (B, nsteps, N, D) and x["step"] == nsteps * thin_by
    assert_blobs_follow_the_chain(blobs, x["chain"], x["log_prob"])
    assert 0 < x["accepted"].sum() < x["accepted"].size * nsteps          # the chains move, and not every proposal is taken
    # a walker that did not move between two stored rows kept its blobs
    still = (x["chain"][:, 1:] == x["chain"][:, :-1]).all(-1)
    assert still.any() and same_bits(blobs[:, 1:][still], blobs[:, :-1][still])
    if model == "x":
        assert ninf > 0                                # proposals left the box: rejected at -inf ...
        assert np.isfinite(x["log_prob"]).all() and np.isfinite(blobs).all()        # ... and their blobs {-inf, ...} reached no walker
        assert (np.abs(x["chain"]) <= mdl.half).all()
    pb = EnsembleBatch(B, N, D, mdl.plain(model), moves=MOVES[mv](), seeds=seeds)
    pb.run_mcmc(p0, nsteps, thin_by=thin_by)
    assert pb.get_blobs() is None and pb.get_last_sample().blobs is None
    assert_equal_runs(x, outputs(pb))
    # the getters' selection and the member view
    assert same_bits(fb.get_blobs(discard=5, thin=2, flat=True), blobs[:, 6::2].reshape(B, -1, K))
    assert same_bits(fb[3].get_blobs(discard=5), blobs[3, 5:])
    fb.close()
    pb.close()
    mdl.close()


# ---------------------------------------------------------------------------------------------------------------- 2. the three paths
@pytest.mark.parametrize("mv,D,model", [("stretch", 5, "g"), ("mix", 8, "x"), ("gauss", 8, "g"), ("de", 5, "x")])
def test_fused_blobs_equal_the_callback_paths(libs, mv, D, model):
    B, N, nsteps = 5, NWALKERS[D], 30
    rs = np.random.RandomState(40 + D + len(mv))
    mdl = Model(libs[D], B, D, 41)
    p0 = start(rs, B, N, D, model)
    seeds = list(range(11, 11 + B))
    runs = {}
    for name, tg in (("fused", mdl.fused(model)), ("kernel", mdl.kernel(model)), ("torch", BatchCallable(mdl.torch_fn(model), nblobs=K))):
        bt = EnsembleBatch(B, N, D, tg, moves=MOVES[mv](), seeds=seeds)
        bt.run_mcmc(p0, nsteps, thin_by=2)
        runs[name] = dict(outputs(bt), blobs=bt.get_blobs(), last_blobs=bt.get_last_sample().blobs)
        bt.close()
    assert_equal_runs(runs["fused"], runs["kernel"])                       # the same device function: blobs included
    t = runs["torch"]
    assert same_bits(t["chain"], runs["fused"]["chain"]) and same_bits(t["log_prob"], runs["fused"]["log_prob"])
    assert_blobs_follow_the_chain(t["blobs"], t["chain"], t["log_prob"])   # its blobs: its own function on its own chain
    assert same_bits(t["last_blobs"], t["blobs"][:, -1])
    mdl.close()


# ---------------------------------------------------------------------------------------------------------------- 3. state
def test_last_sample_resume_and_the_initial_evaluation(libs):
    B, N, D = 7, 64, 8
    rs = np.random.RandomState(50)
    mdl = Model(libs[D], B, D, 51)
    p0 = start(rs, B, N, D, "x")
    seeds = list(range(70, 70 + B))
    mf = MOVES["mix"]
    one = EnsembleBatch(B, N, D, mdl.fused("x"), moves=mf(), seeds=seeds)
    st = one.run_mcmc(p0, 100)
    blobs = one.get_blobs()
    assert st.blobs.shape == (B, N, K) and same_bits(st.blobs, blobs[:, -1])
    assert same_bits(one[2].get_last_sample().blobs, blobs[2, -1])
    two = EnsembleBatch(B, N, D, mdl.fused("x"), moves=mf(), seeds=seeds)
    two.run_mcmc(p0, 40)
    two.run_mcmc(None, 60)                            # the chain (and the blob plane) grows, what is stored stays
    assert_equal_runs(outputs(one), outputs(two))
    assert same_bits(two.get_blobs(), blobs) and same_bits(two.get_last_sample().blobs, st.blobs)
    # the initial state alone: its blobs are the function on it, whether or not the caller supplied log-probs
    for init in (p0, State(p0, log_prob=np.zeros((B, N)))):
        z = EnsembleBatch(B, N, D, mdl.fused("x"), moves=mf(), seeds=seeds)
        s0 = z.run_mcmc(init, 0)
        assert_blobs_follow_the_chain(s0.blobs[:, None], p0[:, None], s0.log_prob[:, None])
        assert not (s0.log_prob == 0).any()
        z.run_mcmc(None, 1)                           # the first stored row: the supplied log-probs left no blob unset
        assert same_bits(z.get_blobs(), blobs[:, :1]) and same_bits(z.get_log_prob(), one.get_log_prob()[:, :1])
        z.close()
    one.close()
    two.close()
    mdl.close()


@pytest.mark.parametrize("D", NDIMS)
def test_launch_shape_changes_no_bit(libs, D):
    B, N = 5, NWALKERS[D]
    rs = np.random.RandomState(6)
    mdl = Model(libs[D], B, D, 7)
    p0 = start(rs, B, N, D, "x")

    def run(tuning):
        fb = EnsembleBatch(B, N, D, mdl.fused("x"), moves=MOVES["mix"](), seeds=list(range(B)))
        for k, v in tuning.items():
            fb.set_tuning(k, v)
        fb.run_mcmc(p0, 30)
        out, info = dict(outputs(fb), blobs=fb.get_blobs(), last_blobs=fb.get_last_sample().blobs), fb.launch_info()
        fb.close()
        return out, info
    ref, info0 = run({})
    for key, field, values in (("batch_threads", "threads", (64, 640)), ("batch_plan_steps", "plan_steps", (1, 3))):
        for v in values:
            out, info = run({key: v})
            assert info[field] == v and info0[field] != v
            assert_equal_runs(ref, out)
    mdl.close()


# ---------------------------------------------------------------------------------------------------------------- 4. summary
@pytest.mark.parametrize("discard,thin", [(0, 1), (20, 3)])
def test_blob_summary_against_numpy(libs, discard, thin):
    """get_blob_summary against NumPy on get_blobs(): order statistics and the MAP blob exact, mean and covariance within the bounds
    of tests/test_gpu_batch_summary.py (|mean - fsum / n| <= n u sum|x| / n; |cov - np.cov| <= 8 n u sqrt(C_jj C_kk))"""
    B, N, D, nsteps = 3, 32, 5, 200
    rs = np.random.RandomState(60)
    mdl = Model(libs[D], B, D, 61)
    bt = EnsembleBatch(B, N, D, mdl.fused("g"), seeds=[100 + b for b in range(B)])
    bt.run_mcmc(rs.randn(B, N, D), nsteps)
    x = bt.get_blobs(discard=discard, thin=thin, flat=True)              # (B, n, K)
    lp = bt.get_log_prob(discard=discard, thin=thin, flat=True)
    n = x.shape[1]
    what = "discard=%d thin=%d n=%d" % (discard, thin, n)
    ranks = np.array([0, n - 1, n // 2, min(n // 2 + 1, n - 1), n // 2, n // 6] + np.random.RandomState(n).randint(0, n, size=9).tolist(),
                     dtype=np.int64)
    n_dev, mean, cov, order, mx, mlp = bt._summary_device(discard, thin, ranks, True, plane=4)
    xs = np.sort(x, axis=1)
    assert n_dev == n and np.array_equal(order, xs[:, ranks, :]), what                  # order statistics: exact
    quantiles = (0.16, 0.5, 0.84)
    s = bt.get_blob_summary(discard=discard, thin=thin, quantiles=quantiles)
    assert s.nsamples == n and s.mean.shape == (B, K) and s.cov.shape == (B, K, K) and s.quantiles.shape == (B, 3, K)
    assert np.array_equal(s.mean, mean) and np.array_equal(s.cov, cov) and np.array_equal(s.map_coords, mx) and np.array_equal(s.map_log_prob, mlp)
    lo, hi, g = summary.quantile_ranks(n, np.asarray(quantiles, dtype=np.float64))
    assert np.array_equal(s.quantiles, summary.lerp(xs[:, lo, :], xs[:, hi, :], g[None, :, None])), what
    for b in range(B):
        for d in range(K):
            col = x[b, :, d]
            exact = math.fsum(col) / n
            bound = n * U * math.fsum(np.abs(col)) / n
            print("%s: mean[%d, %d] err %.3g (bound %.3g)" % (what, b, d, abs(s.mean[b, d] - exact), bound))
            assert abs(s.mean[b, d] - exact) <= bound, (what, b, d, s.mean[b, d], exact, bound)
    assert np.array_equal(s.cov, s.cov.transpose(0, 2, 1)), what
    for b in range(B):
        Cm = np.atleast_2d(np.cov(x[b].T))
        sd = np.sqrt(np.diag(Cm))
        bound = 8 * n * U * np.outer(sd, sd)
        err = np.abs(s.cov[b] - Cm)
        print("%s: cov[%d] worst err / bound = %.3g" % (what, b, float((err / np.where(bound > 0, bound, 1.0)).max())))
        assert (err <= bound).all(), (what, b, err.max(), bound.min())
    for b in range(B):                                # the MAP entry: the blobs of the best stored sample, first in (row, walker) order
        at = int(np.argmax(lp[b]))
        assert s.map_log_prob[b] == lp[b, at] and np.array_equal(s.map_coords[b], x[b, at]), (what, b, at)
        assert s.map_coords[b, 0] == s.map_log_prob[b]
    m = bt[1].get_blob_summary(discard=discard, thin=thin)
    for u, v in zip(m[1:], s[1:]):
        assert np.array_equal(u, v[1])
    # the coordinates' summary is untouched by the plane selector
    sc = bt.get_summary(discard=discard, thin=thin)
    assert sc.mean.shape == (B, D) and np.array_equal(sc.map_log_prob, s.map_log_prob)
    bt.close()
    mdl.close()


# ---------------------------------------------------------------------------------------------------------------- 5. refusals
def test_a_member_that_fits_only_without_blobs_is_refused_not_launched():
    """600 x 16 under a StretchMove fits one workgroup's LDS without blobs and not with four of them (tests/test_batch_blobs_cpu.py
    has the arithmetic): refused by name at construction and at bind time, nothing launched"""
    with pytest.raises(ValueError) as e:
        EnsembleBatch(2, 600, 16, BatchFused(0x1000, 16, nblobs=4))
    assert "LDS" in str(e.value) and "4 blobs" in str(e.value)
    accept = _lib.FUSED_BATCH_FN(lambda launch: 0)      # a launcher that answers the probe and never launches
    fb = EnsembleBatch(2, 600, 16, BatchFused(accept, 16), seeds=[1, 2])
    h = fb._handle()                                  # without blobs the shape is taken
    lib = _lib.load()
    rc = lib.emx_set_batch_target_fused_blobs(h, accept, 16, None, 4)
    msg = lib.emx_batch_last_error(h)
    assert rc == -1 and b"LDS" in msg and b"4 blobs" in msg
    assert fb.launch_info()["launches"] == 0
    assert lib.emx_get_blobs_batch(h, None, None) == -1 and b"no blobs" in lib.emx_batch_last_error(h)
    fb.close()


def test_a_launcher_of_another_blob_count_is_refused_at_bind_time(libs):
    B, N, D = 3, 32, 5
    mdl = Model(libs[D], B, D, 12)
    ptr = libs[D].user_device_pointer(mdl.h)
    p0 = np.random.RandomState(0).randn(B, N, D)
    for launcher, nblobs in (("user_fused_g", 4), ("user_fused_g_blobs", 0), ("user_fused_g_blobs", 3)):
        fb = EnsembleBatch(B, N, D, BatchFused(getattr(libs[D], launcher), D, user=ptr, nblobs=nblobs), seeds=list(range(B)))
        with pytest.raises(_lib.EmxError) as e:
            fb.run_mcmc(p0, 10)
        assert "another number of blobs" in str(e.value) and fb.launch_info()["launches"] == 0
        fb.close()
    # tempering refuses a handle with blobs
    fb = EnsembleBatch(4, N, D, mdl.kernel("g"), seeds=list(range(4)))
    h = fb._handle()
    rc = _lib.load().emx_pt_set_tempering(h, 2, np.array([1.0, 0.5]), None, None)
    assert rc != 0 and b"blobs" in _lib.load().emx_batch_last_error(h)
    fb.close()
    mdl.close()
