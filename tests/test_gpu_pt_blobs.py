"""PTSampler with a likelihood that records blobs, on both paths: the batched callback (k_batch_cb's tempered commit with blobs, k_pt_swap
exchanging them) and the fused tempered kernel (k_pt_run<..., NBLOBS>).  tests/c/user_pt_fused_blobs.hip defines one diagonal-Gaussian
likelihood once and wraps it with and without blobs as PTFused functors and as BatchKernel block functions; the blobs are {L itself,
x[0] + x[1], x[0] * x[1], (double)member}, single correctly rounded operations, so every comparison below is bit for bit.  A blob
belongs to the point: it follows its walker through the tempered commit and through every accepted swap."""
import ctypes as C
import math
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from emcee_amd import PTSampler, _lib, moves, summary  # noqa: E402
from emcee_amd.targets import BatchCallable, BatchKernel, PTFused, get_include  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NDIMS = (3, 7, 16)
K = 4                        # USER_NBLOBS of the model file
U = 2.0 ** -53
SHAPES = [(3, 4, 32, 3),     # the smallest case
          (2, 3, 33, 7),     # odd walker count: the tail lanes of the pair loop and an uneven split
          (2, 8, 64, 16)]    # more rungs than waves' worth of rows: k_pt_run's chunked half-step
BOUND = 3.0                  # the prior functor's box, and the box prior's


def _compile_cmd(ndim, so, extra=()):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return ([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DUSER_NDIM=%d" % ndim] +
            list(extra) + ["-I" + d for d in get_include()] + [os.path.join(HERE, "c", "user_pt_fused_blobs.hip"), "-o", so])


def _load(so):
    _lib.load()                                  # one HIP runtime per process: the library's (torch's) first
    user = C.CDLL(so)
    user.user_setup.restype = C.c_void_p
    user.user_setup.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double]
    user.user_device_pointer.restype = C.c_void_p
    user.user_device_pointer.argtypes = [C.c_void_p]
    user.user_teardown.argtypes = [C.c_void_p]
    return user


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    """one library per ndim (every wrapping), and one at ndim 3 built against another EMX_FUSED_PT_ABI ("wrong"), side by side"""
    d = tmp_path_factory.mktemp("user_pt_fused_blobs")
    t0 = time.time()
    procs = {}
    for n in NDIMS + ("wrong",):
        so = str(d / ("libuser_pt_fused_blobs_%s.so" % n))
        cmd = _compile_cmd(3, so, ["-DEMX_FUSED_PT_ABI=4242u"]) if n == "wrong" else _compile_cmd(n, so)
        procs[n] = (so, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    out = {}
    for n, (so, p) in procs.items():
        _, err = p.communicate(timeout=1200)
        assert p.returncode == 0, err[-4000:]
        out[n] = _load(so)
    print("user_pt_fused_blobs.hip at ndim %s and one other ABI: %.1f s" % (list(NDIMS), time.time() - t0))
    return out


class Model(object):
    """the data of `members` = nbatch * ntemps members on the device, and the likelihood in each of its wrappings"""

    def __init__(self, user, members, D, seed):
        rs = np.random.RandomState(seed)
        self.user, self.D = user, D
        self.mu = np.ascontiguousarray(0.1 * rs.randn(members, D))
        self.ivar = np.ascontiguousarray(1.0 / (0.2 + rs.rand(members, D)))
        self.h = user.user_setup(self.mu.ctypes.data, self.ivar.ctypes.data, members, D, BOUND)
        assert self.h

    def kernel(self, blobs):
        return BatchKernel(self.user.user_block_g_blobs, self.h, nblobs=K) if blobs else BatchKernel(self.user.user_block_g, self.h)

    def prior_kernel(self):
        return BatchKernel(self.user.user_block_p, self.h)

    def fused(self, blobs, prior=False, nblobs=None):
        name = "pt_fused_g" + ("p" if prior else "") + ("_blobs" if blobs else "")
        return PTFused(getattr(self.user, name), self.D, user=self.user.user_device_pointer(self.h),
                       nblobs=(K if blobs else 0) if nblobs is None else nblobs)

    def close(self):
        self.user.user_teardown(self.h)


MOVES = {
    "stretch": lambda: moves.StretchMove(),
    "de_snooker": lambda: [(moves.DEMove(), 0.8), (moves.DESnookerMove(), 0.2)],
}


def make(libs, shape, path, blobs, prior, mv, seed, mdl=None, **kw):
    """-> (sampler, model): `path` "fused" / "kernel"; `prior` "none" / "box" / "functor" (a BatchKernel prior on the callback path)"""
    G, T, N, D = shape
    mdl = mdl or Model(libs[D], G * T, D, seed + 1)
    kw = dict(dict(nbatch=G, moves=MOVES[mv](), seeds=[seed + 10 * g for g in range(G)], blobs=bool(blobs)), **kw)
    box = (-BOUND * np.ones(D), BOUND * np.ones(D))
    if path == "fused":
        like, lp = mdl.fused(blobs, prior == "functor"), (box if prior == "box" else None)
    else:
        like, lp = mdl.kernel(blobs), (box if prior == "box" else mdl.prior_kernel() if prior == "functor" else None)
    return PTSampler(T, N, D, like, log_prior=lp, **kw), mdl


def start(shape, seed, scale=0.5):
    """every walker inside |x| <= BOUND (6 sigma) unless a test widens it"""
    return scale * np.random.RandomState(seed).randn(*shape)


def outputs(pt, stored=True):
    """tests/test_gpu_pt_fused.py's outputs(): every array of a run but the blobs"""
    last = pt.get_last_sample()
    L, P = pt._pt_state()
    att, acc = pt._swap_counts()
    out = dict(coords=last.coords, last_log_prob=last.log_prob, L=L, P=P, ladder=pt.ladder, updates=np.array(pt.adaptation_updates),
               accepted=pt._b._accepted().reshape(L.shape), attempts=att, swaps=acc, step=np.array(pt._b._step))
    if stored:
        out.update(chain=pt.get_chain(), log_prob=pt.get_log_prob(), log_like=pt.get_log_likelihood(), betas=pt.get_betas())
    return out


def blob_outputs(pt, stored=True):
    out = dict(last_blobs=pt.get_last_sample().blobs, state_blobs=pt._pt_blobs())
    if stored:
        out["blobs"] = pt.get_blobs()
    return out


def assert_equal_runs(x, y):
    assert sorted(x) == sorted(y)
    for k in x:
        assert x[k].shape == y[k].shape and np.array_equal(x[k], y[k], equal_nan=True), k


def members_of(shape):
    G, T, N, D = shape
    return (np.arange(G)[:, None] * T + np.arange(T)[None, :]).astype(np.float64)          # (G, T)


def check_blobs_follow_the_chain(pt, shape):
    """the stored blobs against the stored chain and L, and the last sample's against the last stored row"""
    G, T, N, D = shape
    bl, x, L = pt.get_blobs(), pt.get_chain(), pt.get_log_likelihood()
    assert bl.shape == x.shape[:4] + (K,) and bl.dtype == np.float64
    assert np.array_equal(bl[..., 0], L)
    assert np.array_equal(bl[..., 1], x[..., 0] + x[..., 1])
    assert np.array_equal(bl[..., 2], x[..., 0] * x[..., 1])
    lo = (np.arange(G) * T)[:, None, None, None]
    assert np.all((bl[..., 3] >= lo) & (bl[..., 3] < lo + T)) and np.array_equal(bl[..., 3], np.round(bl[..., 3]))
    last = pt.get_last_sample()
    assert last.blobs.shape == (G, T, N, K) and np.array_equal(last.blobs, bl[:, :, -1]) and np.array_equal(last.blobs, pt._pt_blobs())
    flat = pt.get_blobs(discard=3, thin=2, flat=True)
    assert np.array_equal(flat, bl[:, :, 4::2].reshape(G, T, -1, K))
    return bl


# ---------------------------------------------------------------------------------------------------------------- 1. through swaps
@pytest.mark.parametrize("path", ["kernel", "fused"])
@pytest.mark.parametrize("mv", sorted(MOVES))
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_blobs_follow_the_chain_through_swaps(libs, shape, mv, path):
    G, T, N, D = shape
    seed = 100 * G + 7 * T + N + D
    pt, mdl = make(libs, shape, path, True, "none", mv, seed, swap_every=1)
    assert pt.nblobs == K
    pt.run_mcmc(start(shape, seed), 30)
    bl = check_blobs_follow_the_chain(pt, shape)
    # the test says something about the swap only if swaps were accepted and moved a blob to another rung than the one that made it
    assert (pt.tswap_acceptance_fraction > 0).any()
    assert (bl[..., 3] != members_of(shape)[:, :, None, None]).any()
    pt.close()
    mdl.close()


@pytest.mark.parametrize("path", ["kernel", "fused"])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=["x".join(map(str, s)) for s in SHAPES[:2]])
def test_without_swaps_a_blob_names_its_own_member(libs, shape, path):
    seed = 5 + shape[2]
    pt, mdl = make(libs, shape, path, True, "none", "stretch", seed, swap_every=0)
    pt.run_mcmc(start(shape, seed), 20)
    bl = check_blobs_follow_the_chain(pt, shape)
    assert np.array_equal(bl[..., 3], np.broadcast_to(members_of(shape)[:, :, None, None], bl.shape[:4]))
    assert np.all(pt.tswap_acceptance_fraction == 0)
    pt.close()
    mdl.close()


# ---------------------------------------------------------------------------------------------------------------- 2. sampling unchanged
@pytest.mark.parametrize("shape,path,mv,prior,adaptive", [
    (SHAPES[0], "fused", "stretch", "box", False),
    (SHAPES[1], "kernel", "de_snooker", "none", False),
    (SHAPES[2], "fused", "de_snooker", "functor", True),
    (SHAPES[0], "kernel", "stretch", "functor", True),
    (SHAPES[1], "fused", "stretch", "none", False),
    (SHAPES[2], "kernel", "stretch", "box", False),
], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_sampling_is_that_of_the_functor_without_blobs(libs, shape, path, mv, prior, adaptive):
    seed = 31 + shape[2] + shape[3]
    kw = dict(swap_every=1, adaptive=adaptive, adaptation_lag=20, adaptation_time=2)
    with_blobs, mdl = make(libs, shape, path, True, prior, mv, seed, **kw)
    without, _ = make(libs, shape, path, False, prior, mv, seed, mdl=mdl, **kw)
    p0 = start(shape, seed)
    with_blobs.run_mcmc(p0, 30)
    without.run_mcmc(p0, 30)
    x = outputs(with_blobs)
    assert_equal_runs(x, outputs(without))
    assert x["swaps"].sum() > 0 and 0 < x["accepted"].sum()
    if adaptive:
        assert x["updates"] == 30 and not np.array_equal(x["ladder"], np.tile(with_blobs.betas, (shape[0], 1)))
    assert without.nblobs == 0 and without.get_blobs() is None and without.get_last_sample().blobs is None
    with pytest.raises(ValueError, match="no blobs"):
        without.get_blob_summary()
    check_blobs_follow_the_chain(with_blobs, shape)
    with_blobs.close()
    without.close()
    mdl.close()


# ---------------------------------------------------------------------------------------------------------------- 3. fused == callback
@pytest.mark.parametrize("shape,mv,prior,thin_by,how", [
    (SHAPES[0], "stretch", "box", 1, "one"),
    (SHAPES[1], "de_snooker", "functor", 3, "one"),
    (SHAPES[2], "stretch", "box", 1, "split"),
    (SHAPES[0], "de_snooker", "functor", 1, "unstored"),
    (SHAPES[2], "de_snooker", "none", 3, "split"),
    (SHAPES[1], "stretch", "box", 1, "unstored"),
], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_fused_equals_the_callback_path_blobs_included(libs, shape, mv, prior, thin_by, how):
    seed = 61 + shape[2] + thin_by
    f, mdl = make(libs, shape, "fused", True, prior, mv, seed, swap_every=1)
    k, _ = make(libs, shape, "kernel", True, prior, mv, seed, mdl=mdl, swap_every=1)
    p0 = start(shape, seed)
    n = 12
    for s in (f, k):
        if how == "one":
            s.run_mcmc(p0, 2 * n, thin_by=thin_by)
        elif how == "split":
            s.run_mcmc(p0, n, thin_by=thin_by)
            s.run_mcmc(None, n, thin_by=thin_by)
        else:
            s.run_mcmc(p0, 2 * n, thin_by=thin_by, store=False)
    stored = how != "unstored"
    x = outputs(f, stored)
    assert_equal_runs(x, outputs(k, stored))
    bx, by = blob_outputs(f, stored), blob_outputs(k, stored)
    assert_equal_runs(bx, by)
    assert x["swaps"].sum() > 0 and x["step"] == 2 * n * thin_by
    assert np.array_equal(bx["last_blobs"][..., 0], x["L"]) and np.array_equal(bx["last_blobs"][..., 1], x["coords"][..., 0] + x["coords"][..., 1])
    if stored:
        assert bx["blobs"].shape == shape[:2] + (2 * n, shape[2], K)
        check_blobs_follow_the_chain(f, shape)
    f.close()
    k.close()
    mdl.close()


# ---------------------------------------------------------------------------------------------------------------- 4. the swap pass alone
def swap_draws(seed, step, N, T):
    perm = np.zeros((T - 1, N), dtype=np.int32)
    logu = np.zeros((T - 1, N))
    assert _lib.load().emx_host_pt_swap_draws(int(seed), int(step), N, T, perm, logu) == 0
    return perm, logu


def swap_oracle(X, L, P, Bl, betas, seeds, step):
    """tests/test_gpu_pt.py's swap oracle (ptemcee's pass on (G, T, N, ...) arrays with the library's draws) carrying a blob array with
    X, L and P; -> (X, L, P, Bl, accepts (G, T - 1))"""
    X, L, P, Bl = X.copy(), L.copy(), P.copy(), Bl.copy()
    G, T, N = L.shape
    acc = np.zeros((G, T - 1), dtype=np.uint64)
    for g in range(G):
        perm, logu = swap_draws(seeds[g], step, N, T)
        for i in range(T - 1, 0, -1):
            j = perm[i - 1]
            with np.errstate(invalid="ignore"):
                ok = (betas[i - 1] - betas[i]) * (L[g, i] - L[g, i - 1, j]) > logu[i - 1]
            k = np.flatnonzero(ok)
            jk = j[k]
            for A in (X, L, P, Bl):
                hot, cold = A[g, i, k].copy(), A[g, i - 1, jk].copy()
                A[g, i, k], A[g, i - 1, jk] = cold, hot
            acc[g, i - 1] = len(k)
    return X, L, P, Bl, acc


@pytest.mark.parametrize("path", ["kernel", "fused"])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=["x".join(map(str, s)) for s in SHAPES[:2]])
def test_the_swap_pass_alone_against_the_numpy_oracle(libs, shape, path):
    """The initial state's blobs (run_mcmc(p0, 0)) against NumPy, then one swap pass (emx_pt_swap) against the oracle.  The pass uses the
    draws of the last step taken, so one unstored step without swaps stands between the two (emx_pt_swap refuses a handle at step 0)."""
    G, T, N, D = shape
    seed = 81 + N
    pt, mdl = make(libs, shape, path, True, "box", "stretch", seed, swap_every=0)
    p0 = start(shape, seed)
    pt.run_mcmc(p0, 0)
    L0, P0 = pt._pt_state()
    b0 = pt._pt_blobs()
    assert np.array_equal(P0, np.zeros_like(P0)) and np.array_equal(b0[..., 0], L0)
    assert np.array_equal(b0[..., 1], p0[..., 0] + p0[..., 1]) and np.array_equal(b0[..., 2], p0[..., 0] * p0[..., 1])
    assert np.array_equal(b0[..., 3], np.broadcast_to(members_of(shape)[:, :, None], b0.shape[:3]))
    pt.run_mcmc(None, 1, store=False)
    X = pt.get_last_sample().coords
    L, P = pt._pt_state()
    Bl = np.empty((G, T, N, K))
    assert _lib.load().emx_pt_get_blobs(pt._h, Bl) == 0
    before = pt._swap_counts()
    pt._swap()
    seeds = [int(pt._b._philox[g * T]) for g in range(G)]
    wX, wL, wP, wB, wacc = swap_oracle(X, L, P, Bl, pt.betas, seeds, pt._b._step - 1)
    got = pt.get_last_sample()
    gL, gP = pt._pt_state()
    gB = np.empty((G, T, N, K))
    assert _lib.load().emx_pt_get_blobs(pt._h, gB) == 0
    assert np.array_equal(got.coords, wX) and np.array_equal(gL, wL) and np.array_equal(gP, wP)
    assert np.array_equal(gB, wB) and np.array_equal(got.blobs, wB)
    att, acc = pt._swap_counts()
    assert np.array_equal(acc - before[1], wacc) and wacc.sum() > 0 and np.array_equal(att - before[0], np.full((G, T - 1), N, dtype=np.uint64))
    assert 0 < (gB[..., 3] != members_of(shape)[:, :, None]).sum() <= 2 * wacc.sum()      # an accepted swap moves two blobs to another rung
    assert np.array_equal(gB[..., 0], gL) and np.array_equal(gB[..., 1], wX[..., 0] + wX[..., 1])
    # emx_pt_set_state bypasses the likelihood: the blobs become NaN
    pt._set_pt_state(X.reshape(G * T, N, D), L.reshape(G * T, N), P.reshape(G * T, N))
    assert np.isnan(pt._pt_blobs()).all() and np.array_equal(pt._pt_state()[0], L)
    pt.close()
    mdl.close()


# ---------------------------------------------------------------------------------------------------------------- 5. a torch callable
@pytest.mark.parametrize("mv", sorted(MOVES))
def test_a_torch_batch_callable_with_blobs(mv):
    shape = G, T, N, D = SHAPES[0]
    rs = np.random.RandomState(91)
    mu = torch.as_tensor(0.1 * rs.randn(G, T, 1, D), device="cuda")
    ivar = torch.as_tensor(1.0 / (0.2 + rs.rand(G, T, 1, D)), device="cuda")
    member = torch.as_tensor(members_of(shape), device="cuda")[:, :, None]
    seen = []

    def fn(q):                                       # (G, T, R, D) -> (G, T, R), (G, T, R, K)
        seen.append(tuple(q.shape))
        acc = torch.zeros(q.shape[:3], dtype=torch.float64, device=q.device)
        for d in range(D):
            r = q[..., d] - mu[..., d]
            acc = acc + ivar[..., d] * r * r
        L = -0.5 * acc
        return L, torch.stack([L, q[..., 0] + q[..., 1], q[..., 0] * q[..., 1], member.expand_as(L)], dim=-1)
    box = (-BOUND * np.ones(D), BOUND * np.ones(D))
    pt = PTSampler(T, N, D, BatchCallable(fn, nblobs=K), log_prior=box, nbatch=G, moves=MOVES[mv](), seeds=[3, 4, 5], swap_every=1,
                   blobs=True)
    assert pt.nblobs == K
    pt.run_mcmc(start(shape, 92), 25)
    assert seen and all(s[:2] == (G, T) and s[3] == D for s in seen)
    bl = check_blobs_follow_the_chain(pt, shape)
    assert (pt.tswap_acceptance_fraction > 0).any() and (bl[..., 3] != members_of(shape)[:, :, None, None]).any()
    pt.close()
    # a callable that returns blobs of another shape is the caller's error, raised as itself
    bad = PTSampler(T, N, D, BatchCallable(lambda q: (fn(q)[0], fn(q)[1][..., :2]), nblobs=K), nbatch=G, seeds=[3, 4, 5], blobs=True)
    with pytest.raises(ValueError, match="blobs of shape"):
        bad.run_mcmc(start(shape, 92), 1)
    bad.close()


# ---------------------------------------------------------------------------------------------------------------- 6. outside the box
def test_initial_walkers_outside_the_box_have_nan_blobs_until_they_move(libs):
    shape = G, T, N, D = SHAPES[0]
    p0 = start(shape, 6, scale=2.0)                  # the box is |x| <= 3: some walkers start outside (P = -inf)
    outside = ~((p0 >= -BOUND) & (p0 <= BOUND)).all(-1)
    assert 0 < outside.sum() < outside.size
    runs = {}
    for path in ("fused", "kernel"):
        for every in (0, 1):
            pt, mdl = make(libs, shape, path, True, "box", "stretch", 7, swap_every=every)
            pt.run_mcmc(p0, 0)
            L, P = pt._pt_state()
            b0 = pt.get_last_sample().blobs
            assert np.array_equal(np.isneginf(P), outside) and np.array_equal(np.isneginf(L), outside)
            assert np.array_equal(np.isnan(b0), np.broadcast_to(outside[..., None], b0.shape))          # NaN exactly there, every blob
            assert np.array_equal(b0[~outside][:, 0], L[~outside])
            pt.run_mcmc(None, 40)
            bl, LL, x = pt.get_blobs(), pt.get_log_likelihood(), pt.get_chain()
            # a stored row holds NaN blobs exactly where it still holds a point outside the prior (L = -inf), every blob alike
            assert np.array_equal(np.isnan(bl), np.broadcast_to(np.isneginf(LL)[..., None], bl.shape))
            ok = ~np.isneginf(LL)
            assert np.array_equal(bl[..., 0][ok], LL[ok]) and np.array_equal(bl[..., 1][ok], (x[..., 0] + x[..., 1])[ok])
            if every == 0:
                # without swaps a walker keeps its NaN blobs exactly until its first accepted move
                moved = np.maximum.accumulate((x != p0[:, :, None]).any(-1), axis=2)          # (G, T, steps, N)
                o = np.broadcast_to(outside[:, :, None], moved.shape)
                assert np.array_equal(np.isnan(bl[..., 0])[o], ~moved[o])
                assert moved[o].any()
            runs[path, every] = dict(outputs(pt), **blob_outputs(pt))
            pt.close()
            mdl.close()
    for every in (0, 1):
        assert_equal_runs(runs["fused", every], runs["kernel", every])


# ---------------------------------------------------------------------------------------------------------------- 7. summaries
@pytest.fixture(scope="module")
def summarised(libs):
    shape = SHAPES[0]
    pt, mdl = make(libs, shape, "fused", True, "box", "stretch", 71, swap_every=1)
    pt.run_mcmc(start(shape, 72), 55)
    yield pt, shape
    pt.close()
    mdl.close()


@pytest.mark.parametrize("discard,thin", [(0, 1), (7, 3)])
def test_blob_summary_against_numpy(summarised, discard, thin):
    """get_blob_summary against NumPy on get_blobs(), with tests/test_gpu_batch_blobs.py's assertions: order statistics, the MAP blob and
    the counts exact; |mean - fsum / n| <= n u sum|x| / n; |cov - np.cov| <= 8 n u sqrt(C_jj C_kk)"""
    pt, (G, T, N, D) = summarised
    M = G * T
    x = pt.get_blobs(discard=discard, thin=thin, flat=True).reshape(M, -1, K)
    lp = pt.get_log_prob(discard=discard, thin=thin, flat=True).reshape(M, -1)
    n = x.shape[1]
    what = "discard=%d thin=%d n=%d" % (discard, thin, n)
    ranks = np.array([0, n - 1, n // 2, min(n // 2 + 1, n - 1), n // 2, n // 6] + np.random.RandomState(n).randint(0, n, size=9).tolist(),
                     dtype=np.int64)
    n_dev, mean, cov, order, mx, mlp = pt._b._summary_device(discard, thin, ranks, True, plane=4)
    xs = np.sort(x, axis=1)
    assert n_dev == n and np.array_equal(order, xs[:, ranks, :]), what                  # order statistics: exact
    quantiles = (0.16, 0.5, 0.84)
    s = pt.get_blob_summary(discard=discard, thin=thin, quantiles=quantiles)
    assert s.nsamples == n and s.mean.shape == (G, T, K) and s.cov.shape == (G, T, K, K) and s.quantiles.shape == (G, T, 3, K)
    assert s.map_coords.shape == (G, T, K) and s.map_log_prob.shape == (G, T)
    flat = (lambda a: a.reshape((M,) + a.shape[2:]))
    assert np.array_equal(flat(s.mean), mean) and np.array_equal(flat(s.cov), cov) and np.array_equal(flat(s.map_coords), mx)
    assert np.array_equal(flat(s.map_log_prob), mlp)
    lo, hi, g = summary.quantile_ranks(n, np.asarray(quantiles, dtype=np.float64))
    assert np.array_equal(flat(s.quantiles), summary.lerp(xs[:, lo, :], xs[:, hi, :], g[None, :, None])), what
    for b in range(M):
        for d in range(K):
            col = x[b, :, d]
            exact = math.fsum(col) / n
            bound = n * U * math.fsum(np.abs(col)) / n
            print("%s: mean[%d, %d] err %.3g (bound %.3g)" % (what, b, d, abs(mean[b, d] - exact), bound))
            assert abs(mean[b, d] - exact) <= bound, (what, b, d, mean[b, d], exact, bound)
    assert np.array_equal(cov, cov.transpose(0, 2, 1)), what
    for b in range(M):
        Cm = np.atleast_2d(np.cov(x[b].T))
        sd = np.sqrt(np.diag(Cm))
        bound = 8 * n * U * np.outer(sd, sd)
        err = np.abs(cov[b] - Cm)
        print("%s: cov[%d] worst err / bound = %.3g" % (what, b, float((err / np.where(bound > 0, bound, 1.0)).max())))
        assert (err <= bound).all(), (what, b, err.max(), bound.min())
    for b in range(M):                                # the MAP entry: the blobs of the best stored sample, first in (row, walker) order
        at = int(np.argmax(lp[b]))
        assert mlp[b] == lp[b, at] and np.array_equal(mx[b], x[b, at]), (what, b, at)
    # the coordinates' summary is untouched by the plane selector
    c = pt.get_summary(discard=discard, thin=thin)
    assert c.mean.shape == (G, T, D) and np.array_equal(c.map_log_prob, s.map_log_prob)


def test_blob_histograms_against_numpy(summarised):
    """get_blob_histograms against np.histogram / np.histogram2d on get_blobs(), count for count, rung by rung"""
    pt, (G, T, N, D) = summarised
    x = pt.get_blobs(discard=5, thin=2, flat=True)                          # (G, T, n, K)
    n = x.shape[2]
    rng = [(-12.0, 0.0), (-4.0, 4.0), (-3.0, 3.0), (-0.5, G * T - 0.5)]
    r = pt.get_blob_histograms(bins=24, range=rng, discard=5, thin=2, pairs=[(0, 1), (3, 2)], pair_bins=12)
    assert r.nsamples == n == 25 * N
    assert all(a.shape == (G, T, 25) for a in r.edges) and all(a.shape == (G, T, 24) for a in r.counts)
    assert [p.shape for p in r.pair_counts] == [(G, T, 12, 12)] * 2
    for o in range(G):
        for t in range(T):
            for d in range(K):
                ref, e = np.histogram(x[o, t, :, d], bins=24, range=rng[d])
                assert np.array_equal(r.counts[d][o, t], ref) and np.array_equal(r.edges[d][o, t], e), (o, t, d)
            for p, (i, j) in enumerate([(0, 1), (3, 2)]):
                ref, _, _ = np.histogram2d(x[o, t, :, i], x[o, t, :, j], bins=12, range=[rng[i], rng[j]])
                assert np.array_equal(r.pair_counts[p][o, t], ref.astype(np.int64)), (o, t, i, j)
    auto = pt.get_blob_histograms(bins=10, discard=5, thin=2, pairs=None)              # every rung's own minimum and maximum
    for d in range(K):
        assert np.array_equal(auto.edges[d][..., 0], x[..., d].min(axis=2)) and np.array_equal(auto.edges[d][..., -1], x[..., d].max(axis=2))
        assert np.all(auto.counts[d].sum(axis=-1) == n)
    own = np.zeros((G, T, K, 2)) + [-5.0, 5.0]
    own[1, 2] = [-50.0, 50.0]
    q = pt.get_blob_histograms(bins=9, range=own, pairs=None)
    ref, e = np.histogram(pt.get_blobs()[1, 2, :, :, 0].ravel(), bins=9, range=(-50.0, 50.0))
    assert np.array_equal(q.counts[0][1, 2], ref) and np.array_equal(q.edges[0][1, 2], e)
    check = pt.get_histograms(bins=12, discard=5, thin=2, pairs=None)                  # the coordinates' plane is untouched
    assert all(a.shape == (G, T, 12) for a in check.counts) and len(check.counts) == D


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
def test_a_launcher_of_another_blob_count_is_refused_at_bind_time(libs):
    G, T, N, D = SHAPES[0]
    mdl = Model(libs[D], G * T, D, 81)
    p0 = start(SHAPES[0], 82)
    for blobs, nblobs in ((True, 2), (True, 0), (False, K)):      # the launcher's NBLOBS is K, K, 0
        pt = PTSampler(T, N, D, mdl.fused(blobs, nblobs=nblobs), nbatch=G, seeds=[1, 2, 3], blobs=nblobs > 0)
        with pytest.raises(_lib.EmxError) as e:
            pt.run_mcmc(p0, 10)
        assert "another number of blobs" in str(e.value) and "the %d asked for" % nblobs in str(e.value)
        assert pt.launch_info()["launches"] == 0
        pt.close()
    mdl.close()


def test_a_blob_launcher_of_another_header_version_is_refused_at_bind_time(libs):
    G, T, N, D = SHAPES[0]
    mdl = Model(libs["wrong"], G * T, D, 83)
    for blobs in (True, False):
        pt = PTSampler(T, N, D, mdl.fused(blobs), nbatch=G, seeds=[1, 2, 3], blobs=blobs)
        with pytest.raises(_lib.EmxError) as e:
            pt.run_mcmc(start(SHAPES[0], 84), 10)
        assert "another version of emx_pt_fused.hpp" in str(e.value)
        assert pt.launch_info()["launches"] == 0
        pt.close()
    mdl.close()


def test_a_shape_that_fits_only_without_blobs_is_refused_before_any_launch():
    lib = _lib.load()
    T, D = 8, 16
    msg = C.create_string_buffer(512)
    arr = (_lib.MoveDesc * 1)(moves.StretchMove()._desc(D))
    fits = [n for n in range(2 * D, 1024, 2) if lib.emx_pt_fused_check(T, n, D, 1, arr, msg, 512) == 0]
    N = max(fits)
    assert lib.emx_pt_fused_check(T, N + 2, D, 1, arr, msg, 512) == -1 and N > 2 * D
    assert lib.emx_pt_fused_check_blobs(T, N, D, 1, arr, 0, msg, 512) == 0
    assert lib.emx_pt_fused_check_blobs(T, N, D, 1, arr, 8, msg, 512) == -1
    assert b"LDS" in msg.value and b"8 blobs" in msg.value
    PTSampler(T, N, D, PTFused(0x1000, D), moves=moves.StretchMove())                # constructs: the blob-free object fits
    with pytest.raises(ValueError) as e:
        PTSampler(T, N, D, PTFused(0x1000, D, nblobs=8), moves=moves.StretchMove(), blobs=True)
    assert "LDS" in str(e.value) and "8 blobs" in str(e.value)
