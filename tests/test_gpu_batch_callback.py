"""EnsembleBatch with the user's batched log-probability (targets.BatchCallable / BatchKernel).  Every member must be bit for bit the
single Philox-mode EnsembleSampler with DeviceCallable of the function restricted to that member; the blocks the function
receives, the launch count, the launch shape, chunking and the error paths are checked against that contract."""
import ctypes as C
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from emcee_amd import EnsembleBatch, EnsembleSampler, _lib, moves  # noqa: E402
from emcee_amd.ensemble import philox_seed  # noqa: E402
from emcee_amd.targets import BatchCallable, BatchKernel, DeviceCallable  # noqa: E402

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- helpers
def gauss_params(rs, B, D):
    return 0.1 * rs.randn(B, D), 1.0 / (0.2 + rs.rand(B, D))


def batched_fn(mu, ivar):
    """(B, n, D) -> (B, n): per-member diagonal Gaussian, element-wise ops in a fixed loop over the coordinates (no reduction
    whose association could depend on the block's shape)"""
    mu_t = torch.as_tensor(mu, device="cuda")[:, None, :]
    iv_t = torch.as_tensor(ivar, device="cuda")[:, None, :]
    D = mu.shape[1]

    def fn(q):
        acc = torch.zeros(q.shape[:2], dtype=torch.float64, device=q.device)
        for d in range(D):
            r = q[:, :, d] - mu_t[:, :, d]
            acc = acc + iv_t[:, :, d] * r * r
        return -0.5 * acc
    return fn


def member_fn(mu, ivar, b):
    """the batched function restricted to member b: (n, D) -> (n), the same element-wise ops"""
    mu_t = torch.as_tensor(mu[b], device="cuda")[None, :]
    iv_t = torch.as_tensor(ivar[b], device="cuda")[None, :]
    D = mu.shape[1]

    def fn(q):
        acc = torch.zeros(q.shape[:1], dtype=torch.float64, device=q.device)
        for d in range(D):
            r = q[:, d] - mu_t[:, d]
            acc = acc + iv_t[:, d] * r * r
        return -0.5 * acc
    return fn


def single(N, D, fn_b, move_factory, seed, p0, nsteps, thin_by=1, store=True, skip=False, chunks=None):
    s = EnsembleSampler(N, D, DeviceCallable(fn_b), moves=move_factory(), rng="philox")
    s.random_state = np.random.RandomState(seed).get_state()
    if chunks is None:
        s.final = s.run_mcmc(p0, nsteps, thin_by=thin_by, store=store, skip_initial_state_check=skip)
    else:
        s.final = s.run_mcmc(p0, chunks[0], thin_by=thin_by, store=store, skip_initial_state_check=skip)
        for n in chunks[1:]:
            s.final = s.run_mcmc(None, n, thin_by=thin_by, store=store, skip_initial_state_check=skip)
    return s


def assert_member_equal(batch, b, s, store=True):
    last, ref = batch.get_last_sample(), s.final
    assert np.array_equal(last.coords[b], ref.coords), "member %d: final coordinates" % b
    assert np.array_equal(last.log_prob[b], ref.log_prob), "member %d: final log-probs" % b
    assert batch._step == s._philox_step, "member %d: Philox step" % b
    if store:
        assert batch.iteration == s.iteration
        assert np.array_equal(batch[b].get_chain(), s.get_chain()), "member %d: chain" % b
        assert np.array_equal(batch[b].get_log_prob(), s.get_log_prob()), "member %d: log-prob chain" % b
        assert np.array_equal(batch[b].acceptance_fraction, s.acceptance_fraction), "member %d: accept counts" % b


def members_to_check(B):
    return list(range(B)) if B <= 8 else sorted({0, 1, B // 3, B // 2, B - 2, B - 1})


def outputs(batch):
    return (batch.get_chain(), batch.get_log_prob(), batch.acceptance_fraction, batch.get_last_sample().coords,
            batch.get_last_sample().log_prob)


def assert_outputs_equal(x, y):
    for u, v in zip(x, y):
        assert np.array_equal(u, v)


def splits_of(mv):
    return 1 if isinstance(mv, moves.GaussianMove) else mv.nsplits


def member_splits(seed, step, move_list, weights):
    """the split count of the move member `seed` draws at Philox `step` (the host twin of the kernels' move choice)"""
    if len(move_list) == 1:
        return splits_of(move_list[0])
    cdf = np.cumsum(np.asarray(weights, dtype=np.float64))
    cdf /= cdf[-1]
    k = _lib.load().emx_host_move_choice_philox(philox_seed(np.random.RandomState(seed)), step, np.ascontiguousarray(cdf), len(cdf))
    return splits_of(move_list[k])


def split_size(N, S, k):
    return (N - k + S - 1) // S if k < S else 0


stretch = lambda: moves.StretchMove()  # noqa: E731
de_snooker = lambda: [(moves.DEMove(), 0.8), (moves.DESnookerMove(), 0.2)]  # noqa: E731

CASES = {
    # name: (N, D, moves, B, skip the conditioning check)
    "stretch_32x5": (32, 5, stretch, 3, False),
    "stretch3_45x2": (45, 2, lambda: moves.StretchMove(nsplits=3), 3, False),
    "stretch3_46x2_padding": (46, 2, lambda: moves.StretchMove(nsplits=3), 3, False),
    "de_66x7": (66, 7, lambda: moves.DEMove(), 3, False),
    "snooker_50x3": (50, 3, lambda: moves.DESnookerMove(), 3, False),
    "de_snooker_100x10": (100, 10, de_snooker, 3, False),
    "mix_32x5": (32, 5, lambda: [(moves.StretchMove(), 0.5), (moves.DEMove(), 0.3), (moves.DESnookerMove(), 0.2)], 3, False),
    "gauss_vector": (32, 4, lambda: moves.GaussianMove(0.3), 3, False),
    "gauss_random_factor": (32, 4, lambda: moves.GaussianMove([0.5, 0.3, 0.4, 0.2], mode="random", factor=2.0), 3, False),
    "gauss_sequential": (32, 4, lambda: moves.GaussianMove(0.5, mode="sequential"), 3, False),
    "ndim1_32x1": (32, 1, stretch, 3, False),
    "ndim130_40x130": (40, 130, lambda: moves.StretchMove(nsplits=5, live_dangerously=True), 2, True),
    "nwalkers2_2x1": (2, 1, stretch, 3, True),
    "nwalkers1024_1024x8": (1024, 8, stretch, 2, False),
    "stretch_32x5_B1": (32, 5, stretch, 1, False),
    "stretch_32x5_B37": (32, 5, stretch, 37, False),
    "mix_32x5_B300": (32, 5, lambda: [moves.StretchMove(), moves.DEMove()], 300, False),
}


# ---------------------------------------------------------------------------------------------------------------- 1. members
@pytest.mark.parametrize("name", sorted(CASES))
def test_members_equal_single_sampler(name):
    N, D, mf, B, skip = CASES[name]
    rs = np.random.RandomState(len(name))
    mu, ivar = gauss_params(rs, B, D)
    p0 = rs.randn(B, N, D)
    seeds = [1000 + 17 * b for b in range(B)]
    nsteps = 8 if D > 100 else 20
    batch = EnsembleBatch(B, N, D, BatchCallable(batched_fn(mu, ivar)), moves=mf(), seeds=seeds)
    batch.run_mcmc(p0, nsteps, skip_initial_state_check=skip)
    for b in members_to_check(B):
        s = single(N, D, member_fn(mu, ivar, b), mf, seeds[b], p0[b], nsteps, skip=skip)
        assert_member_equal(batch, b, s)
    batch.close()


# ---------------------------------------------------------------------------------------------------------------- 2. blocks
def test_blocks_handed_to_the_function():
    B, N, D, nsteps = 3, 50, 3, 3
    rs = np.random.RandomState(5)
    mu, ivar = gauss_params(rs, B, D)
    p0 = rs.randn(B, N, D)
    seeds = [21, 22, 23]
    fn = batched_fn(mu, ivar)
    calls = []

    def recording(q):
        calls.append((tuple(q.shape), q.dtype, q.is_cuda, q.is_contiguous(), q.clone()))
        return fn(q)
    batch = EnsembleBatch(B, N, D, BatchCallable(recording), moves=de_snooker(), seeds=seeds)
    batch.run_mcmc(p0, nsteps)
    smax, R = 4, 25
    assert len(calls) == 1 + nsteps * smax
    assert calls[0][0] == (B, N, D) and np.array_equal(calls[0][4].cpu().numpy(), p0)
    for shape, dtype, cuda, contig, _ in calls[1:]:
        assert shape == (B, R, D) and dtype == torch.float64 and cuda and contig
    chain = batch.get_chain()
    move_list = [m for m, _ in de_snooker()]
    for b in range(B):
        got = []

        def rec_b(q, f=member_fn(mu, ivar, b)):
            got.append(q.clone().cpu().numpy())
            return f(q)
        single(N, D, rec_b, de_snooker, seeds[b], p0[b], nsteps)
        assert np.array_equal(got[0], p0[b])
        it = 1
        for s in range(nsteps):
            S = member_splits(seeds[b], s, move_list, [0.8, 0.2])
            prev, cur = (p0[b] if s == 0 else chain[b, s - 1]), chain[b, s]
            for k in range(smax):
                q = calls[1 + s * smax + k][4][b].cpu().numpy()
                n = split_size(N, S, k)
                if n:
                    assert np.array_equal(q[:n], got[it]), (b, s, k)
                    it += 1
                pad = q[n:]
                assert np.all(np.isfinite(pad))
                rows = np.arange(n, R)
                assert np.all((pad == prev[rows]).all(1) | (pad == cur[rows]).all(1)), (b, s, k)
        assert it == len(got)


def test_nan_on_padding_rows_changes_nothing():
    B, N, D, nsteps = 4, 50, 3, 6
    rs = np.random.RandomState(8)
    mu, ivar = gauss_params(rs, B, D)
    p0 = rs.randn(B, N, D)
    seeds = [3, 4, 5, 6]
    fn = batched_fn(mu, ivar)
    move_list, smax = [moves.DEMove(), moves.DESnookerMove()], 4
    count = [0]

    def nan_on_padding(q):
        out = fn(q)
        c = count[0]
        count[0] += 1
        if c > 0:
            s, k = divmod(c - 1, smax)
            for b in range(B):
                n = split_size(N, member_splits(seeds[b], s, move_list, [0.8, 0.2]), k)
                out[b, n:] = float("nan")
        return out
    clean = EnsembleBatch(B, N, D, BatchCallable(fn), moves=de_snooker(), seeds=seeds)
    clean.run_mcmc(p0, nsteps)
    padded = EnsembleBatch(B, N, D, BatchCallable(nan_on_padding), moves=de_snooker(), seeds=seeds)
    padded.run_mcmc(p0, nsteps)
    assert count[0] == 1 + nsteps * smax
    assert_outputs_equal(outputs(clean), outputs(padded))


# ---------------------------------------------------------------------------------------------------------------- 3. launches
def test_launches_do_not_grow_with_the_batch():
    N, D, nsteps, thin_by = 32, 5, 5, 2
    got = []
    for B in (16, 1024):
        rs = np.random.RandomState(B)
        mu, ivar = gauss_params(rs, B, D)
        batch = EnsembleBatch(B, N, D, BatchCallable(batched_fn(mu, ivar)), moves=de_snooker(), seeds=list(range(B)))
        batch.run_mcmc(rs.randn(B, N, D), nsteps, thin_by=thin_by)
        got.append(batch.launch_info()["launches"])
        batch.close()
    assert got[0] == got[1] == 1 + (nsteps * thin_by * 4 + 1), got


# ---------------------------------------------------------------------------------------------------------------- 4. shape
def test_launch_shape_and_member_order_do_not_change_bits():
    B, N, D, nsteps = 6, 40, 6, 15
    rs = np.random.RandomState(9)
    mu, ivar = gauss_params(rs, B, D)
    p0 = rs.randn(B, N, D)
    seeds = list(range(70, 70 + B))
    mix = lambda: [(moves.StretchMove(), 0.5), (moves.DEMove(), 0.3), (moves.DESnookerMove(), 0.2)]  # noqa: E731
    outs, threads = [], []
    for t in (0, 64, 256):
        bt = EnsembleBatch(B, N, D, BatchCallable(batched_fn(mu, ivar)), moves=mix(), seeds=seeds)
        bt.set_tuning("batch_threads", t)
        bt.run_mcmc(p0, nsteps)
        threads.append(bt.launch_info()["threads"])
        outs.append(outputs(bt))
        bt.close()
    assert threads[1:] == [64, 256] and threads[0] > 0
    for o in outs[1:]:
        assert_outputs_equal(outs[0], o)
    perm = [3, 0, 5, 1, 4, 2]
    pb = EnsembleBatch(B, N, D, BatchCallable(batched_fn(mu[perm], ivar[perm])), moves=mix(), seeds=[seeds[k] for k in perm])
    pb.run_mcmc(p0[perm], nsteps)
    assert_outputs_equal([x[perm] for x in outs[0]], outputs(pb))


# ---------------------------------------------------------------------------------------------------------------- 5. chunks
def test_chunking_resume_thinning_and_growth():
    B, N, D = 4, 32, 5
    rs = np.random.RandomState(11)
    mu, ivar = gauss_params(rs, B, D)
    p0 = rs.randn(B, N, D)
    seeds = [5, 6, 7, 8]
    one = EnsembleBatch(B, N, D, BatchCallable(batched_fn(mu, ivar)), moves=de_snooker(), seeds=seeds)
    one.run_mcmc(p0, 30)
    two = EnsembleBatch(B, N, D, BatchCallable(batched_fn(mu, ivar)), moves=de_snooker(), seeds=seeds)
    two.run_mcmc(p0, 18)
    two.run_mcmc(None, 12)                  # the chain grows across the calls and keeps what it stored
    assert_outputs_equal(outputs(one), outputs(two))
    for b in (0, 3):
        s = single(N, D, member_fn(mu, ivar, b), de_snooker, seeds[b], p0[b], None, chunks=(18, 12))
        assert_member_equal(two, b, s)
        for kw in (dict(discard=7, thin=3), dict(flat=True)):
            assert np.array_equal(two[b].get_chain(**kw), s.get_chain(**kw))
            assert np.array_equal(two.get_log_prob(**kw)[b], s.get_log_prob(**kw))
    th = EnsembleBatch(B, N, D, BatchCallable(batched_fn(mu, ivar)), seeds=seeds)
    th.run_mcmc(p0, 10, thin_by=3)
    ns = EnsembleBatch(B, N, D, BatchCallable(batched_fn(mu, ivar)), seeds=seeds)
    ns.run_mcmc(p0, 10, store=False)
    for b in range(B):
        assert_member_equal(th, b, single(N, D, member_fn(mu, ivar, b), stretch, seeds[b], p0[b], 10, thin_by=3))
        assert_member_equal(ns, b, single(N, D, member_fn(mu, ivar, b), stretch, seeds[b], p0[b], 10, store=False), store=False)
    assert ns.iteration == 0


# ---------------------------------------------------------------------------------------------------------------- 6. errors
def test_errors():
    B, N, D, nsteps = 5, 32, 5, 10
    rs = np.random.RandomState(2)
    mu, ivar = gauss_params(rs, B, D)
    p0 = rs.randn(B, N, D)
    seeds = list(range(B))
    fn = batched_fn(mu, ivar)
    clean = EnsembleBatch(B, N, D, BatchCallable(fn), seeds=seeds)
    clean.run_mcmc(p0, nsteps)

    def nan_at(call, member):
        count = [0]

        def f(q):
            out = fn(q)
            if count[0] == call:
                out[member, 0] = float("nan")
            count[0] += 1
            return out
        return f
    bt = EnsembleBatch(B, N, D, BatchCallable(nan_at(5, 3)), seeds=seeds)
    with pytest.raises(ValueError, match="member 3: Probability function returned NaN"):
        bt.run_mcmc(p0, nsteps)
    others = [b for b in range(B) if b != 3]
    assert np.array_equal(bt.get_last_sample().coords[others], clean.get_last_sample().coords[others])
    assert np.array_equal(bt.get_chain()[others], clean.get_chain()[others])
    bt = EnsembleBatch(B, N, D, BatchCallable(nan_at(0, 1)), seeds=seeds)
    with pytest.raises(ValueError, match="member 1: The initial log_prob was NaN"):
        bt.run_mcmc(p0, nsteps)

    # -inf is a rejection: a box on the first coordinate, the same rule in the single sampler
    def boxed(f):
        def g(q):
            out = f(q)
            return torch.where(q[..., 0] > 0.5, torch.full_like(out, -float("inf")), out)
        return g
    pb = np.minimum(p0, 0.4)
    pb[:, :, 1:] = p0[:, :, 1:]
    bx = EnsembleBatch(B, N, D, BatchCallable(boxed(fn)), seeds=seeds)
    bx.run_mcmc(pb, nsteps)
    assert np.all(bx.get_chain()[..., 0] <= 0.5)
    for b in (0, 4):
        assert_member_equal(bx, b, single(N, D, boxed(member_fn(mu, ivar, b)), stretch, seeds[b], pb[b], nsteps))

    class Boom(Exception):
        pass
    count = [0]

    def raising(q):
        count[0] += 1
        if count[0] == 4:
            raise Boom("from the user's function")
        return fn(q)
    bt = EnsembleBatch(B, N, D, BatchCallable(raising), seeds=seeds)
    with pytest.raises(Boom, match="user's function"):
        bt.run_mcmc(p0, nsteps)
    bt = EnsembleBatch(B, N, D, BatchCallable(lambda q: fn(q)[:, :-1]), seeds=seeds)
    with pytest.raises(ValueError, match="returned"):
        bt.run_mcmc(p0, nsteps)
    flat = EnsembleBatch(B, N, D, BatchCallable(lambda q: fn(q).reshape(-1)), seeds=seeds)      # B * n values are accepted
    flat.run_mcmc(p0, nsteps)
    assert_outputs_equal(outputs(clean), outputs(flat))


# ---------------------------------------------------------------------------------------------------------------- 7. kernel
def _build_user_lib(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "user_batch_logprob.hip")
    so = str(tmp_path / "libuser_batch_logprob.so")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so], check=True,
                   timeout=600, capture_output=True)
    _lib.load()                                  # one HIP runtime per process: the library's (torch's) first
    user = C.CDLL(so)
    user.user_setup.restype = C.c_void_p
    user.user_setup.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    user.user_stats.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    user.user_teardown.argtypes = [C.c_void_p]
    return user


def test_a_users_hip_kernel_through_the_c_abi(tmp_path):
    user = _build_user_lib(tmp_path)
    B, N, D, nsteps = 5, 50, 3, 20
    rs = np.random.RandomState(13)
    mu, ivar = gauss_params(rs, B, D)
    p0 = rs.randn(B, N, D)
    seeds = list(range(40, 40 + B))
    h = user.user_setup(np.ascontiguousarray(mu).ctypes.data, np.ascontiguousarray(ivar).ctypes.data, B, D)
    assert h
    kb = EnsembleBatch(B, N, D, BatchKernel(user.user_batch_log_prob, h), moves=de_snooker(), seeds=seeds)
    kb.run_mcmc(p0, nsteps)
    tb = EnsembleBatch(B, N, D, BatchCallable(batched_fn(mu, ivar)), moves=de_snooker(), seeds=seeds)
    tb.run_mcmc(p0, nsteps)
    assert_outputs_equal(outputs(tb), outputs(kb))
    calls, rows = C.c_longlong(), C.c_longlong()
    user.user_stats(h, C.byref(calls), C.byref(rows))
    assert calls.value == 1 + nsteps * 4 and rows.value == N + nsteps * 4 * 25
    assert kb.launch_info()["launches"] == tb.launch_info()["launches"] == 1 + nsteps * 4 + 1
    kb.close()
    user.user_teardown(h)


# ---------------------------------------------------------------------------------------------------------------- 8. throughput
def test_throughput_against_a_loop_of_single_samplers():
    N, D, nsteps, B, nsingle = 32, 5, 200, 512, 16
    rs = np.random.RandomState(0)
    mu, ivar = gauss_params(rs, B, D)
    p0 = rs.randn(B, N, D)
    samplers = [EnsembleSampler(N, D, DeviceCallable(member_fn(mu, ivar, b)), rng="philox") for b in range(nsingle)]
    for b, s in enumerate(samplers):
        s.run_mcmc(p0[b], 5, store=False)                   # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in samplers:
        s.run_mcmc(None, nsteps, store=False)
    torch.cuda.synchronize()
    rate_single = nsingle * nsteps / (time.perf_counter() - t0)
    bt = EnsembleBatch(B, N, D, BatchCallable(batched_fn(mu, ivar)), seeds=list(range(B)))
    bt.run_mcmc(p0, 5, store=False)                          # warm-up
    t0 = time.perf_counter()
    bt.run_mcmc(None, nsteps, store=False)
    rate_batch = B * nsteps / (time.perf_counter() - t0)
    print("loop of %d single samplers: %.3g member-steps/s; batch of %d: %.3g member-steps/s (%.0fx)"
          % (nsingle, rate_single, B, rate_batch, rate_batch / rate_single))
    assert rate_batch >= 20 * rate_single
