"""Throughput of EnsembleBatch with the user's batched log-probability (targets.BatchCallable, torch eager, and targets.BatchKernel, a
HIP kernel of the user's own) in member-steps/s, beside a Python loop of single EnsembleSampler(DeviceCallable) runs, and the
share of a step the user's function takes.  Writes profiles/batch_callback.md (the k_batch_cb kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of `--prof`, see that file).
usage: python tools/batch_callback_bench.py [--quick] [--prof] [--out profiles/batch_callback.md]"""
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from emcee_amd import EnsembleBatch, EnsembleSampler, _lib, moves  # noqa: E402
from emcee_amd.targets import BatchCallable, BatchKernel, DeviceCallable  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
de_snooker = lambda: [(moves.DEMove(), 0.8), (moves.DESnookerMove(), 0.2)]  # noqa: E731
SHAPES = [
    # name, N, D, target, moves, S_max
    ("32x5 iso stretch", 32, 5, "iso", lambda: moves.StretchMove(), 2),
    ("100x10 diag DE+snooker", 100, 10, "diag", de_snooker, 4),
    ("256x32 rosenbrock stretch", 256, 32, "rosen", lambda: moves.StretchMove(), 2),
]


def torch_fn(kind, mu, ivar):
    """the (B, n, D) -> (B, n) log-probability a user writes in torch, per-member parameters (B, 1, D) in the closure"""
    mu_t = torch.as_tensor(mu, device="cuda")[:, None, :]
    iv_t = torch.as_tensor(ivar, device="cuda")[:, None, :]
    if kind == "iso":
        return lambda q: -0.5 * (q * q).sum(-1)
    if kind == "diag":
        return lambda q: -0.5 * (iv_t * (q - mu_t) ** 2).sum(-1)
    return lambda q: -(100.0 * (q[..., 1:] - q[..., :-1] ** 2) ** 2 + (1.0 - q[..., :-1]) ** 2).sum(-1) / 20.0


def member_fn(kind, mu, ivar, b):
    """the same function restricted to member b: (n, D) -> (n)"""
    f = torch_fn(kind, mu[b:b + 1], ivar[b:b + 1])
    return lambda q: f(q[None])[0]


def p0_of(kind, shape, rs):
    return 1.0 + 0.1 * rs.randn(*shape) if kind == "rosen" else rs.randn(*shape)


def timed(run, steps):
    run(max(2, steps // 10))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(steps)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def adaptive(run, budget=0.25, most=2000):
    """steps so that the timed run takes about `budget` seconds; -> seconds per step"""
    probe = timed(run, 10) / 10
    steps = int(max(10, min(most, budget / max(probe, 1e-9))))
    return timed(run, steps) / steps


def build_user_kernel():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    so = os.path.join(tempfile.mkdtemp(), "libuser_batch_logprob.so")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-shared", "-fPIC",
                    os.path.join(ROOT, "tests", "c", "user_batch_logprob.hip"), "-o", so], check=True, timeout=600, capture_output=True)
    _lib.load()
    user = C.CDLL(so)
    user.user_setup.restype = C.c_void_p
    user.user_setup.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    user.user_teardown.argtypes = [C.c_void_p]
    user.user_batch_log_prob.restype = C.c_int
    user.user_batch_log_prob.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    return user


def bench_batch(B, N, D, target, mf, p0):
    bt = EnsembleBatch(B, N, D, target, moves=mf(), seeds=list(range(B)))
    bt.run_mcmc(p0, 1, store=False, skip_initial_state_check=True)
    sec = adaptive(lambda n: bt.run_mcmc(None, n, store=False))
    info = bt.launch_info()
    bt.close()
    return sec, info


def user_share(call, B, R, D, smax):
    """seconds per step of the user's function alone: S_max calls on a (B, R, D) block, enqueued as in a run"""
    q = torch.randn(B, R, D, dtype=torch.float64, device="cuda")
    out = torch.empty(B, R, dtype=torch.float64, device="cuda")
    return adaptive(lambda n: [call(q, out) for _ in range(n * smax)])


def bench_loop(N, D, kind, mf, rs, count=16, steps=50):
    """a Python loop over `count` single EnsembleSampler(DeviceCallable) runs of the same steps (what a user writes without the batch)"""
    mu, ivar = 0.1 * rs.randn(count, D), 1.0 / (0.2 + rs.rand(count, D))
    p0 = p0_of(kind, (count, N, D), rs)
    ss = [EnsembleSampler(N, D, DeviceCallable(member_fn(kind, mu, ivar, b)), moves=mf(), rng="philox") for b in range(count)]
    for b, s in enumerate(ss):
        s.run_mcmc(p0[b], 2, store=False, skip_initial_state_check=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in ss:
        s.run_mcmc(None, steps, store=False)
    torch.cuda.synchronize()
    return count * steps / (time.perf_counter() - t0)


def main():
    quick, prof = "--quick" in sys.argv, "--prof" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "batch_callback.md")
    Bs = [1024] if prof else ([1, 16, 1024] if quick else [1, 16, 256, 1024, 4096])
    user = None if prof else build_user_kernel()
    rows = []
    for name, N, D, kind, mf, smax in SHAPES:
        rs = np.random.RandomState(1)
        smin = 1 if smax == 1 else 2
        R = (N + smin - 1) // smin
        loop = None
        for B in Bs:
            mu, ivar = 0.1 * rs.randn(B, D), 1.0 / (0.2 + rs.rand(B, D))
            p0 = p0_of(kind, (B, N, D), rs)
            fn = torch_fn(kind, mu, ivar)
            sec_cb, info = bench_batch(B, N, D, BatchCallable(fn), mf, p0)
            if prof:
                print("%s B=%d: %.3g member-steps/s" % (name, B, B / sec_cb), flush=True)
                continue
            if loop is None:
                loop = bench_loop(N, D, kind, mf, rs)

            def torch_call(q, out):
                out.copy_(fn(q))
            u_cb = user_share(torch_call, B, R, D, smax)
            h = user.user_setup(np.ascontiguousarray(mu).ctypes.data, np.ascontiguousarray(ivar).ctypes.data, B, D)
            sec_k, _ = bench_batch(B, N, D, BatchKernel(user.user_batch_log_prob, h), mf, p0)
            stream = torch.cuda.current_stream().cuda_stream

            def kernel_call(q, out):
                user.user_batch_log_prob(h, q.data_ptr(), B, R, D, out.data_ptr(), stream)
            u_k = user_share(kernel_call, B, R, D, smax)
            user.user_teardown(h)
            r = dict(shape=name, B=B, R=R, smax=smax, threads=info["threads"], loop=loop, cb=B / sec_cb, cb_step_us=1e6 * sec_cb,
                     cb_user_us=1e6 * u_cb, k=B / sec_k, k_step_us=1e6 * sec_k, k_user_us=1e6 * u_k)
            print(r, flush=True)
            rows.append(r)
    if prof:
        return
    with open(out_path, "w") as f:
        f.write(HEADER)
        f.write("| shape | B | threads | loop member-steps/s | BatchCallable member-steps/s (x loop) | step us: user share | "
                "BatchKernel member-steps/s (x loop) | step us: user share |\n|---|---:|---:|---:|---:|---:|---:|---:|\n")
        for r in rows:
            f.write("| %s | %d | %d | %.3g | %.3g (%.0fx) | %.0f: %.0f %% | %.3g (%.0fx) | %.0f: %.0f %% |\n"
                    % (r["shape"], r["B"], r["threads"], r["loop"], r["cb"], r["cb"] / r["loop"], r["cb_step_us"],
                       100 * min(1.0, r["cb_user_us"] / r["cb_step_us"]), r["k"], r["k"] / r["loop"], r["k_step_us"],
                       100 * min(1.0, r["k_user_us"] / r["k_step_us"])))


HEADER = """# EnsembleBatch with the user's batched log-probability

Made by `python tools/batch_callback_bench.py` on one MI355X (256 CUs).  Member-steps/s: B members x steps per second of wall
time around `run_mcmc(None, n, store=False)` (n chosen for about 0.25 s).  *loop*: 16 single
`EnsembleSampler(DeviceCallable(fn_b), rng="philox")` runs of the same function restricted to one member, run one after another
from Python (what a user writes without the batch), scaled to member-steps/s.  *BatchCallable*: torch eager, per-member
parameters `(B, 1, D)` in the closure (`iso`: `-0.5 (q q).sum(-1)`; `diag`: `-0.5 (ivar (q - mu)^2).sum(-1)`; `rosenbrock`: the
BASELINE config-3 form over `q[..., 1:]`, `q[..., :-1]`).  *BatchKernel*: `tests/c/user_batch_logprob.hip`, one thread a row
evaluating the per-member diagonal Gaussian at every shape (the library's side of the step is the same for any target).  *step
us*: wall time of one proposal step (S_max launches of `k_batch_cb` + S_max calls); *user share*: the same S_max calls of the
user's function alone on a `(B, R, D)` block, over the step time -- the rest is the library's kernels and their launches.

"""

if __name__ == "__main__":
    main()
