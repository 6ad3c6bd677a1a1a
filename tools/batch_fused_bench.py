"""Throughput of EnsembleBatch with the user's model compiled into the batch kernel (targets.BatchFused), beside the same model as a
batched callback (targets.BatchKernel) and the built-in DiagGaussian, in member-steps/s.  The model is model (a) of
tests/c/user_fused_logprob.hip (a per-member diagonal Gaussian) at every shape; the three columns are measured in one process,
one after another per (shape, B).  Each figure: `run_mcmc(None, n, store=False)` with n for about 0.25 s of wall time, one
warm-up run, then `--repeats` (default 5, at least 3) timed runs: median and range.  Prints a JSON line per row and the markdown
table of profiles/batch_fused.md.  `--prof`: the fused runs alone at B = 1 024 (for `rocprofv3 --kernel-trace --stats -- python
tools/batch_fused_bench.py --prof`).
usage: python tools/batch_fused_bench.py [--quick] [--prof] [--repeats K]"""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emcee_amd import EnsembleBatch, _lib, moves  # noqa: E402
from emcee_amd.targets import BatchFused, BatchKernel, DiagGaussian, get_include  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 20
de_snooker = lambda: [(moves.DEMove(), 0.8), (moves.DESnookerMove(), 0.2)]  # noqa: E731
SHAPES = [
    ("32x5 stretch", 32, 5, lambda: moves.StretchMove()),
    ("100x10 DE+snooker", 100, 10, de_snooker),
    ("256x32 stretch", 256, 32, lambda: moves.StretchMove()),
]


def build_models(ndims):
    """tests/c/user_fused_logprob.hip for every ndim, side by side -> ({ndim: CDLL}, seconds of the slowest single compile)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    d = tempfile.mkdtemp()
    procs, t0 = {}, time.perf_counter()
    for n in ndims:
        so = os.path.join(d, "libuser_fused_%d.so" % n)
        cmd = ([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DUSER_NDIM=%d" % n] +
               ["-I" + i for i in get_include()] + [os.path.join(ROOT, "tests", "c", "user_fused_logprob.hip"), "-o", so])
        procs[n] = (so, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    libs = {}
    for n, (so, p) in procs.items():
        _, err = p.communicate(timeout=1200)
        if p.returncode != 0:
            raise RuntimeError(err[-4000:])
        _lib.load()
        u = C.CDLL(so)
        u.user_setup.restype = C.c_void_p
        u.user_setup.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double]
        u.user_device_pointer.restype = C.c_void_p
        u.user_device_pointer.argtypes = [C.c_void_p]
        u.user_teardown.argtypes = [C.c_void_p]
        libs[n] = u
    return libs, time.perf_counter() - t0


def timed(bt, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bt.run_mcmc(None, n, store=False)         # returns the last state: the run has finished
    return time.perf_counter() - t0


def measure(B, N, D, target, mf, p0, repeats):
    """-> (median, lowest, highest member-steps/s over the repeats, steps per run, launch_info)"""
    bt = EnsembleBatch(B, N, D, target, moves=mf(), seeds=list(range(B)))
    bt.run_mcmc(p0, 1, store=False, skip_initial_state_check=True)
    n = 10
    for _ in range(2):                        # a short run is mostly its launch: size the run from one of about the right length
        n = int(max(10, min(400000, n * 0.25 / max(timed(bt, n), 1e-9))))
    timed(bt, n)                              # warm-up at the measured length
    rates = sorted(B * n / timed(bt, n) for _ in range(repeats))
    info = bt.launch_info()
    bt.close()
    return rates[len(rates) // 2], rates[0], rates[-1], n, info


def main():
    quick, prof = "--quick" in sys.argv, "--prof" in sys.argv
    repeats = max(3, int(sys.argv[sys.argv.index("--repeats") + 1])) if "--repeats" in sys.argv else 5
    Bs = [1024] if prof else ([16, 1024] if quick else [16, 256, 1024, 4096])
    libs, compile_s = build_models(sorted({s[2] for s in SHAPES}))
    print("compiled tests/c/user_fused_logprob.hip (two models, four kernels a library) for ndim %s side by side in %.1f s"
          % (sorted(libs), compile_s), flush=True)
    rows = []
    for name, N, D, mf in SHAPES:
        rs = np.random.RandomState(1)
        for B in Bs:
            mu = np.ascontiguousarray(0.1 * rs.randn(B, D))
            ivar = np.ascontiguousarray(1.0 / (0.2 + rs.rand(B, D)))
            data = np.zeros((B, 3, K))
            p0 = rs.randn(B, N, D)
            u = libs[D]
            h = u.user_setup(mu.ctypes.data, ivar.ctypes.data, data.ctypes.data, B, D, -1, 0.0)
            fused = measure(B, N, D, BatchFused(u.user_fused_a, D, user=u.user_device_pointer(h)), mf, p0, repeats)
            if prof:
                print("%s B=%d fused: %.3g member-steps/s" % (name, B, fused[0]), flush=True)
                u.user_teardown(h)
                continue
            kern = measure(B, N, D, BatchKernel(u.user_block_a, h), mf, p0, repeats)
            built = measure(B, N, D, [DiagGaussian(mu[b], ivar[b]) for b in range(B)], mf, p0, repeats)
            u.user_teardown(h)
            r = dict(shape=name, B=B, threads=fused[4]["threads"], plan_steps=fused[4]["plan_steps"], fused=fused[:3], fused_steps=fused[3],
                     kernel=kern[:3], kernel_steps=kern[3], builtin=built[:3], builtin_steps=built[3],
                     ranges_apart=bool(fused[1] > kern[2]))
            print(json.dumps(r), flush=True)
            rows.append(r)
    if prof:
        return
    cell = lambda v: "%.3g (%.3g - %.3g)" % tuple(v)  # noqa: E731
    print("\n| shape | B | threads, plan steps | BatchFused: median (range) | BatchKernel | built-in DiagGaussian | fused / kernel | "
          "fused / built-in | ranges apart |\n|---|---:|---:|---:|---:|---:|---:|---:|---|")
    for r in rows:
        print("| %s | %d | %d, %d | %s | %s | %s | %.1fx | %.2f | %s |"
              % (r["shape"], r["B"], r["threads"], r["plan_steps"], cell(r["fused"]), cell(r["kernel"]), cell(r["builtin"]),
                 r["fused"][0] / r["kernel"][0], r["fused"][0] / r["builtin"][0], "yes" if r["ranges_apart"] else "NO"))


if __name__ == "__main__":
    main()
