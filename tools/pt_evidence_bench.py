"""PTSampler.get_evidence (emx_pt_evidence: the stored log-likelihood plane reduced next to the chain) against the only path
there was before it: get_log_likelihood() over PCIe plus pt.stepping_stone_log_evidence on the host.  Two shapes: 128 objects x
8 rungs x 32 walkers with 5 000 stored steps (the batch profiles' 1 024 members), and 1 object x 8 rungs x 64 walkers with 100 000
stored steps (8 members: the shape that needs the slicing).  The model is the 2-d unit Gaussian in the +-10 box as a fused
tempered target (compile_fused_pt), so that filling the chain takes seconds.

get_evidence is timed once cold and then repeatedly for at least `--seconds` and at least 5 calls: the median; a call returns after
its results are on the host.  The host path is timed once, whole.  "plane GB/s" is the bytes of the used part of the L plane,
counted once, over the call's time; the kernel reads them once.
"of it the library call" times emx_pt_evidence through ctypes alone (PTSampler._evidence_blocks): the rest of a get_evidence call
is the NumPy merge of the blocks.
usage: python tools/pt_evidence_bench.py [--quick] [--out pt_evidence_bench.json] [--seconds 1] [--cache DIR] [--nblocks 8]
       python tools/pt_evidence_bench.py --prof       (a dozen calls per shape: for rocprofv3 --kernel-trace --stats)
       python tools/pt_evidence_bench.py --compile-only --cache DIR       (builds the fused target into DIR; needs no GPU)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emcee_amd import PTSampler  # noqa: E402
from emcee_amd.pt import stepping_stone_log_evidence  # noqa: E402
from emcee_amd.targets import compile_fused_pt  # noqa: E402

SOURCE = r"""
struct Gauss {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const {
        double acc = 0.0;
        for (int d = 0; d < ndim; ++d) acc = acc + x[d] * x[d];
        return -0.5 * acc - 1.8378770664093453;
    }
};
"""
D = 2


def timed(call, seconds):
    t0 = time.perf_counter()
    out = call()
    cold = time.perf_counter() - t0
    times, total = [], 0.0
    while total < seconds or len(times) < 5:
        t0 = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t0)
        total += times[-1]
    return cold, float(np.median(times)), len(times), out


def bench(lib, G, T, N, steps, K, seconds):
    s = PTSampler(T, N, D, lib.target(), log_prior=(-10 * np.ones(D), 10 * np.ones(D)), Tmax=np.inf, nbatch=G, seeds=list(range(G)))
    t0 = time.perf_counter()
    s.run_mcmc(np.random.RandomState(1).uniform(-1, 1, size=(G, T, N, D)), steps)
    fill = time.perf_counter() - t0
    cold, warm, calls, ev = timed(lambda: s.get_evidence(nblocks=K), seconds)
    _, lib_warm, _, _ = timed(lambda: s._evidence_blocks(nblocks=K), seconds)          # the library call alone: no NumPy merge
    t0 = time.perf_counter()
    L = s.get_log_likelihood()
    t_copy = time.perf_counter() - t0
    host = stepping_stone_log_evidence(s.ladder, L, nblocks=K)
    t_host = time.perf_counter() - t0
    del L
    gb = G * T * N * (steps // K) * K * 8 / 1e9
    s.close()
    return dict(shape="%d objects x %d rungs x %d walkers, %d stored steps" % (G, T, N, steps), nblocks=K, plane_GB=gb, fill_s=fill,
                first_s=cold, warm_s=warm, calls_timed=calls, plane_GBps=gb / warm, library_call_s=lib_warm, host_copy_s=t_copy, host_s=t_host,
                host_over_warm=t_host / warm, max_abs_diff_logz_ss=float(np.abs(ev.logz_ss - host.logz_ss).max()),
                logz_ss=[float(ev.logz_ss.mean()), float(ev.logz_ss.std())], mean_err_ss=float(ev.err_ss.mean()),
                logz_ti=float(ev.logz_ti.mean()), exact=float(-2 * np.log(20)))


def main():
    arg = lambda flag, default, kind: kind(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default  # noqa: E731
    lib = compile_fused_pt(SOURCE, "Gauss", D, name="evidence_bench_gauss", cache_dir=arg("--cache", None, str))
    if "--compile-only" in sys.argv:
        return
    seconds, K, out_path = arg("--seconds", 1.0, float), arg("--nblocks", 8, int), arg("--out", "pt_evidence_bench.json", str)
    if "--prof" in sys.argv:           # six calls of each kind per shape: for rocprofv3 --kernel-trace --stats
        seconds = 0.0
    shapes = ((16, 8, 32, 500), (1, 8, 64, 10000)) if "--quick" in sys.argv else ((128, 8, 32, 5000), (1, 8, 64, 100000))
    rows = []
    for G, T, N, steps in shapes:
        rows.append(bench(lib, G, T, N, steps, K, seconds))
        print(json.dumps(rows[-1]), flush=True)
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
    print("\n| shape | plane GB | first s | warm s (calls) | of it the library call s | plane GB/s | host: copy s | host: copy + estimator s | host / warm | max diff of logz_ss |")
    print("|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|")
    for r in rows:
        print("| %s | %.3f | %.4f | %.5f (%d) | %.5f | %.0f | %.3f | %.3f | %.0fx | %.2g |" % (
            r["shape"], r["plane_GB"], r["first_s"], r["warm_s"], r["calls_timed"], r["library_call_s"], r["plane_GBps"], r["host_copy_s"], r["host_s"],
            r["host_over_warm"], r["max_abs_diff_logz_ss"]))


if __name__ == "__main__":
    main()
