"""What blobs cost a PTSampler, on both paths, and whether a blob-free run costs what it did before blobs existed.

    python tools/pt_blobs_bench.py --parent /path/to/a/built/checkout/of/the/parent/commit [--reps 5] [--json out.json]

For every shape (objects x rungs x walkers x ndim; the shapes of profiles/pt_fused.md) and both paths -- the fused tempered kernel
(targets.PTFused, compile_fused_pt) and the batched callback (targets.BatchKernel around the same __device__ function) -- three
figures in microseconds per proposal step of the whole sampler: K = 0 blobs with the parent's library and headers, K = 0 with
this tree's, K = 4 with this tree's.  The two trees are measured in processes of their own, alternated `reps` times in one
session on one machine; a figure is one window of at least `--window` seconds of run_mcmc(None, steps, store=False) calls after a
warm-up, swap_every = 1, the box prior, Tmax = 1e3 (tools/pt_bench.py's conditions).  The table gives the median of the
repetitions and the spread (max - min) / median; the K = 0 figure of this tree is held against the parent's spread.

    python tools/pt_blobs_bench.py --worker --tree PATH [--blobs]      # one repetition of one tree: a JSON line (what --parent spawns)
    python tools/pt_blobs_bench.py --worker --tree PATH --compile-only # fill the compile cache (needs no GPU)

The likelihood is tools/pt_bench.py's two-mode mixture; its blobs are {L, x[0] + x[1], x[0] * x[1], (double)member}."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(64, 16, 32, 5), (1024, 4, 32, 5), (8, 8, 64, 16)]
K = 4

SOURCE = r"""
#define BENCH_NBLOBS 4
__device__ inline double mixture(const double* x, int ndim) {
    const double s2 = 0.3 * 0.3;
    double d1 = 0.0, d2 = 0.0;
    for (int d = 0; d < ndim; ++d) {
        d1 = d1 + (x[d] + 4.0) * (x[d] + 4.0);
        d2 = d2 + (x[d] - 4.0) * (x[d] - 4.0);
    }
    const double a = -1.3862943611198906 - 0.5 * d1 / s2, b = -0.2876820724517809 - 0.5 * d2 / s2;
    const double hi = a > b ? a : b, lo = a > b ? b : a;
    return hi + log1p(exp(lo - hi)) - 0.5 * (double)ndim * log(2.0 * 3.141592653589793 * s2);
}
__device__ inline void the_blobs(double L, const double* x, int member, double* blobs) {
    blobs[0] = L;
    blobs[1] = x[0] + x[1];
    blobs[2] = x[0] * x[1];
    blobs[3] = (double)member;
}
struct Mixture {
    __device__ double operator()(const double* x, int ndim, int, const void*) const { return mixture(x, ndim); }
};
struct MixtureBlobs {
    __device__ double operator()(const double* x, int ndim, int member, const void*, double* blobs) const {
        const double L = mixture(x, ndim);
        the_blobs(L, x, member, blobs);
        return L;
    }
};
__global__ void k_mixture(const double* q, long long n, long long rows, int D, double* out, double* blobs) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const double L = mixture(q + k * D, D);
    out[k] = L;
    if (blobs) the_blobs(L, q + k * D, (int)(k / rows), blobs + k * BENCH_NBLOBS);
}
static int block(const double* q, int32_t nbatch, int64_t rows, int32_t ndim, double* out, double* blobs, void* stream) {
    const long long n = (long long)nbatch * rows;
    if (n > 0)
        hipLaunchKernelGGL(k_mixture, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, q, n, (long long)rows, (int)ndim, out,
                           blobs);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}
extern "C" __attribute__((visibility("default"))) int mixture_block(void*, const double* q, int32_t nbatch, int64_t rows, int32_t ndim,
                                                                    double* out, void* stream) {
    return block(q, nbatch, rows, ndim, out, nullptr, stream);
}
extern "C" __attribute__((visibility("default"))) int mixture_block_blobs(void*, const double* q, int32_t nbatch, int64_t rows, int32_t ndim,
                                                                          double* out, int32_t nblobs, double* blobs, void* stream) {
    return nblobs == BENCH_NBLOBS && blobs ? block(q, nbatch, rows, ndim, out, blobs, stream) : 1;
}
"""


def worker(a):
    """one repetition in the tree a.tree: every shape, both paths, K = 0 and (with --blobs) K = 4 -> one JSON line"""
    sys.path.insert(0, os.path.abspath(a.tree))
    from emcee_amd import PTSampler
    from emcee_amd.targets import BatchKernel, compile_fused_pt
    ks = (0, K) if a.blobs else (0,)
    libs = {}
    for D in sorted({s[3] for s in SHAPES}):
        for k in ks:
            kw = dict(nblobs=k) if k else {}
            libs[D, k] = compile_fused_pt(SOURCE, "MixtureBlobs" if k else "Mixture", D, cache_dir=a.cache, **kw)
    if a.compile_only:
        print(json.dumps(dict(tree=a.tree, compiled=sorted("%dx%d" % dk for dk in libs))))
        return
    import torch
    out = dict(tree=a.tree, figures={})
    for G, T, N, D in SHAPES:
        box = (-10 * np.ones(D), 10 * np.ones(D))
        p0 = -4.0 + 0.3 * np.random.RandomState(0).randn(G, T, N, D)
        for path in ("fused", "callback"):
            for k in ks:
                lib = libs[D, k]
                if path == "fused":
                    like = lib.target()
                else:
                    like = BatchKernel(lib.lib.mixture_block_blobs, nblobs=k) if k else BatchKernel(lib.lib.mixture_block)
                pt = PTSampler(T, N, D, like, log_prior=box, Tmax=1e3, nbatch=G, seeds=list(range(G)), swap_every=1,
                               **(dict(blobs=True) if k else {}))
                pt.run_mcmc(p0, a.steps, store=False)
                pt.run_mcmc(None, a.steps, store=False)
                n, t = 0, 0.0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                while t < a.window:
                    pt.run_mcmc(None, a.steps, store=False)
                    torch.cuda.synchronize()
                    n += a.steps
                    t = time.perf_counter() - t0
                out["figures"]["%dx%dx%dx%d %s K=%d" % (G, T, N, D, path, k)] = 1e6 * t / n
                pt.close()
    print(json.dumps(out))


def spawn(tree, a, blobs):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree, "--steps", str(a.steps), "--window", str(a.window)]
    cmd += ["--cache", a.cache] if a.cache else []
    cmd += ["--blobs"] if blobs else []
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("worker failed in %s:\n%s" % (tree, (r.stderr or r.stdout)[-4000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])["figures"]


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    med = float(np.median(v))
    return med, float((v.max() - v.min()) / med)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--cache", default=None, help="compile cache directory (default: compile_fused_pt's)")
    ap.add_argument("--json", default=None)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(HERE))
    ap.add_argument("--blobs", action="store_true")
    ap.add_argument("--compile-only", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent:
        ap.error("--parent: a built checkout of the parent commit")
    runs = dict(parent=[], this=[])
    for rep in range(a.reps):                        # alternated: both trees see the same drift of the machine
        runs["parent"].append(spawn(a.parent, a, False))
        runs["this"].append(spawn(os.path.dirname(HERE), a, True))
        print("repetition %d of %d done" % (rep + 1, a.reps), file=sys.stderr, flush=True)
    rows = []
    print("| objects x rungs x walkers x ndim | path | K = 0, parent: us / step (spread) | K = 0, this: us / step (spread) | this / parent | "
          "inside the parent's spread | K = %d, this: us / step (spread) | K = %d / K = 0 |" % (K, K))
    print("|---|---|---:|---:|---:|---|---:|---:|")
    for G, T, N, D in SHAPES:
        for path in ("fused", "callback"):
            key = "%dx%dx%dx%d %s" % (G, T, N, D, path)
            par = [r[key + " K=0"] for r in runs["parent"]]
            new = [r[key + " K=0"] for r in runs["this"]]
            blb = [r[key + " K=%d" % K] for r in runs["this"]]
            (pm, ps), (nm, ns), (bm, bs) = stats(par), stats(new), stats(blb)
            inside = nm <= max(par)                  # the median is no slower than the parent's own slowest repeat
            rows.append(dict(shape=[G, T, N, D], path=path, parent_us=par, this_us=new, blobs_us=blb, inside=bool(inside)))
            print("| %d x %d x %d x %d | %s | %.1f (%.1f %%) | %.1f (%.1f %%) | %.3f | %s | %.1f (%.1f %%) | %.3f |"
                  % (G, T, N, D, path, pm, 100 * ps, nm, 100 * ns, nm / pm, "yes" if inside else "NO", bm, 100 * bs, bm / nm))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(reps=a.reps, steps=a.steps, window=a.window, rows=rows), f)


if __name__ == "__main__":
    main()
