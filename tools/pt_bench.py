"""PTSampler throughput against EnsembleBatch's callback path at the same members and the same callable.

    python tools/pt_bench.py [--nbatch 64 --ntemps 16 --nwalkers 32 --ndim 5 --steps 200 --reps 3] [--adaptive] [--json out.json]
    python tools/pt_bench.py --fused [--adaptive] [...]      # PTFused against the BatchKernel wrapping of the same functor

Shape: nbatch objects x ntemps rungs x nwalkers x ndim with a torch two-component Gaussian mixture likelihood.  Reports member-steps
per second (members = nbatch * ntemps) of PTSampler with swap_every = 1 and 0, and of EnsembleBatch on the tempered callable
(beta_t L + box prior), best of `reps` timed runs of `steps` steps without storing.  --adaptive also times PTSampler with
swap_every = 1 and the adaptive ladder (ptemcee's lag and time)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from emcee_amd import EnsembleBatch, PTSampler  # noqa: E402
from emcee_amd.targets import BatchCallable  # noqa: E402


def mixture(D):
    s2 = 0.3 ** 2
    lw1, lw2, norm = np.log(0.25), np.log(0.75), -0.5 * D * np.log(2 * np.pi * s2)

    def fn(q):
        d1 = ((q + 4.0) ** 2).sum(-1)
        d2 = ((q - 4.0) ** 2).sum(-1)
        return torch.logaddexp(lw1 - 0.5 * d1 / s2, lw2 - 0.5 * d2 / s2) + norm
    return fn


def timed(run, steps, reps):
    best = 0.0
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        best = max(best, steps / (time.perf_counter() - t0))
    return best


FUSED_SOURCE = r"""
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
struct Mixture {
    __device__ double operator()(const double* x, int ndim, int, const void*) const { return mixture(x, ndim); }
};
__global__ void k_mixture(const double* q, long long n, int D, double* out) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = mixture(q + k * D, D);
}
extern "C" __attribute__((visibility("default"))) int mixture_block(void*, const double* q, int32_t nbatch, int64_t rows, int32_t ndim,
                                                                    double* out, void* stream) {
    const long long n = (long long)nbatch * rows;
    if (n > 0) hipLaunchKernelGGL(k_mixture, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, q, n, (int)ndim, out);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}
"""


def fused_main(a):
    """PTFused against PTSampler with the BatchKernel wrapping of the same device function: alternated, warmed up, windows of
    at least 1 s, best and spread of `reps` repetitions each, outputs compared for equality at the timed shape."""
    from emcee_amd.targets import BatchKernel, compile_fused_pt
    G, T, N, D = a.nbatch, a.ntemps, a.nwalkers, a.ndim
    lib = compile_fused_pt(FUSED_SOURCE, "Mixture", D)
    box = (-10 * np.ones(D), 10 * np.ones(D))
    p0 = -4.0 + 0.3 * np.random.RandomState(0).randn(G, T, N, D)
    out = dict(nbatch=G, ntemps=T, nwalkers=N, ndim=D, steps=a.steps, members=G * T, adaptive=bool(a.adaptive))
    mk = lambda like: PTSampler(T, N, D, like, log_prior=box, Tmax=1e3, nbatch=G, seeds=list(range(G)), swap_every=1,  # noqa: E731
                                adaptive=a.adaptive)
    pts = dict(fused=mk(lib.target()), kernel=mk(BatchKernel(lib.lib.mixture_block)))
    for pt in pts.values():
        pt.run_mcmc(p0, 20)
    out["equal"] = bool(np.array_equal(pts["fused"].get_chain(), pts["kernel"].get_chain()) and
                        np.array_equal(pts["fused"].get_log_likelihood(), pts["kernel"].get_log_likelihood()) and
                        np.array_equal(pts["fused"].ladder, pts["kernel"].ladder))
    rates = dict(fused=[], kernel=[])
    for _ in range(a.reps):
        for name, pt in pts.items():
            n, t = 0, 0.0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            while t < 1.0:
                pt.run_mcmc(None, a.steps, store=False)
                torch.cuda.synchronize()
                n += a.steps
                t = time.perf_counter() - t0
            rates[name].append(G * T * n / t)
    for name, pt in pts.items():
        n0 = pt.launch_info()["launches"]
        pt.run_mcmc(None, 10, store=False)
        out["%s_launches_per_step" % name] = (pt.launch_info()["launches"] - n0) / 10.0
        out["%s_member_steps_per_s" % name] = max(rates[name])
        out["%s_spread" % name] = (max(rates[name]) - min(rates[name])) / max(rates[name])
        pt.close()
    out["fused_over_kernel"] = out["fused_member_steps_per_s"] / out["kernel_member_steps_per_s"]
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nbatch", type=int, default=64)
    ap.add_argument("--ntemps", type=int, default=16)
    ap.add_argument("--nwalkers", type=int, default=32)
    ap.add_argument("--ndim", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--adaptive", action="store_true", help="also time swap_every=1 with the adaptive ladder")
    ap.add_argument("--json", default=None)
    ap.add_argument("--fused", action="store_true", help="targets.PTFused against the BatchKernel wrapping of the same functor")
    a = ap.parse_args()
    if a.fused:
        return fused_main(a)
    G, T, N, D = a.nbatch, a.ntemps, a.nwalkers, a.ndim
    fn = mixture(D)
    box = (-10 * np.ones(D), 10 * np.ones(D))
    p0 = -4.0 + 0.3 * np.random.RandomState(0).randn(G, T, N, D)
    out = dict(nbatch=G, ntemps=T, nwalkers=N, ndim=D, steps=a.steps, members=G * T)
    for every, adaptive in ((1, False), (0, False)) + (((1, True),) if a.adaptive else ()):
        pt = PTSampler(T, N, D, BatchCallable(fn), log_prior=box, Tmax=1e3, nbatch=G, seeds=list(range(G)), swap_every=every,
                       adaptive=adaptive)
        pt.run_mcmc(p0, 10, store=False)
        key = "pt_swap_every_%d%s_member_steps_per_s" % (every, "_adaptive" if adaptive else "")
        out[key] = G * T * timed(lambda n: pt.run_mcmc(None, n, store=False), a.steps, a.reps)
        if adaptive:
            n0 = pt.launch_info()["launches"]
            pt.run_mcmc(None, 10, store=False)
            out["pt_adaptive_launches_per_step"] = (pt.launch_info()["launches"] - n0) / 10.0
            out["tswap_acceptance_mean_adaptive"] = float(pt.tswap_acceptance_fraction.mean())
        elif every == 1:
            out["pt_launches_per_step"] = None
            n0 = pt.launch_info()["launches"]
            pt.run_mcmc(None, 10, store=False)
            out["pt_launches_per_step"] = (pt.launch_info()["launches"] - n0) / 10.0
            out["tswap_acceptance_mean"] = float(pt.tswap_acceptance_fraction.mean())
        pt.close()
    betas = PTSampler(T, N, D, BatchCallable(fn), Tmax=1e3).betas
    bt = torch.as_tensor(np.tile(betas, G), device="cuda")[:, None]
    lo, hi = (torch.as_tensor(v, device="cuda") for v in box)

    def tempered(q):
        inside = ((q >= lo) & (q <= hi)).all(-1)
        return bt * fn(q) + torch.where(inside, 0.0, -float("inf")).to(torch.float64)
    eb = EnsembleBatch(G * T, N, D, BatchCallable(tempered), seeds=list(range(G * T)))
    eb.run_mcmc(p0.reshape(G * T, N, D), 10, store=False)
    out["batch_member_steps_per_s"] = G * T * timed(lambda n: eb.run_mcmc(None, n, store=False), a.steps, a.reps)
    out["pt_over_batch"] = out["pt_swap_every_1_member_steps_per_s"] / out["batch_member_steps_per_s"]
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
