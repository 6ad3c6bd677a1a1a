"""us per step of ONE user model -- a diagonal Gaussian with its data behind `user` -- run three ways through EnsembleSampler:

  fused    targets.DeviceFused: the functor compiled into the half-step kernel (one launch a half-step) and, where the ensemble
           fits one workgroup's LDS and that is the faster path, into the one-workgroup kernel (one launch a chunk of steps)
  fused_small     the same target with the tuning key small_kernel = 2: the one-workgroup kernel wherever the ensemble fits
  fused_general   the same target with the tuning key small_kernel = 0: always one launch a half-step
  kernel   targets.DeviceKernel: the same function behind an emx_device_log_prob_fn (three launches a half-step)
  builtin  targets.DiagGaussian: the library's own closed form (the distance left to a built-in target)

  fused+K  the same functor in its five-argument form with K blobs a sample (--nblobs 1,4,32 adds one such mode per count)
  host     the same model with one blob as a vectorised Python callable: the host-callable path, for scale

    python tools/ensemble_fused_bench.py [--modes fused,kernel,builtin,host] [--shapes 65536x64,4096x16,1048576x32] [--seconds 1.5]
                                         [--nblobs 1,4,32] [--store] [--flags="-IDIR ..."] [--out FILE]
                                         [--rng philox|mt19937] [--moves stretch|de+snooker] [--block STEPS]

`--rng` picks the plans (default Philox), `--moves` the schedule (default one StretchMove; de+snooker: a 0.6 / 0.4 mixture).  Blocks of steps timed by a host clock around a device synchronise; the median of at least `--seconds`
of blocks per mode, the modes of a shape taken in alternation so that drift of the machine hits them alike.  store=False unless
`--store`: then every step appends chain, log-probs and blobs, the sampler is reset before each block (the chain keeps its
allocation) and a block is as many steps as fit 4 GB of chain.  `--modes kernel` needs
nothing of the fused target, so the same file measures a checkout that predates it.  `--flags` are further compiler flags of the
fused launcher: tuning experiments put an edited copy of emx_fused_ensemble.hpp ahead of the library's with --flags=-IDIR.  Prints
one JSON line per shape and mode; `steps_total` counts every step the mode's sampler ran (a kernel trace has two half-steps each)."""
import argparse
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import emcee_amd  # noqa: E402
from emcee_amd import _lib, targets  # noqa: E402

MODEL = r"""
struct diag_data { const double* mu; const double* ivar; };
__device__ inline double diag_model(const double* x, int ndim, const void* user) {
    const diag_data* u = (const diag_data*)user;
    double acc = 0.0;
    for (int d = 0; d < ndim; ++d) {
        const double r = x[d] - u->mu[d];
        acc = acc + u->ivar[d] * r * r;
    }
    return -0.5 * acc;
}
#ifndef BENCH_NBLOBS
#define BENCH_NBLOBS 0
#endif
struct DiagModel {
    __device__ double operator()(const double* x, int ndim, int, const void* user) const { return diag_model(x, ndim, user); }
    __device__ double operator()(const double* x, int ndim, int, const void* user, double* blobs) const {
        const double lp = diag_model(x, ndim, user);
        blobs[0] = lp;
#pragma unroll
        for (int k = 1; k < BENCH_NBLOBS; ++k) blobs[k] = x[k % ndim] * (double)(k + 1);
        return lp;
    }
};
"""

# the DeviceKernel wrapping of the same function: one thread a row, and the setup of its data
CALLBACK = r"""
#include <hip/hip_runtime.h>
#include <stdint.h>
""" + MODEL + r"""
__global__ __launch_bounds__(256) void k_diag_rows(const double* __restrict__ q, long long n, int D, const diag_data* u, double* __restrict__ out) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = diag_model(q + k * D, D, u);
}
extern "C" {
__attribute__((visibility("default"))) void* diag_setup(const double* mu, const double* ivar, int ndim) {
    double *dmu = nullptr, *div = nullptr;
    diag_data h, *d = nullptr;
    if (hipMalloc((void**)&dmu, ndim * 8) != hipSuccess || hipMalloc((void**)&div, ndim * 8) != hipSuccess ||
        hipMalloc((void**)&d, sizeof(diag_data)) != hipSuccess)
        return nullptr;
    h.mu = dmu;
    h.ivar = div;
    if (hipMemcpy(dmu, mu, ndim * 8, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(div, ivar, ndim * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d, &h, sizeof(h), hipMemcpyHostToDevice) != hipSuccess)
        return nullptr;
    return d;
}
__attribute__((visibility("default"))) int diag_rows(void* user, const double* q, int64_t n, int32_t ndim, double* out, void* st) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_diag_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)st, q, (long long)n, (int)ndim,
                       (const diag_data*)user, out);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}
}
"""


def build_callback(work):
    so = os.path.join(work, "libdiag_cb_%s.so" % hashlib.sha256(CALLBACK.encode()).hexdigest()[:16])
    if not os.path.exists(so):              # a --cache directory keeps it between runs
        src = os.path.join(work, "diag_cb.hip")
        with open(src, "w") as f:
            f.write(CALLBACK)
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        tmp = "%s.%d.tmp" % (so, os.getpid())
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", tmp], check=True,
                       capture_output=True, timeout=900)
        os.replace(tmp, so)
    _lib.load()
    lib = C.CDLL(so)
    lib.diag_setup.restype = C.c_void_p
    lib.diag_setup.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="fused,kernel,builtin")
    ap.add_argument("--shapes", default="65536x64,4096x16,1048576x32")
    ap.add_argument("--seconds", type=float, default=1.5)
    ap.add_argument("--flags", default="", help="further hipcc flags of the fused launcher, separated by blanks")
    ap.add_argument("--nblobs", default="", help="blob counts: each adds a mode fused+K (the five-argument functor)")
    ap.add_argument("--store", action="store_true", help="store the chain (and the blobs): the sampler is reset before every block")
    ap.add_argument("--cache", default=None, help="directory of compiled user libraries (default: a temporary one)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--block", type=int, default=0, help="steps a timed block (default: some tens of milliseconds of the large shapes, 2 000 at most)")
    ap.add_argument("--rng", default="philox", choices=["philox", "mt19937"])
    ap.add_argument("--moves", default="stretch", choices=["stretch", "de+snooker"])
    a = ap.parse_args()
    modes = a.modes.split(",") + ["fused+%d" % int(k) for k in a.nblobs.split(",") if k]
    work = a.cache or tempfile.mkdtemp(prefix="ensemble_fused_bench_")
    os.makedirs(work, exist_ok=True)
    cb = build_callback(work)
    lines = []
    for shape in a.shapes.split(","):
        N, D = (int(v) for v in shape.split("x"))
        rs = np.random.RandomState(7)
        mu = np.ascontiguousarray(0.3 * rs.randn(D))
        ivar = np.ascontiguousarray(1.0 / (0.5 + rs.rand(D)) ** 2)
        p0 = mu + rs.randn(N, D) / np.sqrt(ivar)
        dev = cb.diag_setup(mu.ctypes.data, ivar.ctypes.data, D)
        assert dev
        samplers = {}
        for mode in modes:
            kw = {}
            if mode in ("fused", "fused_small", "fused_general"):
                lib = targets.compile_fused_ensemble(MODEL, "DiagModel", D, flags=a.flags.split(), cache_dir=work)
                t = lib.target(user=dev)
            elif mode.startswith("fused+"):
                K = int(mode[6:])
                lib = targets.compile_fused_ensemble(MODEL, "DiagModel", D, flags=a.flags.split() + ["-DBENCH_NBLOBS=%d" % K], cache_dir=work,
                                                     nblobs=K)
                t = lib.target(user=dev)
            elif mode == "host":
                def t(p, mu=mu, ivar=ivar):
                    lp = -0.5 * np.sum(ivar * (p - mu) ** 2, axis=1)
                    return np.column_stack([lp, lp])
                kw = dict(vectorize=True)
            elif mode == "kernel":
                t = targets.DeviceKernel(cb.diag_rows, dev)
            else:
                t = targets.DiagGaussian(mu, ivar)
            if a.moves == "de+snooker":
                kw["moves"] = [(emcee_amd.moves.DEMove(), 0.6), (emcee_amd.moves.DESnookerMove(), 0.4)]
            s = emcee_amd.EnsembleSampler(N, D, t, rng=a.rng, **kw)
            s._random.seed(3)
            if mode in ("fused_small", "fused_general"):
                s._device_ensemble().set_tuning("small_kernel", 2 if mode == "fused_small" else 0)
            samplers[mode] = [s, s.run_mcmc(p0, 16, store=a.store, skip_initial_state_check=True), [], 16]
        block = max(32, min(2000, int(6.4e9 / (N * D)) // 16 * 16))      # some tens of milliseconds a block
        if a.block > 0:
            block = a.block
        if a.store:
            block = max(16, min(block, int(4e9 / (N * D * 8)) // 16 * 16))

        def run(ent, n):
            if a.store:
                ent[0].reset()
            ent[1] = ent[0].run_mcmc(ent[1], n, store=a.store, skip_initial_state_check=True)
        t_end = time.perf_counter() + 0.5                    # clocks up, every mode warm
        while time.perf_counter() < t_end:
            for mode in modes:
                ent = samplers[mode]
                run(ent, block if mode != "host" else 4)
                ent[3] += block
        spent = dict((m, 0.0) for m in modes)
        while min(spent.values()) < a.seconds:
            for mode in modes:                               # alternating
                ent = samplers[mode]
                nb = block if mode != "host" else 4          # (milliseconds a step: a few steps are a block)
                if a.store:
                    ent[0].reset()
                ent[0]._ens.sync()
                t0 = time.perf_counter()
                ent[1] = ent[0].run_mcmc(ent[1], nb, store=a.store, skip_initial_state_check=True)
                ent[0]._ens.sync()
                dt = time.perf_counter() - t0
                ent[2].append(dt / nb)
                ent[3] += nb
                spent[mode] += dt
        for mode in modes:
            v = np.sort(np.array(samplers[mode][2])) * 1e6
            acc = float(np.mean(samplers[mode][0]._ens.accepted_mask()))
            ens = samplers[mode][0]._ens
            small = ens.small_info()["launches"] if hasattr(ens, "small_info") else None
            rec = dict(shape=shape, mode=mode, rng=a.rng, moves=a.moves, small_launches=small, flags=a.flags, store=bool(a.store), us_per_step=float(np.median(v)), p10=float(v[int(0.1 * (len(v) - 1))]),
                       p90=float(v[int(np.ceil(0.9 * (len(v) - 1)))]), blocks=len(v), steps_per_block=block if mode != "host" else 4, steps_total=samplers[mode][3],
                       last_accept_fraction=acc)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        for mode in modes:
            samplers[mode][0]._ens.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
