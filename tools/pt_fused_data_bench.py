"""us per proposal step of PTSampler on ONE likelihood that sums over an object's data -- a straight-line fit,
-0.005 |theta|^2 - 0.5 sum_k ivar_k (y_k - theta_0 - theta_1 x_k)^2  over ndata points behind `user`, a box prior on the handle -- as

  data     targets.PTFused(..., ndata=): base / term compiled by EMX_FUSED_PT_DATA_TARGET, a wave a row in the data sum
  loop     the same model as a plain EMX_FUSED_PT_TARGET functor the way a user writes it without the data form: ONE lane a row
           loops over the data, one accumulator, k ascending (other bits than `data`: another order of the sum)

    python tools/pt_fused_data_bench.py [--modes data,loop] [--shapes 1x8x32x5,16x8x32x5,256x8x32x5,16x8x64x16]
                                        [--ndata 16,64,256,1024,4096] [--seconds 0.4] [--cache DIR] [--out FILE] [--md FILE]

A shape is nbatch x ntemps x nwalkers x ndim; every object has its own ndata points.  The default ladder, a swap pass after every
step, the StretchMove, store=False.  Each mode is warmed up (first launches, then 0.2 s of chunks), then chunks of steps are timed by
a host clock around run_mcmc (which returns the state, so the device has finished), the modes of a cell taken in alternation so that
drift of the machine hits them alike; the figure is the median over at least `--seconds` of chunks a mode, with the p10 ... p90
spread.  `--modes loop` needs nothing of the data form, so the same file measures a checkout that predates it.  Prints one JSON line
per shape, ndata and mode; `--md` writes the table (and the command) as markdown."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from emcee_amd import PTSampler, targets  # noqa: E402

MODEL = r"""
struct line_rec { const double* d; long long n; long long ntemps; };      // d: (3, n) x, y, ivar of one object
__device__ inline const line_rec* line_of(const void* user, int member) {
    const line_rec* r = (const line_rec*)user;
    return r + member / r->ntemps;
}
struct LineModel {
    __device__ double base(const double* x, int ndim, int member, const void* user) const {
        double acc = 0.0;
        for (int d = 0; d < ndim; ++d) acc = acc + x[d] * x[d];
        return -0.005 * acc;
    }
    __device__ double term(const double* x, int ndim, int member, long long k, const void* user) const {
        const line_rec* r = line_of(user, member);
        const double d = r->d[r->n + k] - (x[0] + x[1] * r->d[k]);
        return -0.5 * (r->d[2 * r->n + k] * d * d);
    }
};
// one lane a row, one accumulator
struct LineLoop {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const {
        const LineModel m;
        const double b = m.base(x, ndim, member, user);
        const long long ndata = line_of(user, member)->n;
        double acc = 0.0;
        for (long long k = 0; k < ndata; ++k) acc = acc + m.term(x, ndim, member, k, user);
        return b + acc;
    }
};
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="data,loop")
    ap.add_argument("--shapes", default="1x8x32x5,16x8x32x5,256x8x32x5,16x8x64x16")
    ap.add_argument("--ndata", default="16,64,256,1024,4096")
    ap.add_argument("--seconds", type=float, default=0.4)
    ap.add_argument("--cache", default=None, help="directory of compiled user libraries (default: a temporary one)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None, help="write the table as markdown")
    a = ap.parse_args()
    modes = [m for m in a.modes.split(",") if m]
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    counts = [int(v) for v in a.ndata.split(",")]
    work = a.cache or tempfile.mkdtemp(prefix="pt_fused_data_bench_")
    os.makedirs(work, exist_ok=True)
    libs = {}
    for D in sorted({s[3] for s in shapes}):
        for mode in modes:
            libs[mode, D] = (targets.compile_fused_pt(MODEL, "LineModel", D, cache_dir=work, data=True) if mode == "data" else
                             targets.compile_fused_pt(MODEL, "LineLoop", D, cache_dir=work))
    import torch
    lines, cells = [], {}
    for shape in shapes:
        G, T, N, D = shape
        for ndata in counts:
            rs = np.random.RandomState(7)
            x = np.broadcast_to(np.linspace(-1.0, 1.0, ndata), (G, ndata))
            sigma = 1.5 * np.sqrt(max(ndata, 16) / 200.0) * (1.0 + 0.5 * rs.rand(G, ndata))
            data = torch.as_tensor(np.ascontiguousarray(np.stack([x, 0.2 + 0.5 * x + sigma * rs.randn(G, ndata), 1.0 / (sigma * sigma)], axis=1))).cuda()
            rec = np.zeros((G, 3), dtype=np.int64)              # line_rec: pointer, count, rungs an object
            rec[:, 0] = data.data_ptr() + 8 * 3 * ndata * np.arange(G)
            rec[:, 1], rec[:, 2] = ndata, T
            user = torch.as_tensor(rec).cuda()
            p0 = 0.1 * rs.randn(G, T, N, D)
            run = {}
            for mode in modes:
                t_ = libs[mode, D].target(user=user, ndata=ndata) if mode == "data" else libs[mode, D].target(user=user)
                pt = PTSampler(T, N, D, t_, log_prior=(-3.0 * np.ones(D), 3.0 * np.ones(D)), nbatch=G, seeds=list(range(1, G + 1)))
                pt.run_mcmc(p0, 4, store=False, skip_initial_state_check=True)           # first launches: modules load, buffers grow
                t0 = time.perf_counter()
                pt.run_mcmc(None, 8, store=False)
                run[mode] = [pt, [], (time.perf_counter() - t0) / 8]
            for mode in modes:                                  # a chunk of about 30 ms, 8 ... 2 000 steps
                run[mode].append(max(8, min(2000, int(0.03 / run[mode][2]))))
            t_end = time.perf_counter() + 0.2                   # clocks up, every mode warm
            while time.perf_counter() < t_end:
                for mode in modes:
                    run[mode][0].run_mcmc(None, run[mode][3], store=False)
            spent = dict((m, 0.0) for m in modes)
            while min(spent.values()) < a.seconds:
                for mode in modes:                              # alternating
                    pt, times, _, chunk = run[mode]
                    t0 = time.perf_counter()
                    pt.run_mcmc(None, chunk, store=False)
                    dt = time.perf_counter() - t0
                    times.append(dt / chunk)
                    spent[mode] += dt
            for mode in modes:
                pt, times, _, chunk = run[mode]
                v = np.sort(np.array(times)) * 1e6
                info = pt.launch_info()
                r = dict(shape="x".join(map(str, shape)), ndata=ndata, mode=mode, us_per_step=float(np.median(v)),
                         p10=float(v[int(0.1 * (len(v) - 1))]), p90=float(v[int(np.ceil(0.9 * (len(v) - 1)))]), chunks=len(v),
                         steps_per_chunk=chunk, threads=info["threads"], plan_steps=info["plan_steps"])
                cells[shape, ndata, mode] = r
                lines.append(json.dumps(r))
                print(lines[-1], flush=True)
                pt.close()
            del user, data
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if a.md:
        with open(a.md, "w") as f:
            f.write("# PTSampler: the data form of a fused likelihood against the one-lane functor\n\n")
            f.write("Made by\n\n    python tools/pt_fused_data_bench.py %s\n\n" % " ".join(x for i, x in enumerate(sys.argv[1:]) if x != "--cache" and sys.argv[i] != "--cache"))
            f.write("us per proposal step (median of timed `run_mcmc` chunks, p10 ... p90 in brackets); `data / loop` below 1: the data form "
                    "is faster.\n\n")
            f.write("| nbatch x ntemps x nwalkers x ndim | ndata | " + " | ".join("%s us/step" % m for m in modes) +
                    (" | data / loop |" if "data" in modes and "loop" in modes else " |") + "\n")
            f.write("|---|---:|" + "---:|" * (len(modes) + (1 if "data" in modes and "loop" in modes else 0)) + "\n")
            for shape in shapes:
                for ndata in counts:
                    row = ["x".join(map(str, shape)), str(ndata)]
                    for m in modes:
                        r = cells[shape, ndata, m]
                        row.append("%.1f (%.1f ... %.1f)" % (r["us_per_step"], r["p10"], r["p90"]))
                    if "data" in modes and "loop" in modes:
                        row.append("%.2f" % (cells[shape, ndata, "data"]["us_per_step"] / cells[shape, ndata, "loop"]["us_per_step"]))
                    f.write("| " + " | ".join(row) + " |\n")


if __name__ == "__main__":
    main()
