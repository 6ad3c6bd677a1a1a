"""us per step of ONE likelihood that sums over data -- the straight-line fit of tests/c/user_ensemble_fused_data.hip, model (a):
a flat box prior and  -0.5 ((y_k - m t_k - b) / sigma_k)^2  over ndata points behind `user` -- run through EnsembleSampler as

  data     targets.DeviceFused(..., ndata=): base / term compiled by EMX_FUSED_ENSEMBLE_DATA_TARGET, a wave a row in the data sum,
           the rows a workgroup takes chosen by the library's rule
  data@R   the same with the tuning key fused_data_rows = R (--rows 4,8,16,32,64 adds one such mode per count, clamped to the tile)
  serial   the same model as a plain EMX_FUSED_ENSEMBLE_TARGET functor: ONE lane a row loops over the data, in the order the data
           target defines (64 partials, then the pairwise tree), so both produce the same chain.  This is what a user had before.
  loop     the plain functor as a user would write it without that order in mind: one accumulator, k ascending (other bits)

    python tools/ensemble_fused_data_bench.py [--modes data,serial] [--shapes 1024x5,4096x16,65536x8] [--ndata 64,1024,16384]
                                              [--rows 4,8,16,32,64] [--seconds 1.0] [--block STEPS] [--cache DIR] [--out FILE]
                                              [--flags="-IDIR ..."]

`--modes serial,loop` needs nothing of the data target, so the same file measures a checkout that predates it.  Blocks of steps timed by
a host clock around a device synchronise; the median and the p10 ... p90 spread of at least `--seconds` of blocks per mode (at least
20 blocks where another mode is so slow that it has taken ten times `--seconds` by then), the modes of a shape taken in alternation
so that drift of the machine hits them alike.  store=False.  Prints one JSON line per shape, ndata and
mode; `--flags` are further compiler flags of the launchers (--flags=-IDIR puts another copy of the headers ahead of the library's);
with both `data` and `serial` among the modes the two final states are compared (they must be equal bit for bit)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import emcee_amd  # noqa: E402
from emcee_amd import targets  # noqa: E402

MODEL = r"""
struct line_data { const double* d; long long n; double box; };      // d: (3, n) t, y, sigma
struct LineModel {
    __device__ double base(const double* x, int ndim, const void* user) const {
        const line_data* u = (const line_data*)user;
        for (int d = 0; d < ndim; ++d)
            if (!(x[d] >= -u->box && x[d] <= u->box)) return -__builtin_inf();
        return 0.0;
    }
    __device__ double term(const double* x, int ndim, long long k, const void* user) const {
        const line_data* u = (const line_data*)user;
        double r = u->d[u->n + k] - x[0] * u->d[k];
        if (ndim > 1) r = r - x[1];
        r = r / u->d[2 * u->n + k];
        return -0.5 * (r * r);
    }
};
"""
# one lane a row, the defined order written serially (the 64 partials stay in registers: every index is a constant)
SERIAL = MODEL + r"""
struct LineSerial {
    __device__ double operator()(const double* x, int ndim, int, const void* user) const {
        const LineModel m;
        const double b = m.base(x, ndim, user);
        if (b != b || b == -__builtin_inf()) return b;
        const long long ndata = ((const line_data*)user)->n;
        double p[64];
#pragma unroll
        for (int l = 0; l < 64; ++l) p[l] = 0.0;
        for (long long k0 = 0; k0 < ndata; k0 += 64) {
#pragma unroll
            for (int l = 0; l < 64; ++l)
                if (k0 + l < ndata) p[l] = p[l] + m.term(x, ndim, k0 + l, user);
        }
#pragma unroll
        for (int w = 64; w > 1; w /= 2)
#pragma unroll
            for (int l = 0; l < w / 2; ++l) p[l] = p[2 * l] + p[2 * l + 1];
        return b + p[0];
    }
};
"""
# one lane a row, one accumulator
LOOP = MODEL + r"""
struct LineLoop {
    __device__ double operator()(const double* x, int ndim, int, const void* user) const {
        const LineModel m;
        const double b = m.base(x, ndim, user);
        if (b != b || b == -__builtin_inf()) return b;
        const long long ndata = ((const line_data*)user)->n;
        double acc = 0.0;
        for (long long k = 0; k < ndata; ++k) acc = acc + m.term(x, ndim, k, user);
        return b + acc;
    }
};
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="data,serial")
    ap.add_argument("--shapes", default="1024x5,4096x16,65536x8")
    ap.add_argument("--ndata", default="64,1024,16384")
    ap.add_argument("--rows", default="", help="rows a workgroup: each adds a mode data@R (tuning key fused_data_rows)")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--block", type=int, default=0, help="steps a timed block (default: about 20 ms of the slowest mode, 8 ... 2 000)")
    ap.add_argument("--cache", default=None, help="directory of compiled user libraries (default: a temporary one)")
    ap.add_argument("--flags", default="", help="further hipcc flags of the launchers, separated by blanks")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    modes = [m for m in a.modes.split(",") if m] + ["data@%d" % int(r) for r in a.rows.split(",") if r]
    work = a.cache or tempfile.mkdtemp(prefix="ensemble_fused_data_bench_")
    os.makedirs(work, exist_ok=True)
    lines = []
    for shape in a.shapes.split(","):
        N, D = (int(v) for v in shape.split("x"))
        libs = {}
        for mode in modes:
            kind = mode if mode in ("serial", "loop") else "data"
            if kind not in libs:
                libs[kind] = (targets.compile_fused_ensemble(SERIAL, "LineSerial", D, cache_dir=work, small=False, flags=a.flags.split()) if kind == "serial" else
                              targets.compile_fused_ensemble(LOOP, "LineLoop", D, cache_dir=work, small=False, flags=a.flags.split()) if kind == "loop" else
                              targets.compile_fused_ensemble(MODEL, "LineModel", D, cache_dir=work, data=True, flags=a.flags.split()))
        for ndata in (int(v) for v in a.ndata.split(",")):
            rs = np.random.RandomState(7)
            t = np.linspace(-1.0, 1.0, max(ndata, 2))[:ndata]
            sigma = 1.5 * np.sqrt(max(ndata, 16) / 200.0) * (1.0 + 0.5 * rs.rand(ndata))
            data = torch.as_tensor(np.ascontiguousarray(np.stack([t, 0.2 + 0.5 * t + sigma * rs.randn(ndata), sigma]))).cuda()
            desc = np.zeros(3, dtype=np.int64)                 # line_data: pointer, count, box
            desc[0], desc[1] = data.data_ptr(), ndata
            desc[2:].view(np.float64)[0] = 2.5
            user = torch.as_tensor(desc).cuda()
            p0 = 0.1 * rs.randn(N, D)
            samplers = {}
            for mode in modes:
                t_ = libs[mode].target(user=user) if mode in ("serial", "loop") else libs["data"].target(user=user, ndata=ndata)
                s = emcee_amd.EnsembleSampler(N, D, t_, rng="philox")
                s._random.seed(3)
                if "@" in mode:
                    s._device_ensemble().set_tuning("fused_data_rows", int(mode.split("@")[1]))
                st = s.run_mcmc(p0, 4, store=False, skip_initial_state_check=True)      # first launches: modules load, buffers grow
                s._ens.sync()
                t0 = time.perf_counter()
                st = s.run_mcmc(st, 8, store=False, skip_initial_state_check=True)
                s._ens.sync()
                samplers[mode] = [s, st, [], 12, (time.perf_counter() - t0) / 8]
            block = a.block if a.block > 0 else max(8, min(2000, int(0.02 / max(e[4] for e in samplers.values()))))
            t_end = time.perf_counter() + 0.3                    # clocks up, every mode warm
            while time.perf_counter() < t_end:
                for mode in modes:
                    ent = samplers[mode]
                    ent[1] = ent[0].run_mcmc(ent[1], block, store=False, skip_initial_state_check=True)
                    ent[3] += block
            spent = dict((m, 0.0) for m in modes)
            # until every mode has `--seconds` of blocks -- or, where one mode is tens of times slower than another, until the slowest
            # has ten times that and every mode at least 20 blocks
            while min(spent.values()) < a.seconds and not (max(spent.values()) >= 10.0 * a.seconds and
                                                            min(len(e[2]) for e in samplers.values()) >= 20):
                for mode in modes:                               # alternating
                    ent = samplers[mode]
                    ent[0]._ens.sync()
                    t0 = time.perf_counter()
                    ent[1] = ent[0].run_mcmc(ent[1], block, store=False, skip_initial_state_check=True)
                    ent[0]._ens.sync()
                    dt = time.perf_counter() - t0
                    ent[2].append(dt / block)
                    ent[3] += block
                    spent[mode] += dt
            same = None
            if "data" in samplers and "serial" in samplers:      # the same number of steps from the same start: the same state
                same = bool(np.array_equal(samplers["data"][1].coords, samplers["serial"][1].coords) and
                            np.array_equal(samplers["data"][1].log_prob, samplers["serial"][1].log_prob))
            for mode in modes:
                v = np.sort(np.array(samplers[mode][2])) * 1e6
                ens = samplers[mode][0]._ens
                rec = dict(shape=shape, ndata=ndata, mode=mode, us_per_step=float(np.median(v)), p10=float(v[int(0.1 * (len(v) - 1))]),
                           p90=float(v[int(np.ceil(0.9 * (len(v) - 1)))]), blocks=len(v), steps_per_block=block, steps_total=samplers[mode][3],
                           last_accept_fraction=float(np.mean(ens.accepted_mask())), small_launches=ens.small_info()["launches"],
                           same_state_as_serial=same if mode == "data" else None)
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
            for mode in modes:
                samplers[mode][0]._ens.close()
            del user, data
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
