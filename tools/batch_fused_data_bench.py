"""Member-steps per second of ONE likelihood that sums over per-member data -- a straight-line fit,  -0.005 |theta|^2  plus
-0.5 ivar_k (y_k - theta_0 - theta_1 x_k)^2  over the member's ndata points behind `user` -- run through EnsembleBatch as

  data     targets.BatchFused(..., ndata=): base / term compiled by EMX_FUSED_BATCH_DATA_TARGET, a wave a row in the data sum
  loop     the same model as a plain EMX_FUSED_BATCH_TARGET functor as a user would write it: ONE lane a row, one accumulator, k
           ascending (other bits).  What a user had before; the fair baseline.
  serial   the plain functor summing in the order the data target defines (64 partials, then the pairwise tree): the data target's
           chain, one lane a row

    python tools/batch_fused_data_bench.py [--modes data,loop,serial] [--batches 64,1024] [--shapes 32x5,100x10]
                                           [--ndata 16,64,256,1024,4096,ragged] [--seconds 0.5] [--cache DIR] [--out FILE.jsonl]
    python tools/batch_fused_data_bench.py --unchanged --label NAME [--out FILE.jsonl]
    python tools/batch_fused_data_bench.py --report FILE.jsonl [FILE.jsonl ...] --md profiles/batch_fused_data.md

`ragged`: every member's count drawn uniformly from 16 ... 1 024.  `--modes loop,serial` and `--unchanged` need nothing of the data
target, so the same file measures a checkout that predates it.  `--unchanged`: the paths that share SmallRunArgs with the data form
and run none of it -- the built-in DiagGaussian and a plain BatchFused diagonal model at 1 024 members of 32 x 5 -- labelled NAME.

Procedure: blocks of steps (about 20 ms each, store=False) timed by a host clock around run_mcmc, which returns the state and so
waits for the device; first launches and 0.2 s of blocks are warm-up; then the modes of a case are taken in alternation, so that
drift of the machine hits them alike, until each has `--seconds` of blocks (or the slowest has ten times that and each at least 12
blocks).  Reported: the median and the p10 ... p90 spread over the blocks.  One JSON line per case and mode."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from emcee_amd import EnsembleBatch, targets  # noqa: E402

MODEL = r"""
struct line_rec { const double* x; const double* y; const double* ivar; long long n; };
__device__ inline double line_base(const double* th, int ndim) {
    double acc = 0.0;
    for (int d = 0; d < ndim; ++d) acc = acc + th[d] * th[d];
    return -0.005 * acc;
}
__device__ inline double line_term(const double* th, const line_rec* r, long long k) {
    const double d = r->y[k] - (th[0] + th[1] * r->x[k]);
    return -0.5 * (r->ivar[k] * d * d);
}
"""
DATA = MODEL + r"""
struct LineData {
    __device__ double base(const double* x, int ndim, int member, const void* user) const { return line_base(x, ndim); }
    __device__ double term(const double* x, int ndim, int member, long long k, const void* user) const {
        return line_term(x, (const line_rec*)user + member, k);
    }
};
"""
LOOP = MODEL + r"""
struct LineLoop {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const {
        const line_rec* r = (const line_rec*)user + member;
        double acc = 0.0;
        for (long long k = 0; k < r->n; ++k) acc = acc + line_term(x, r, k);
        return line_base(x, ndim) + acc;
    }
};
"""
# the defined order written serially (the 64 partials stay in registers: every index is a constant)
SERIAL = MODEL + r"""
struct LineSerial {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const {
        const line_rec* r = (const line_rec*)user + member;
        double p[64];
#pragma unroll
        for (int l = 0; l < 64; ++l) p[l] = 0.0;
        for (long long k0 = 0; k0 < r->n; k0 += 64) {
#pragma unroll
            for (int l = 0; l < 64; ++l)
                if (k0 + l < r->n) p[l] = p[l] + line_term(x, r, k0 + l);
        }
#pragma unroll
        for (int w = 64; w > 1; w /= 2)
#pragma unroll
            for (int l = 0; l < w / 2; ++l) p[l] = p[2 * l] + p[2 * l + 1];
        return line_base(x, ndim) + p[0];
    }
};
"""
DIAG = r"""
struct DiagPlain {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const {
        const double* mu = (const double*)user + (long long)member * 2 * ndim;
        const double* ivar = mu + ndim;
        double acc = 0.0;
        for (int d = 0; d < ndim; ++d) {
            const double r = x[d] - mu[d];
            acc = acc + ivar[d] * r * r;
        }
        return -0.5 * acc;
    }
};
"""


def measure(batches, seconds, rate_of):
    """batches: {mode: EnsembleBatch, already given its first state}; -> {mode: (blocks of member-steps/s, steps a block)}"""
    ent = {}
    for mode, bt in batches.items():
        bt.run_mcmc(None, 4, store=False)                   # first launches: modules load, buffers grow
        t0 = time.perf_counter()
        bt.run_mcmc(None, 8, store=False)
        ent[mode] = [bt, [], (time.perf_counter() - t0) / 8]
    block = max(4, min(2000, int(0.02 / max(e[2] for e in ent.values()))))
    t_end = time.perf_counter() + 0.2                       # clocks up, every mode warm
    while time.perf_counter() < t_end:
        for e in ent.values():
            e[0].run_mcmc(None, block, store=False)
    spent = dict((m, 0.0) for m in ent)
    while min(spent.values()) < seconds and not (max(spent.values()) >= 10.0 * seconds and min(len(e[1]) for e in ent.values()) >= 12):
        for mode, e in ent.items():                         # alternating
            t0 = time.perf_counter()
            e[0].run_mcmc(None, block, store=False)
            dt = time.perf_counter() - t0
            e[1].append(rate_of(block, dt))
            spent[mode] += dt
    return dict((m, (np.sort(np.array(e[1])), block)) for m, e in ent.items())


def stats(v):
    return dict(median=float(np.median(v)), p10=float(v[int(0.1 * (len(v) - 1))]), p90=float(v[int(np.ceil(0.9 * (len(v) - 1)))]), blocks=len(v))


def run_cases(a):
    import torch
    modes = [m for m in a.modes.split(",") if m]
    work = a.cache or tempfile.mkdtemp(prefix="batch_fused_data_bench_")
    lines = []
    for shape in a.shapes.split(","):
        N, D = (int(v) for v in shape.split("x"))
        libs = {}
        for mode in modes:
            libs[mode] = (targets.compile_fused(DATA, "LineData", D, cache_dir=work, data=True) if mode == "data" else
                          targets.compile_fused(LOOP, "LineLoop", D, cache_dir=work) if mode == "loop" else
                          targets.compile_fused(SERIAL, "LineSerial", D, cache_dir=work))
        if a.compile_only:
            continue
        for B in (int(v) for v in a.batches.split(",")):
            for nd in a.ndata.split(","):
                rs = np.random.RandomState(7)
                counts = rs.randint(16, 1025, size=B) if nd == "ragged" else np.full(B, int(nd))
                off = np.concatenate([[0], np.cumsum(counts)])
                x = np.concatenate([np.linspace(-1.0, 1.0, n) for n in counts])
                sigma = 1.5 * np.sqrt(np.repeat(counts, counts) / 200.0) * (1.0 + 0.5 * rs.rand(off[-1]))
                y = 0.2 + 0.5 * x + sigma * rs.randn(off[-1])
                dev = torch.as_tensor(np.ascontiguousarray(np.stack([x, y, 1.0 / (sigma * sigma)]))).cuda()
                rec = np.zeros((B, 4), dtype=np.int64)
                for k in range(3):
                    rec[:, k] = dev.data_ptr() + 8 * (k * off[-1] + off[:-1])
                rec[:, 3] = counts
                user = torch.as_tensor(rec).cuda()
                p0 = 0.1 * rs.randn(B, N, D)
                batches = {}
                for mode in modes:
                    t = libs[mode].target(user=user, ndata=[int(n) for n in counts]) if mode == "data" else libs[mode].target(user=user)
                    bt = EnsembleBatch(B, N, D, t, seeds=list(range(1, B + 1)))
                    bt.run_mcmc(p0, 0, skip_initial_state_check=True)
                    batches[mode] = bt
                res = measure(batches, a.seconds, lambda block, dt: B * block / dt)
                same = None
                if "data" in batches and "serial" in batches:      # the same number of steps from the same start: the same state
                    u, v = batches["data"].get_last_sample(), batches["serial"].get_last_sample()
                    same = bool(np.array_equal(u.coords, v.coords) and np.array_equal(u.log_prob, v.log_prob))
                for mode in modes:
                    v, block = res[mode]
                    info = batches[mode].launch_info()
                    lines.append(json.dumps(dict(kind="case", B=B, shape=shape, ndata=nd, mode=mode, member_steps_per_s=stats(v), steps_per_block=block,
                                                 threads=info["threads"], plan_steps=info["plan_steps"],
                                                 same_state_as_serial=same if mode == "data" else None)))
                    print(lines[-1], flush=True)
                for bt in batches.values():
                    bt.close()
                del user, dev
    return lines


def run_unchanged(a):
    import torch
    B, N, D = 1024, 32, 5
    work = a.cache or tempfile.mkdtemp(prefix="batch_fused_data_bench_")
    lib = targets.compile_fused(DIAG, "DiagPlain", D, cache_dir=work)
    if a.compile_only:
        return []
    rs = np.random.RandomState(3)
    mu, ivar = 0.1 * rs.randn(B, D), 1.0 / (0.2 + rs.rand(B, D))
    user = torch.as_tensor(np.ascontiguousarray(np.concatenate([mu, ivar], axis=1))).cuda()
    p0 = rs.randn(B, N, D)
    batches = {"builtin DiagGaussian": EnsembleBatch(B, N, D, [targets.DiagGaussian(mu[b], ivar[b]) for b in range(B)], seeds=list(range(1, B + 1))),
               "plain BatchFused diag": EnsembleBatch(B, N, D, lib.target(user=user), seeds=list(range(1, B + 1)))}
    for bt in batches.values():
        bt.run_mcmc(p0, 0, skip_initial_state_check=True)
    res = measure(batches, a.seconds, lambda block, dt: B * block / dt)
    lines = []
    for mode, (v, block) in res.items():
        lines.append(json.dumps(dict(kind="unchanged", label=a.label, B=B, shape="%dx%d" % (N, D), mode=mode, member_steps_per_s=stats(v), steps_per_block=block)))
        print(lines[-1], flush=True)
    for bt in batches.values():
        bt.close()
    return lines


def fmt(s):
    return "%.3g (%.3g ... %.3g)" % (s["median"], s["p10"], s["p90"])


def report(files, md):
    recs = [json.loads(ln) for f in files for ln in open(f) if ln.strip().startswith("{")]
    cases, unch = [r for r in recs if r["kind"] == "case"], [r for r in recs if r["kind"] == "unchanged"]
    out = ["# EnsembleBatch: fused likelihoods that sum over per-member data", "",
           "Written by `tools/batch_fused_data_bench.py --report` from its own measurements on one MI355X; the procedure is in that file's",
           "docstring.  Member-steps/s: median (p10 ... p90) over blocks of about 20 ms, the modes of a case in alternation.  `data`: the",
           "wave-a-row data target; `loop`: the same model as a one-lane functor with one accumulator (what a user had before: the fair",
           "baseline, other bits); `serial`: the one-lane functor summing in the data target's order (the same chain).", ""]
    keys = []
    for r in cases:
        k = (r["B"], r["shape"])
        if k not in keys:
            keys.append(k)
    pays = []
    for B, shape in keys:
        out += ["## B = %d, %s" % (B, shape), "", "| ndata | data | loop | serial | data / loop | data / serial | threads (data / loop) | same state as serial |",
                "|---|---|---|---|---|---|---|---|"]
        first = None
        for nd in [r["ndata"] for r in cases if (r["B"], r["shape"]) == (B, shape) and r["mode"] == cases[0]["mode"]]:
            m = dict((r["mode"], r) for r in cases if (r["B"], r["shape"], r["ndata"]) == (B, shape, nd))
            g = lambda k: m[k]["member_steps_per_s"] if k in m else None  # noqa: E731
            ratio = lambda p, q: "%.2f" % (g(p)["median"] / g(q)["median"]) if g(p) and g(q) else "-"  # noqa: E731
            out.append("| %s | %s | %s | %s | %s | %s | %s / %s | %s |" % (
                nd, *[fmt(g(k)) if g(k) else "-" for k in ("data", "loop", "serial")], ratio("data", "loop"), ratio("data", "serial"),
                m["data"]["threads"] if "data" in m else "-", m["loop"]["threads"] if "loop" in m else "-",
                m["data"]["same_state_as_serial"] if "data" in m else "-"))
            if first is None and nd != "ragged" and g("data") and g("loop") and g("data")["median"] > g("loop")["median"]:
                first = nd
        pays.append("- B = %d, %s: the data form first beats the one-accumulator loop at ndata = %s" % (B, shape, first if first else "(none measured)"))
        out.append("")
    out += ["## Where the data form first pays", ""] + pays + [""]
    if unch:
        out += ["## The unchanged paths (SmallRunArgs grew by one pointer)", "",
                "1 024 members of 32 x 5, the parent commit's build and this one's in alternating processes on the same machine; each row one",
                "process.  The paths count as unchanged if the builds differ by less than the parent's own run-to-run spread.", "",
                "| build | path | member-steps/s |", "|---|---|---|"]
        for r in unch:
            out.append("| %s | %s | %s |" % (r["label"], r["mode"], fmt(r["member_steps_per_s"])))
        out.append("")
        for mode in sorted({r["mode"] for r in unch}):
            by = {}
            for r in unch:
                if r["mode"] == mode:
                    by.setdefault(r["label"], []).append(r["member_steps_per_s"]["median"])
            desc = ["%s: medians %s" % (lb, ", ".join("%.4g" % v for v in vs)) for lb, vs in sorted(by.items())]
            out.append("- %s -- %s" % (mode, "; ".join(desc)))
            if len(by) == 2 and "parent" in by:
                par = by["parent"]
                new = by[[k for k in by if k != "parent"][0]]
                spread = (max(par) - min(par)) / np.mean(par)
                diff = (np.mean(new) - np.mean(par)) / np.mean(par)
                out.append("  - parent run-to-run spread (max - min over its processes): %.2f %%; this build against the parent (means): %+.2f %%: %s"
                           % (100 * spread, 100 * diff, "unchanged" if abs(diff) <= spread else "NOT inside the spread"))
        out.append("")
    with open(md, "w") as f:
        f.write("\n".join(out))
    print("wrote %s" % md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="data,loop,serial")
    ap.add_argument("--batches", default="64,1024")
    ap.add_argument("--shapes", default="32x5,100x10")
    ap.add_argument("--ndata", default="16,64,256,1024,4096,ragged")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--cache", default=None, help="directory of compiled user libraries (default: a temporary one)")
    ap.add_argument("--compile-only", action="store_true", help="fill --cache and stop: needs no GPU")
    ap.add_argument("--unchanged", action="store_true")
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=None, help="JSON lines are appended to this file")
    ap.add_argument("--report", nargs="+", default=None)
    ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "batch_fused_data.md"))
    a = ap.parse_args()
    if a.report:
        return report(a.report, a.md)
    lines = run_unchanged(a) if a.unchanged else run_cases(a)
    if a.out and lines:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
