"""EnsembleBatch.get_histograms (emx_chain_minmax_batch + emx_histograms_batch: every member's marginal histograms and pair panels
next to the chain) against the only path there was before it: get_chain(flat=True) and np.histogram / np.histogram2d per member,
and against the time of reading the selected bytes once at the bandwidth a streaming read achieves on an MI355X (6.3 TB/s).

The host path is timed on the first members of the batch (16 at 32 x 5, 2 at 256 x 32 with its 496 panels; `--host-members`
overrides both; one chain copy of that many members) and extrapolated linearly to B: it is the same work for every member.  The
device call is timed once cold (scratch allocated) and then repeatedly for at least `--seconds` (default 1 s) and at least 5 calls: the median, by the host clock around get_histograms, which returns with
the counts on the host.  The counts of the members timed on the host are compared with NumPy's (they must be equal).
usage: python tools/batch_histograms_bench.py [--quick] [--out batch_histograms_bench.json] [--host-members K] [--seconds 1]
       python tools/batch_histograms_bench.py --prof     (two device calls per case: for rocprofv3 --kernel-trace --stats)"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from emcee_amd import EnsembleBatch, moves, targets  # noqa: E402

ACHIEVABLE_BPS = 6.3e12          # a streaming read of HBM on an MI355X (8 TB/s nominal)
# name, B, nwalkers, ndim, stored steps, members timed on the host, the get_histograms calls timed on that batch
SHAPES = [("32x5", 1024, 32, 5, 5000, 16, [dict(bins=64, pairs=None), dict(bins=64, pairs="all")]),
          ("256x32", 64, 256, 32, 500, 2, [dict(bins=64, pairs=None), dict(bins=64, pairs="all", pair_bins=16)])]
QUICK = [("32x5", 64, 32, 5, 500, 4, [dict(bins=64, pairs=None), dict(bins=64, pairs="all")]),
         ("256x32", 4, 256, 32, 50, 1, [dict(bins=64, pairs=None), dict(bins=64, pairs="all", pair_bins=16)])]


def make_batch(B, N, D, steps, rs):
    bt = EnsembleBatch(B, N, D, targets.IsoGaussian(), moves=moves.StretchMove(), seeds=list(range(B)))
    bt.run_mcmc(rs.randn(B, N, D), steps, skip_initial_state_check=True)
    return bt


def device_call(bt, kw):
    t0 = time.perf_counter()
    r = bt.get_histograms(**kw)             # returns after the counts are on the host
    return time.perf_counter() - t0, r


def host_path(bt, k, kw):
    """what the caller does without get_histograms, for members [0, k) -> (counts, pair counts) as get_histograms shapes them"""
    x = bt._read(0, 0, k, 0, 1, True)                       # (k, n, D)
    D = x.shape[2]
    pb = kw.get("pair_bins") or min(kw["bins"], 64)
    pairs = [] if kw["pairs"] is None else [(i, j) for i in range(D) for j in range(i + 1, D)]
    counts = [np.stack([np.histogram(x[m, :, d], bins=kw["bins"])[0] for m in range(k)]) for d in range(D)]
    pc = [np.stack([np.histogram2d(x[m, :, i], x[m, :, j], bins=pb)[0].astype(np.int64) for m in range(k)]) for i, j in pairs]
    return counts, pc


def breakdown(bt, kw):
    """one more call with a clock around its two library calls -> (emx_chain_minmax_batch s, emx_histograms_batch s, whole call s)"""
    spent = {}

    def clocked(name):
        f = getattr(bt, name)

        def g(*a, **k):
            t0 = time.perf_counter()
            r = f(*a, **k)
            spent[name] = spent.get(name, 0.0) + time.perf_counter() - t0
            return r
        setattr(bt, name, g)
        return f
    saved = {name: clocked(name) for name in ("_minmax_device", "_hist_device")}
    whole = device_call(bt, kw)[0]
    for name, f in saved.items():
        setattr(bt, name, f)
    return spent["_minmax_device"], spent["_hist_device"], whole


def bench(name, B, N, D, steps, kw, bt, host_members, seconds):
    cold, r = device_call(bt, kw)
    times, total = [], 0.0
    while total < seconds or len(times) < 5:
        t, r = device_call(bt, kw)
        times.append(t)
        total += t
    warm, best = float(np.median(times)), float(np.min(times))
    t_minmax, t_count, t_whole = breakdown(bt, kw)
    launches = bt.histogram_launches() + 2                  # + emx_chain_minmax_batch's two (the range is every member's own)
    k = min(B, host_members)
    t0 = time.perf_counter()
    h_counts, h_pc = host_path(bt, k, kw)
    t_host_k = time.perf_counter() - t0
    equal = all(np.array_equal(a[:k], b) for a, b in zip(r.counts, h_counts)) and all(np.array_equal(a[:k], b) for a, b in zip(r.pair_counts, h_pc))
    chain_gb = B * steps * N * D * 8 / 1e9
    floor = 2 * chain_gb * 1e9 / ACHIEVABLE_BPS             # the call reads the selection twice: min / max, then the binning pass
    host_all = t_host_k * B / k
    out_mb = (sum(c.nbytes for c in r.counts) + sum(c.nbytes for c in r.pair_counts)) / 1e6
    return dict(shape=name, call=repr(kw), B=B, N=N, D=D, steps=steps, nsamples=r.nsamples, npairs=len(r.pairs), host_members_timed=k,
                host_s_timed=t_host_k, host_s_extrapolated=host_all, device_first_s=cold, device_warm_s=warm, device_min_s=best,
                device_calls_timed=len(times), speedup_warm=host_all / warm, chain_GB=chain_gb, read_once_s=floor / 2,
                read_twice_s=floor, warm_over_read_once=warm / (floor / 2), launches_per_call=launches, counts_MB_to_host=out_mb,
                minmax_call_s=t_minmax, count_call_s=t_count, host_edges_and_rest_s=t_whole - t_minmax - t_count,
                counts_equal_numpy=bool(equal))


def main():
    quick = "--quick" in sys.argv
    shapes = QUICK if quick else SHAPES
    if "--prof" in sys.argv:
        for name, B, N, D, steps, hm, calls in shapes:
            bt = make_batch(B, N, D, steps, np.random.RandomState(1))
            for kw in calls:
                for _ in range(2):
                    print(name, kw, "%.4f s" % device_call(bt, kw)[0], flush=True)
            bt.close()
        return
    arg = lambda flag, default, kind: kind(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default  # noqa: E731
    out_path = arg("--out", "batch_histograms_bench.json", str)
    host_members, seconds = arg("--host-members", 0, int), arg("--seconds", 1.0, float)
    rows = []
    for name, B, N, D, steps, hm, calls in shapes:
        bt = make_batch(B, N, D, steps, np.random.RandomState(1))
        for kw in calls:
            r = bench(name, B, N, D, steps, kw, bt, host_members or hm, seconds)
            print(json.dumps(r), flush=True)
            rows.append(r)
        bt.close()
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
    print("\n| shape | call | B | steps | chain GB | host s (timed members) | host s for B (extrapolated) | device 1st s | device warm s (calls) | "
          "host / warm | read once at 6.3 TB/s, s | warm / read once | launches | MB of counts | min/max call s | counting call s | equal NumPy |")
    print("|---|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---|")
    for r in rows:
        print("| %s | `%s` | %d | %d | %.2f | %.2f (%d) | %.1f | %.4f | %.4f (%d) | %.0fx | %.5f | %.1fx | %d | %.1f | %.4f | %.4f | %s |" % (
            r["shape"], r["call"], r["B"], r["steps"], r["chain_GB"], r["host_s_timed"], r["host_members_timed"], r["host_s_extrapolated"],
            r["device_first_s"], r["device_warm_s"], r["device_calls_timed"], r["speedup_warm"], r["read_once_s"], r["warm_over_read_once"],
            r["launches_per_call"], r["counts_MB_to_host"], r["minmax_call_s"], r["count_call_s"], r["counts_equal_numpy"]))


if __name__ == "__main__":
    main()
