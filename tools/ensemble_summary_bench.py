"""EnsembleSampler.get_summary (emx_summary: mean, covariance, three quantiles and MAP next to the chain) against the host path
it replaces on the same sampler: get_chain(flat=True) / get_log_prob(flat=True) and np.mean / np.cov / np.quantile / argmax.

Both are host clocks around calls that return with their results on the host.  The device call is timed once cold (scratch
allocated) and then at least 5 times and for at least `--seconds`: the median.  The host path is run once to warm up where a
call takes under `--host-budget` seconds, then 5 times (median); a slower one is timed `--host-calls-slow` times without a
warm-up.  Bytes are computed from the shapes; the reads of the selection come from emx_summary_info.
usage: python tools/ensemble_summary_bench.py [--quick] [--out ensemble_summary_bench.json] [--seconds 1] [--only K]"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from emcee_amd import EnsembleSampler, targets  # noqa: E402

QUANTILES = (0.16, 0.5, 0.84)
PEAK = 8e12
# nwalkers, ndim, target kind, stored rows
SHAPES = [(65536, 64, "dense", 50), (65536, 64, "dense", 200), (1048576, 8, "iso", 50), (4096, 16, "dense", 5000), (32, 5, "iso", 10000)]
QUICK = [(8192, 64, "dense", 8), (4096, 16, "dense", 100), (32, 5, "iso", 500)]


def make_sampler(N, D, kind, rows, rs):
    if kind == "iso":
        tg = targets.IsoGaussian()
    else:
        A = rs.randn(D, D)
        icov = np.linalg.inv(A @ A.T / D + 0.5 * np.eye(D))
        tg = targets.DenseGaussian(0.1 * rs.randn(D), 0.5 * (icov + icov.T))
    s = EnsembleSampler(N, D, tg, rng="philox")
    s.run_mcmc(rs.randn(N, D), rows, skip_initial_state_check=True)
    assert s.backend._dev is not None
    return s


def device_call(s):
    t0 = time.perf_counter()
    r = s.get_summary(quantiles=QUANTILES)
    return time.perf_counter() - t0, r


def host_call(s):
    t0 = time.perf_counter()
    x = s.get_chain(flat=True)
    lp = s.get_log_prob(flat=True)
    t_copy = time.perf_counter() - t0
    at = int(np.argmax(lp))
    r = (x.mean(axis=0), np.atleast_2d(np.cov(x.T)), np.quantile(x, QUANTILES, axis=0), x[at].copy(), lp[at])
    return time.perf_counter() - t0, t_copy, r


def bench(N, D, kind, rows, seconds, host_budget, host_calls_slow, rs):
    s = make_sampler(N, D, kind, rows, rs)
    cold, r = device_call(s)
    times, total = [], 0.0
    while total < seconds or len(times) < 5:
        t, r = device_call(s)
        times.append(t)
        total += t
    warm = float(np.median(times))
    sel_reads, listed, list_reads = s.backend._dev.summary_info()
    t, t_copy, h = host_call(s)
    if t < host_budget:
        runs = [host_call(s)[:2] for _ in range(5)]
    else:
        runs = [(t, t_copy)] + [host_call(s)[:2] for _ in range(host_calls_slow - 1)]
    host = float(np.median([u[0] for u in runs]))
    host_copy = float(np.median([u[1] for u in runs]))
    sel = rows * N * D * 8
    gram_reads = (((D + 15) // 16) * ((D + 15) // 16 + 1) // 2 + 31) // 32 if D >= 16 else 1
    moment_bytes = sel * (2 + gram_reads) + rows * N * 8
    order_bytes = sel * sel_reads + max(listed, 0) * 12 * (1 + list_reads)
    return dict(N=N, D=D, kind=kind, rows=rows, nsamples=r.nsamples, selection_GB=sel / 1e9, device_first_s=cold, device_warm_s=warm,
                device_calls_timed=len(times), host_s=host, host_copy_s=host_copy, host_calls_timed=len(runs), host_over_device=host / warm,
                reads_mean_cov_map=2 + gram_reads + 1.0 / D, reads_selection=sel_reads, listed_elements=listed, list_reads=list_reads,
                bytes_per_call_GB=(moment_bytes + order_bytes) / 1e9, GBps_warm=(moment_bytes + order_bytes) / warm / 1e9,
                share_of_8TBps=(moment_bytes + order_bytes) / warm / PEAK,
                max_abs_mean_diff=float(np.abs(r.mean - h[0]).max()), max_rel_cov_diff=float((np.abs(r.cov - h[1]) / np.abs(h[1]).max()).max()),
                max_abs_quantile_diff=float(np.abs(r.quantiles - h[2]).max()),
                map_equal=bool(np.array_equal(r.map_coords, h[3]) and r.map_log_prob == h[4]))


def main():
    arg = lambda flag, default, kind: kind(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default  # noqa: E731
    shapes = QUICK if "--quick" in sys.argv else SHAPES
    only = arg("--only", -1, int)
    if only >= 0:
        shapes = shapes[only:only + 1]
    out_path = arg("--out", "ensemble_summary_bench.json", str)
    rows = []
    for shape in shapes:
        r = bench(*shape, arg("--seconds", 1.0, float), arg("--host-budget", 5.0, float), arg("--host-calls-slow", 2, int), np.random.RandomState(1))
        print(json.dumps(r), flush=True)
        rows.append(r)
        with open(out_path, "w") as f:
            json.dump(rows, f, indent=1)
    print("\n| walkers x ndim | rows | selection GB | host s (copy s; calls) | device 1st s | device warm s (calls) | host / device | "
          "reads: mean+cov+MAP | reads: selection (+ list elements x reads) | GB per call | GB/s | of 8 TB/s |")
    print("|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|")
    for r in rows:
        print("| %d x %d %s | %d | %.3f | %.3f (%.3f; %d) | %.4f | %.5f (%d) | %.0fx | %.2f | %d (+ %d x %d) | %.2f | %.0f | %.1f %% |" % (
            r["N"], r["D"], r["kind"], r["rows"], r["selection_GB"], r["host_s"], r["host_copy_s"], r["host_calls_timed"], r["device_first_s"],
            r["device_warm_s"], r["device_calls_timed"], r["host_over_device"], r["reads_mean_cov_map"], r["reads_selection"],
            max(r["listed_elements"], 0), r["list_reads"], r["bytes_per_call_GB"], r["GBps_warm"], 100 * r["share_of_8TBps"]))


if __name__ == "__main__":
    main()
