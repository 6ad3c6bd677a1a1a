"""get_rhat (emx_rhat / emx_rhat_batch: split-R-hat next to the chain) against the host path it replaces -- get_chain() and
summary.split_rhat -- at the README's two chain shapes: 1 024 members of 32 x 5 with 5 000 stored steps (EnsembleBatch, both
groupings) and 65 536 x 64 with 200 stored steps (EnsembleSampler).  The yardstick for a reduction that passes over the chain
twice is get_summary(cov=False, quantiles=()) on the same handle: its mean kernels read the chain twice (and the log-probs once).

Device calls are timed once cold and then repeatedly for at least `--seconds` and at least 5 calls: the median; a call returns
after its results are on the host.  The host path: the batch's is timed on the first `--host-members` members in blocks of 64 and
extrapolated linearly to B; the single ensemble's chain copy is timed whole and split_rhat on the first `--host-walkers` walkers of
it, extrapolated linearly to all (its temporaries are several times the chain).  "selected GB/s" is the bytes of the selected
samples, counted once, over the call's time; get_rhat reads them twice.
usage: python tools/rhat_bench.py [--quick] [--out rhat_bench.json] [--seconds 1] [--host-members 128] [--host-walkers 4096]
       python tools/rhat_bench.py --prof --host-members 64 --host-walkers 256     (six calls of each: for rocprofv3 --kernel-trace --stats)"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from emcee_amd import EnsembleBatch, EnsembleSampler, moves, summary, targets  # noqa: E402


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


def row(shape, what, gb, cold, warm, calls, host_s=None, note=""):
    return dict(shape=shape, call=what, selected_GB=gb, first_s=cold, warm_s=warm, calls_timed=calls, selected_GBps=gb / warm,
                host_s=host_s, host_over_warm=None if host_s is None else host_s / warm, note=note)


def bench_batch(B, N, D, steps, seconds, host_members, rs):
    shape = "%d members of %d x %d, %d steps" % (B, N, D, steps)
    bt = EnsembleBatch(B, N, D, targets.IsoGaussian(), moves=moves.StretchMove(), seeds=list(range(B)))
    bt.run_mcmc(rs.randn(B, N, D), steps, skip_initial_state_check=True)
    gb = B * steps * N * D * 8 / 1e9
    k = min(B, host_members)
    t0 = time.perf_counter()
    parts = [summary.split_rhat(bt._read(0, lo, min(lo + 64, k), 0, 1, False).transpose(1, 0, 2, 3)) for lo in range(0, k, 64)]
    host = (time.perf_counter() - t0) * B / k
    rows = []
    cold, warm, n, r = timed(lambda: bt.get_rhat(), seconds)
    hw = np.concatenate([p.within for p in parts])
    note = "max rel diff of rhat against the host on %d members: %.2g" % (k, np.abs(r.rhat[:k] / np.concatenate([p.rhat for p in parts]) - 1).max())
    assert np.allclose(r.within[:k], hw, rtol=1e-9)
    rows.append(row(shape, 'get_rhat(chains="walkers")', gb, cold, warm, n, host, note))
    cold, warm, n, r = timed(lambda: bt.get_rhat(chains="members"), seconds)
    rows.append(row(shape, 'get_rhat(chains="members")', gb, cold, warm, n, None, "pooled rhat %s" % np.array2string(r.rhat, precision=4)))
    cold, warm, n, r = timed(lambda: bt.get_rhat(log_prob=True), seconds)
    rows.append(row(shape, "get_rhat(log_prob=True)", gb * (D + 1) / D, cold, warm, n))
    cold, warm, n, _ = timed(lambda: bt.get_summary(cov=False, quantiles=()), seconds)
    rows.append(row(shape, "get_summary(cov=False, quantiles=())", gb, cold, warm, n, None, "the chain twice, the log-probs once"))
    bt.close()
    return rows


def bench_single(N, D, steps, seconds, host_walkers, rs):
    shape = "%d x %d, %d steps" % (N, D, steps)
    s = EnsembleSampler(N, D, targets.IsoGaussian(), rng="philox")
    s.run_mcmc(rs.randn(N, D), steps, skip_initial_state_check=True)
    assert s.backend._dev is not None
    gb = steps * N * D * 8 / 1e9
    rows = []
    cold, warm, n, r = timed(lambda: s.get_rhat(), seconds)
    t0 = time.perf_counter()
    x = s.get_chain()
    t_copy = time.perf_counter() - t0
    k = min(N, host_walkers)
    t0 = time.perf_counter()
    summary.split_rhat(x[:, :k])
    t_host = (time.perf_counter() - t0) * N / k
    del x
    note = "host = chain copy %.2f s + split_rhat %.2f s (timed on %d walkers, extrapolated)" % (t_copy, t_host, k)
    rows.append(row(shape, "get_rhat()", gb, cold, warm, n, t_copy + t_host, note))
    cold, warm, n, _ = timed(lambda: s.get_rhat(log_prob=True), seconds)
    rows.append(row(shape, "get_rhat(log_prob=True)", gb * (D + 1) / D, cold, warm, n))
    cold, warm, n, _ = timed(lambda: s.get_summary(cov=False, quantiles=()), seconds)
    rows.append(row(shape, "get_summary(cov=False, quantiles=())", gb, cold, warm, n, None, "the chain twice, the log-probs once"))
    return rows, r


def main():
    arg = lambda flag, default, kind: kind(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default  # noqa: E731
    quick = "--quick" in sys.argv
    seconds, out_path = arg("--seconds", 1.0, float), arg("--out", "rhat_bench.json", str)
    rs = np.random.RandomState(1)
    if "--prof" in sys.argv:           # two calls of each per shape: for rocprofv3 --kernel-trace --stats
        seconds = 0.0
    rows = bench_batch(*((64, 32, 5, 500) if quick else (1024, 32, 5, 5000)), seconds, arg("--host-members", 128, int), rs)
    single, _ = bench_single(*((4096, 64, 40) if quick else (65536, 64, 200)), seconds, arg("--host-walkers", 4096, int), rs)
    rows += single
    for r in rows:
        print(json.dumps(r), flush=True)
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
    print("\n| shape | call | selected GB | first s | warm s (calls) | selected GB/s | host s | host / warm | note |")
    print("|---|---|---:|---:|---:|---:|---:|---:|---|")
    for r in rows:
        print("| %s | `%s` | %.2f | %.4f | %.4f (%d) | %.0f | %s | %s | %s |" % (
            r["shape"], r["call"], r["selected_GB"], r["first_s"], r["warm_s"], r["calls_timed"], r["selected_GBps"],
            "" if r["host_s"] is None else "%.1f" % r["host_s"], "" if r["host_s"] is None else "%.0fx" % r["host_over_warm"], r["note"]))


if __name__ == "__main__":
    main()
