"""EnsembleBatch.get_summary (emx_summary_batch: mean, covariance, quantiles and MAP of every member next to the chain) against
the host path it replaces: get_chain(flat=True) / get_log_prob(flat=True) and np.mean / np.cov / np.quantile / argmax.

The host path is timed on the first `--host-members` members in blocks of 64 (a block's chain copy is what fits a host
comfortably: at 1 024 members of 32 x 5 x 5 000 the whole copy is 6.5 GB) and extrapolated linearly to B: it is the same work for
every member.  The device call is timed once cold (scratch allocated) and then repeatedly for at least `--seconds` (default 1 s)
and at least 5 calls: the median.  Bytes per call are computed from the shapes: the chain once for the mean, once for the
residual sums (the mean kernels again, on x - mean), once for the Gram matrix and once per selection pass (8), the log-probs once for the MAP.
usage: python tools/batch_summary_bench.py [--quick] [--out batch_summary_bench.json] [--host-members 128] [--seconds 1]
       python tools/batch_summary_bench.py --prof        (two device calls per shape: for rocprofv3 --kernel-trace --stats)"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from emcee_amd import EnsembleBatch, moves, targets  # noqa: E402

QUANTILES = (0.16, 0.5, 0.84)
# name, B, nwalkers, ndim, target kind, stored steps
SHAPES = [("32x5 iso stretch", 1024, 32, 5, "iso", 5000), ("64x32 dense stretch", 256, 64, 32, "dense", 2000)]
QUICK = [("32x5 iso stretch", 64, 32, 5, "iso", 500), ("64x32 dense stretch", 16, 64, 32, "dense", 200)]


def make_batch(B, N, D, kind, steps, rs):
    if kind == "iso":
        tg = targets.IsoGaussian()
    else:
        A = rs.randn(D, D)
        icov = np.linalg.inv(A @ A.T / D + 0.5 * np.eye(D))
        tg = targets.DenseGaussian(0.1 * rs.randn(D), 0.5 * (icov + icov.T))
    bt = EnsembleBatch(B, N, D, tg, moves=moves.StretchMove(), seeds=list(range(B)))
    bt.run_mcmc(rs.randn(B, N, D), steps, skip_initial_state_check=True)
    return bt


def device_call(bt):
    t0 = time.perf_counter()
    s = bt.get_summary(quantiles=QUANTILES)          # returns after the results are on the host
    return time.perf_counter() - t0, s


def host_block(bt, lo, hi):
    """what the caller does without get_summary, for members [lo, hi)"""
    x = bt._read(0, lo, hi, 0, 1, True)
    lp = bt._read(1, lo, hi, 0, 1, True)
    mean = x.mean(axis=1)
    cov = np.stack([np.atleast_2d(np.cov(x[b].T)) for b in range(hi - lo)])
    q = np.quantile(x, QUANTILES, axis=1).transpose(1, 0, 2)
    at = lp.argmax(axis=1)
    return mean, cov, q, x[np.arange(hi - lo), at], lp[np.arange(hi - lo), at]


def bench(name, B, N, D, kind, steps, host_members, seconds, rs):
    bt = make_batch(B, N, D, kind, steps, rs)
    cold, s = device_call(bt)
    times, total = [], 0.0
    while total < seconds or len(times) < 5:
        t, s = device_call(bt)
        times.append(t)
        total += t
    warm = float(np.median(times))
    k = min(B, host_members)
    t0 = time.perf_counter()
    parts = [host_block(bt, lo, min(lo + 64, k)) for lo in range(0, k, 64)]
    t_host_k = time.perf_counter() - t0
    h_mean, h_cov, h_q, h_x, h_lp = [np.concatenate([p[i] for p in parts]) for i in range(5)]
    bt.close()
    chain_gb = B * steps * N * D * 8 / 1e9
    gbytes = chain_gb * (3 + 8) + B * steps * N * 8 / 1e9
    host_all = t_host_k * B / k
    return dict(shape=name, B=B, N=N, D=D, steps=steps, nsamples=s.nsamples, host_members_timed=k, host_s_timed=t_host_k,
                host_s_extrapolated=host_all, device_first_s=cold, device_warm_s=warm, device_calls_timed=len(times),
                speedup_warm=host_all / warm, chain_GB=chain_gb, bytes_per_call_GB=gbytes, GBps_warm=gbytes / warm,
                max_abs_mean_diff=float(np.abs(s.mean[:k] - h_mean).max()),
                max_rel_cov_diff=float((np.abs(s.cov[:k] - h_cov) / np.abs(h_cov).max()).max()),
                max_abs_quantile_diff=float(np.abs(s.quantiles[:k] - h_q).max()),
                map_equal=bool(np.array_equal(s.map_coords[:k], h_x) and np.array_equal(s.map_log_prob[:k], h_lp)))


def main():
    quick = "--quick" in sys.argv
    shapes = QUICK if quick else SHAPES
    if "--prof" in sys.argv:
        for name, B, N, D, kind, steps in shapes:
            bt = make_batch(B, N, D, kind, steps, np.random.RandomState(1))
            for _ in range(2):
                print(name, "%.4f s" % device_call(bt)[0], flush=True)
            if D < 16:                 # k_bacf_mean on the same chain: the yardstick for a pass over it
                bt.get_autocorr_time(quiet=True, on_device=True)
            bt.close()
        return
    arg = lambda flag, default, kind: kind(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default  # noqa: E731
    out_path = arg("--out", "batch_summary_bench.json", str)
    host_members, seconds = arg("--host-members", 128, int), arg("--seconds", 1.0, float)
    rows = []
    for shape in shapes:
        r = bench(*shape, host_members, seconds, np.random.RandomState(1))
        print(json.dumps(r), flush=True)
        rows.append(r)
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
    print("\n| shape | B | steps | chain GB | host s (timed members) | host s for B (extrapolated) | device 1st s | device warm s (calls) | "
          "host / warm | GB read per call | GB/s warm |")
    print("|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|")
    for r in rows:
        print("| %s | %d | %d | %.2f | %.2f (%d) | %.1f | %.4f | %.4f (%d) | %.0fx | %.1f | %.0f |" % (
            r["shape"], r["B"], r["steps"], r["chain_GB"], r["host_s_timed"], r["host_members_timed"], r["host_s_extrapolated"],
            r["device_first_s"], r["device_warm_s"], r["device_calls_timed"], r["speedup_warm"], r["bytes_per_call_GB"], r["GBps_warm"]))


if __name__ == "__main__":
    main()
