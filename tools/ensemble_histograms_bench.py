"""EnsembleSampler.get_histograms (emx_chain_minmax + emx_histograms: the marginal histograms and the pair panels of a corner plot,
counted next to the chain) against the host path it replaces on the same sampler: get_chain(flat=True), then np.histogram per
column and np.histogram2d per pair.

Both are host clocks around calls that return with their results on the host.  The device call is timed once cold (scratch
allocated) and then at least 3 times and for at least `--seconds`: the median.  The host path is timed once (it takes seconds to
minutes); where it would take more than `--host-budget` seconds for the panels, `--host-pairs` of the panels are timed and the
rest is extrapolated in proportion -- the table says which.  Counts are compared (np.array_equal) on everything the host counted.
Chain passes are from the design: one for the min / max when the range comes from the data, one for the binning (the column tiles
partition the columns), none per pair -- the panels read one byte a value from the code plane.
usage: python tools/ensemble_histograms_bench.py [--quick] [--out ensemble_histograms_bench.json] [--seconds 1] [--only K]"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from emcee_amd import EnsembleSampler, targets  # noqa: E402

BINS = 64
# nwalkers, ndim, stored rows, pairs: None (marginals only), an int (that many chosen pairs) or "all"
CASES = [(65536, 64, 200, None), (65536, 64, 200, 8), (65536, 64, 200, "all"), (4096, 8, 500, "all")]
QUICK = [(8192, 64, 8, None), (8192, 64, 8, 8), (8192, 64, 8, "all"), (512, 8, 100, "all")]
_SAMPLERS = {}


def make_sampler(N, D, rows):
    if (N, D, rows) not in _SAMPLERS:
        _SAMPLERS.clear()                                   # one chain in HBM at a time
        rs = np.random.RandomState(1)
        A = rs.randn(D, D)
        icov = np.linalg.inv(A @ A.T / D + 0.5 * np.eye(D))
        s = EnsembleSampler(N, D, targets.DenseGaussian(0.1 * rs.randn(D), 0.5 * (icov + icov.T)), rng="philox")
        s.run_mcmc(rs.randn(N, D), rows, skip_initial_state_check=True)
        assert s.backend._dev is not None
        _SAMPLERS[(N, D, rows)] = s
    return _SAMPLERS[(N, D, rows)]


def choose_pairs(D, pairs):
    if pairs is None:
        return None
    if pairs == "all":
        return "all"
    rs = np.random.RandomState(2)
    out = set()
    while len(out) < pairs:
        i, j = rs.randint(0, D, 2)
        if i != j:
            out.add((int(min(i, j)), int(max(i, j))))
    return sorted(out)


def device_call(s, pairs):
    t0 = time.perf_counter()
    h = s.get_histograms(bins=BINS, pairs=pairs)
    return time.perf_counter() - t0, h


def host_call(s, h, budget, host_pairs):
    """-> (copy s, marginals s, panels s, panels timed, whether every count the host made equals the device's)"""
    t0 = time.perf_counter()
    x = s.get_chain(flat=True)
    t_copy = time.perf_counter() - t0
    t0 = time.perf_counter()
    cols = [np.ascontiguousarray(x[:, d]) for d in range(x.shape[1])]
    ok = True
    for d, col in enumerate(cols):
        c, e = np.histogram(col, bins=BINS)
        ok = ok and np.array_equal(c, h.counts[d]) and np.array_equal(e, h.edges[d])
    t_marg = time.perf_counter() - t0
    t_pairs, timed = 0.0, 0
    P = len(h.pairs)
    for p in range(P):
        if timed >= host_pairs and t_pairs / timed * P > budget:
            break
        i, j = h.pairs[p]
        t0 = time.perf_counter()
        c = np.histogram2d(cols[i], cols[j], bins=BINS)[0]
        t_pairs += time.perf_counter() - t0
        timed += 1
        ok = ok and np.array_equal(c, h.pair_counts[p])
    return t_copy, t_marg, t_pairs, timed, bool(ok)


def bench(N, D, rows, pairs, seconds, budget, host_pairs):
    s = make_sampler(N, D, rows)
    pr = choose_pairs(D, pairs)
    cold, h = device_call(s, pr)
    times, total = [], 0.0
    while total < seconds or len(times) < 3:
        t, h = device_call(s, pr)
        times.append(t)
        total += t
    warm = float(np.median(times))
    P = len(h.pairs)
    t_copy, t_marg, t_pairs, timed, ok = host_call(s, h, budget, host_pairs)
    host_panels = t_pairs * P / timed if timed else 0.0
    host = t_copy + t_marg + host_panels
    sel = rows * N * D * 8
    return dict(N=N, D=D, rows=rows, pairs=P, bins=BINS, pair_bins=min(BINS, 64), nsamples=h.nsamples, selection_GB=sel / 1e9,
                chain_passes=1 + 1,      # every call here has range=None: the min / max pass + the binning pass (1 with an explicit range)
                code_plane_GB=(rows * N * D / 1e9 if P else 0.0), code_bytes_read_GB=2 * P * rows * N / 1e9,
                device_first_s=cold, device_warm_s=warm, device_calls_timed=len(times), host_copy_s=t_copy, host_marginals_s=t_marg,
                host_panels_s=host_panels, host_panels_timed=timed, host_panels_extrapolated=bool(timed < P), host_s=host,
                host_over_device=host / warm, counts_equal=ok)


def main():
    arg = lambda flag, default, kind: kind(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default  # noqa: E731
    cases = QUICK if "--quick" in sys.argv else CASES
    only = arg("--only", -1, int)
    if only >= 0:
        cases = cases[only:only + 1]
    out_path = arg("--out", "ensemble_histograms_bench.json", str)
    rows = []
    for case in cases:
        r = bench(*case, arg("--seconds", 1.0, float), arg("--host-budget", 30.0, float), arg("--host-pairs", 8, int))
        print(json.dumps(r), flush=True)
        rows.append(r)
        with open(out_path, "w") as f:
            json.dump(rows, f, indent=1)
    print("\n| walkers x ndim x rows | pairs | selection GB | chain passes | host s = copy + marginals + panels (panels timed) | device 1st s | "
          "device warm s (calls) | host / device | counts equal |")
    print("|---|---:|---:|---:|---:|---:|---:|---:|---|")
    for r in rows:
        # an extrapolated host time is an estimate: its ratio is quoted to one digit
        ratio = ("~%dx" % float("%.1g" % r["host_over_device"]) if r["host_panels_extrapolated"] else "%.0fx" % r["host_over_device"])
        print("| %d x %d x %d | %d | %.3f | %d | %.2f = %.2f + %.2f + %.2f (%d of %d%s) | %.4f | %.5f (%d) | %s | %s |" % (
            r["N"], r["D"], r["rows"], r["pairs"], r["selection_GB"], r["chain_passes"], r["host_s"], r["host_copy_s"], r["host_marginals_s"],
            r["host_panels_s"], r["host_panels_timed"], r["pairs"], ", rest extrapolated" if r["host_panels_extrapolated"] else "",
            r["device_first_s"], r["device_warm_s"], r["device_calls_timed"], ratio, r["counts_equal"]))


if __name__ == "__main__":
    main()
