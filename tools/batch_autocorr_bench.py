"""EnsembleBatch.get_autocorr_time: the host path (one chain copy and one NumPy integrated_time per member) against
on_device=True (emx_autocorr_batch: one call for every member, only (B, ndim) numbers back).

The host path is timed on the first `--host-members` members and extrapolated linearly to B (it is a loop over members, each
the same work).  The device call is timed twice: the first call creates the hipFFT plans and grows the scratch, the second
reuses them (the median of three such calls).  Bytes per device call are computed from the shapes:
series x (7 L + 4 nt) x 8 with L = 2 next_pow_two(nt): the gather's write, the D2Z, power and Z2D passes' reads and writes
(2 L each: the half spectrum of L / 2 + 1 complex doubles is ~L doubles), the two-part mean's (two) and the gather's chain reads and the
accumulate's read (nt each); rocFFT's own intermediate passes are not counted.
usage: python tools/batch_autocorr_bench.py [--quick] [--out batch_autocorr_bench.json] [--host-members 8]
       python tools/batch_autocorr_bench.py --prof        (device calls only at B = 1 024 x 5 000 steps: for rocprofv3)"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from emcee_amd import EnsembleBatch, moves, targets  # noqa: E402
from emcee_amd.autocorr import next_pow_two  # noqa: E402

SHAPES = [
    ("32x5 iso stretch", 32, 5, "iso", lambda: moves.StretchMove()),
    ("100x10 diag DE+snooker", 100, 10, "diag", lambda: [(moves.DEMove(), 0.8), (moves.DESnookerMove(), 0.2)]),
]


def make_batch(B, N, D, kind, mf, steps, rs):
    tg = targets.IsoGaussian() if kind == "iso" else targets.DiagGaussian(np.zeros(D), 1.0 / (0.1 + rs.rand(D)))
    bt = EnsembleBatch(B, N, D, tg, moves=mf(), seeds=list(range(B)))
    bt.run_mcmc(rs.randn(B, N, D), steps, skip_initial_state_check=True)
    return bt


def device_call(bt):
    t0 = time.perf_counter()
    tau = bt.get_autocorr_time(quiet=True, on_device=True)       # returns after the device results are on the host
    return time.perf_counter() - t0, tau


def bench(B, N, D, kind, mf, steps, host_members, rs):
    bt = make_batch(B, N, D, kind, mf, steps, rs)
    cold, tau = device_call(bt)
    warm = float(np.median([device_call(bt)[0] for _ in range(3)]))
    k = min(B, host_members)
    t0 = time.perf_counter()
    host = np.stack([bt[b].get_autocorr_time(quiet=True) for b in range(k)])
    t_host_k = time.perf_counter() - t0
    bt.close()
    host_all = t_host_k * B / k
    nt = steps
    L = 2 * next_pow_two(nt)
    series = B * N * D
    gbytes = series * (7 * L + 4 * nt) * 8 / 1e9
    return dict(B=B, N=N, D=D, steps=steps, host_members_timed=k, host_s_timed=t_host_k, host_s_extrapolated=host_all,
                device_first_s=cold, device_warm_s=warm, speedup_warm=host_all / warm, speedup_first=host_all / cold,
                bytes_per_call_GB=gbytes, GBps_warm=gbytes / warm,
                max_rel_diff_vs_host=float(np.nanmax(np.abs(tau[:k] - host) / np.abs(host))))


def main():
    if "--prof" in sys.argv:           # what rocprofv3 --kernel-trace --stats traces: two device calls per shape
        for name, N, D, kind, mf in SHAPES:
            bt = make_batch(1024, N, D, kind, mf, 5000, np.random.RandomState(1))
            for _ in range(2):
                print(name, "%.4f s" % device_call(bt)[0], flush=True)
            bt.close()
        return
    quick = "--quick" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "batch_autocorr_bench.json"
    host_members = int(sys.argv[sys.argv.index("--host-members") + 1]) if "--host-members" in sys.argv else 8
    Bs, steps_list = ([16, 64], [200]) if quick else ([16, 256, 1024], [1000, 5000])
    rows = []
    for name, N, D, kind, mf in SHAPES:
        for steps in steps_list:
            for B in Bs:
                r = dict(shape=name, **bench(B, N, D, kind, mf, steps, host_members, np.random.RandomState(1)))
                print(json.dumps(r), flush=True)
                rows.append(r)
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
    print("\n| shape | B | steps | host s (timed members) | host s for B (extrapolated) | device 1st call s | device warm s | "
          "host / warm | GB per call | GB/s warm |")
    print("|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|")
    for r in rows:
        print("| %s | %d | %d | %.3f (%d) | %.2f | %.4f | %.4f | %.0fx | %.1f | %.0f |" % (
            r["shape"], r["B"], r["steps"], r["host_s_timed"], r["host_members_timed"], r["host_s_extrapolated"], r["device_first_s"],
            r["device_warm_s"], r["speedup_warm"], r["bytes_per_call_GB"], r["GBps_warm"]))


if __name__ == "__main__":
    main()
