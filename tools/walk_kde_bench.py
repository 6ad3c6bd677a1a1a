"""µs/step of WalkMove(s=8), WalkMove() and KDEMove() on the device (rng="philox", DenseGaussian target), alone and as a
50/50 mixture with StretchMove, at 4 096 x 16, 16 384 x 32 and 65 536 x 64, and of the host path (exact mode: host
get_proposal) at 1 024 x 16 for the ratio.  One JSON line per case; --md also prints a markdown table.

    python tools/walk_kde_bench.py [--shapes 4096x16,16384x32,65536x64] [--md]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import emcee_amd  # noqa: E402
from emcee_amd import moves, targets  # noqa: E402

MOVES = {"WalkMove(s=8)": lambda: moves.WalkMove(s=8), "WalkMove()": lambda: moves.WalkMove(), "KDEMove()": lambda: moves.KDEMove()}


def target(D):
    rs = np.random.RandomState(D)
    A = rs.randn(D, D) / np.sqrt(D)
    cov = A @ A.T + np.eye(D)
    mu = rs.randn(D)
    return mu, cov


def time_run(N, D, make, rng, nsteps, warmup):
    mu, cov = target(D)
    s = emcee_amd.EnsembleSampler(N, D, targets.DenseGaussian(mu, np.linalg.inv(cov)), moves=make(), rng=rng)
    s.random_state = np.random.RandomState(1).get_state()
    p0 = mu + np.random.RandomState(2).randn(N, D) @ np.linalg.cholesky(cov).T
    st = s.run_mcmc(p0, warmup, store=False, skip_initial_state_check=True)
    if s._ens is not None:
        s._ens.sync()
    t0 = time.perf_counter()
    st = s.run_mcmc(st, nsteps, store=False, skip_initial_state_check=True)
    if s._ens is not None:
        s._ens.sync()
    dt = time.perf_counter() - t0
    np.asarray(st.coords)
    return 1e6 * dt / nsteps


def steps_for(N, D, name):
    work = N * N * D if name == "KDEMove()" or name == "WalkMove()" else N * D * 8
    return int(max(3, min(50, 2e11 / max(work, 1))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x16,16384x32,65536x64")
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--host-shapes", default="1024x16")
    ap.add_argument("--moves", default=",".join(MOVES), help="comma-separated subset of " + ", ".join(MOVES))
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--alone", action="store_true", help="no 50/50 mixtures")
    ap.add_argument("--md", action="store_true")
    a = ap.parse_args()
    sel = {k: v for k, v in MOVES.items() if k in a.moves.split(",")}
    rows = []
    host = {}
    for hs in ([] if a.no_host else a.host_shapes.split(",")):
        hN, hD = (int(v) for v in hs.split("x"))
        for name, make in sel.items():
            us = time_run(hN, hD, make, "mt19937", a.host_steps, 1)
            host[(name, hN, hD)] = us
            rows.append(dict(move=name, mix="alone", N=hN, D=hD, path="host (mt19937)", us_per_step=round(us, 1)))
            print(json.dumps(rows[-1]), flush=True)
    for shape in a.shapes.split(","):
        N, D = (int(v) for v in shape.split("x"))
        for name, make in sel.items():
            for mix in ("alone",) if a.alone else ("alone", "50/50 stretch"):
                mk = make if mix == "alone" else (lambda make=make: [(make(), 0.5), (moves.StretchMove(), 0.5)])
                n = steps_for(N, D, name)
                us = time_run(N, D, mk, "philox", n, 2)
                r = dict(move=name, mix=mix, N=N, D=D, path="device (philox)", steps=n, us_per_step=round(us, 1))
                for (hname, hN, hD), hus in host.items():
                    if hname == name and mix == "alone" and (N, D) == (4096, 16):
                        r["host_%dx%d_over_this" % (hN, hD)] = round(hus / us, 1)
                rows.append(r)
                print(json.dumps(r), flush=True)
    if a.md:
        print("\n| move | mix | walkers x ndim | path | us/step |\n|---|---|---|---|---|")
        for r in rows:
            print("| %s | %s | %d x %d | %s | %.1f |" % (r["move"], r["mix"], r["N"], r["D"], r["path"], r["us_per_step"]))


if __name__ == "__main__":
    main()
