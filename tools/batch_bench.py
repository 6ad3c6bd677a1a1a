"""Throughput of EnsembleBatch (B independent small ensembles, one launch a chunk) in member-steps/s, beside one ensemble of the
same shape run alone and a Python loop of single samplers.  Two launch shapes: "auto" (tuning keys 0) and "single" (the
single-ensemble shape the B = 1 launch uses, forced for every B).
usage: python tools/batch_bench.py [--quick] [--out batch_bench.json]"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from emcee_amd import EnsembleBatch, EnsembleSampler, moves, targets  # noqa: E402

SHAPES = [
    ("32x5 iso stretch", 32, 5, "iso", lambda: moves.StretchMove()),
    ("32x5 dense stretch", 32, 5, "dense", lambda: moves.StretchMove()),
    ("100x10 diag DE+snooker", 100, 10, "diag", lambda: [moves.DEMove(), moves.DESnookerMove()]),
    ("256x32 rosenbrock stretch", 256, 32, "rosen", lambda: moves.StretchMove()),
]


def make_target(kind, D, rs):
    if kind == "iso":
        return targets.IsoGaussian()
    if kind == "rosen":
        return targets.Rosenbrock(20.0)
    if kind == "diag":
        return targets.DiagGaussian(np.zeros(D), 1.0 / (0.1 + rs.rand(D)))
    A = rs.randn(D, D)
    icov = np.linalg.inv(A @ A.T / D + 0.5 * np.eye(D))
    return targets.DenseGaussian(np.zeros(D), 0.5 * (icov + icov.T))


def p0_of(kind, shape, rs):
    return 1.0 + 0.1 * rs.randn(*shape) if kind == "rosen" else rs.randn(*shape)


def timed(run, steps):
    run(max(2, steps // 10))
    t0 = time.perf_counter()
    run(steps)
    return time.perf_counter() - t0


def adaptive(run, budget=0.25, most=4000):
    """steps so that the timed run takes about `budget` seconds; -> seconds per step"""
    probe = timed(run, 20) / 20
    steps = int(max(20, min(most, budget / max(probe, 1e-9))))
    return timed(run, steps) / steps


def bench_batch(B, N, D, kind, mf, tune, rs):
    tg = make_target(kind, D, rs)
    bt = EnsembleBatch(B, N, D, tg, moves=mf(), seeds=list(range(B)))
    for k, v in tune.items():
        bt.set_tuning(k, v)
    bt.run_mcmc(p0_of(kind, (B, N, D), rs), 1, store=False, skip_initial_state_check=True)
    sec = adaptive(lambda n: bt.run_mcmc(None, n, store=False))
    info = bt.launch_info()
    bt.close()
    return B / sec, info


def bench_single(N, D, kind, mf, rs):
    s = EnsembleSampler(N, D, make_target(kind, D, rs), moves=mf(), rng="philox")
    s.run_mcmc(p0_of(kind, (N, D), rs), 1, store=False, skip_initial_state_check=True)
    return 1.0 / adaptive(lambda n: s.run_mcmc(None, n, store=False))


def bench_loop(N, D, kind, mf, rs, count=16, steps=200):
    """a Python loop over `count` single samplers, each run_mcmc'd in turn (what a user without the batch writes)"""
    ss = [EnsembleSampler(N, D, make_target(kind, D, rs), moves=mf(), rng="philox") for _ in range(count)]
    for s in ss:
        s.run_mcmc(p0_of(kind, (N, D), rs), 1, store=False, skip_initial_state_check=True)
    t0 = time.perf_counter()
    for s in ss:
        s.run_mcmc(None, steps, store=False)
    return count * steps / (time.perf_counter() - t0)


def main():
    quick = "--quick" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "batch_bench.json"
    Bs = [1, 16, 256, 1024] if quick else [1, 16, 256, 1024, 4096]
    rows = []
    for name, N, D, kind, mf in SHAPES:
        rs = np.random.RandomState(1)
        single = bench_single(N, D, kind, mf, rs)
        loop = bench_loop(N, D, kind, mf, rs)
        _, info1 = bench_batch(1, N, D, kind, mf, {}, rs)
        forced = {"batch_threads": info1["threads"], "batch_plan_steps": info1["plan_steps"]}
        for B in Bs:
            auto, ia = bench_batch(B, N, D, kind, mf, {}, rs)
            lat, il = bench_batch(B, N, D, kind, mf, forced, rs)
            r = dict(shape=name, B=B, single_steps_per_s=single, loop_member_steps_per_s=loop,
                     auto_member_steps_per_s=auto, auto_shape=[ia["threads"], ia["plan_steps"]],
                     single_shape_member_steps_per_s=lat, single_shape=[il["threads"], il["plan_steps"]],
                     auto_vs_single=auto / single)
            print(json.dumps(r), flush=True)
            rows.append(r)
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
