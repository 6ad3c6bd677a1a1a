"""SHA-256 of everything short runs of the three one-workgroup kernels (k_small_run, k_pt_run, k_batch_cb) leave behind, case by
case, through the public Python API only -- so that the same file runs on any commit of this project and its output can be held
against another commit's (tests/golden/one_workgroup_bits.json, tests/test_gpu_one_workgroup_bits.py).

usage: python tools/one_workgroup_bits.py [--out FILE] [--compile-only] [--cache DIR]

Per case: the final coordinates and log-probs, the stored chain and its log-probs, the acceptance fractions (accept counts over the
stored steps), blobs where the target has them, and for PTSampler the log-likelihood chain, the stored betas, the final ladder and
the swap acceptance fractions.  --compile-only builds the user libraries (no GPU needed) and stops.

The digests come from the public API alone.  The optional path report of run_all does not: for EnsembleSampler it reads the device
handle's small_info() through the private attribute _ens (the sampler exposes no launch report of its own), and is empty where
that attribute is missing."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NBLOBS = 2
MAXDATA = 200

SOURCE = r"""
// user: per member 2 ndim doubles (mean, inverse variance), then 3 * 200 doubles of data (t, y, weight)
#define OWB_MAXDATA 200
__device__ inline const double* owb_rec(const void* user, int ndim, int member) {
    return (const double*)user + (size_t)member * (2 * ndim + 3 * OWB_MAXDATA);
}
struct OwbQuad {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const {
        const double* r = owb_rec(user, ndim, member);
        double acc = 0.0;
        for (int d = 0; d < ndim; ++d) {
            const double e = x[d] - r[d];
            acc = acc + r[ndim + d] * e * e;
        }
        return -0.5 * acc;
    }
    __device__ double operator()(const double* x, int ndim, int member, const void* user, double* blobs) const {
        const double lp = (*this)(x, ndim, member, user);
        blobs[0] = lp;
        blobs[1] = x[0] + x[ndim - 1];
        return lp;
    }
};
struct OwbLine {
    __device__ double base(const double* x, int ndim, int member, const void* user) const {
        double acc = 0.0;
        for (int d = 0; d < ndim; ++d) acc = acc + x[d] * x[d];
        return -0.05 * acc;
    }
    __device__ double term(const double* x, int ndim, int member, long long k, const void* user) const {
        const double* r = owb_rec(user, ndim, member) + 2 * ndim;
        const double e = r[OWB_MAXDATA + k] - (x[0] + x[ndim - 1] * r[k]);
        return -0.5 * (r[2 * OWB_MAXDATA + k] * e * e);
    }
};
struct OwbPrior {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const {
        double acc = 0.0;
        for (int d = 0; d < ndim; ++d) {
            if (x[d] > 4.0 || x[d] < -4.0) return -__builtin_inf();
            acc = acc + x[d] * x[d];
        }
        return -0.02 * acc;
    }
};
"""

# (walkers, ndim): odd ndim; uneven thirds and partly dead wave groups under nsplits = 3; two doubles a lane and two chunks a row
SHAPES = {"32x5": (32, 5), "14x3": (14, 3), "40x18": (40, 18)}
# name -> (shape, move, proposal steps, thin_by); 72 steps are more than any path's plan batch holds
RUNS = [("stretch", "32x5", "stretch", 10, 1), ("de", "32x5", "de", 10, 1), ("snooker", "32x5", "snooker", 10, 1),
        ("gauss", "32x5", "gauss", 10, 1), ("mix_long_thin3", "32x5", "mix", 72, 3), ("thirds", "14x3", "stretch3", 12, 1),
        ("wide_mix", "40x18", "mix", 8, 1)]
MT_RUNS = [("stretch", "32x5", "stretch", 10, 1), ("stretch_long_thin3", "32x5", "stretch", 72, 3), ("thirds", "14x3", "stretch3", 12, 1),
           ("wide", "40x18", "stretch", 8, 1)]
NBATCH = 4
NDATA = [0, 1, 65, 200]              # ragged, around the 64 lanes of the data sum
NTEMPS = 3
PT_OBJECTS = 2
PT_NDATA = [1, 130]
PT_CHUNKED = (200, 17)               # 3 rungs of 200 x 17 do not fit with the 100 rows of a split staged: a half-step runs in chunks


def make_moves(name):
    from emcee_amd import moves
    live = dict(live_dangerously=True)
    if name == "stretch":
        return moves.StretchMove(**live)
    if name == "stretch3":
        return moves.StretchMove(nsplits=3, **live)
    if name == "de":
        return moves.DEMove(**live)
    if name == "snooker":
        return moves.DESnookerMove(**live)
    if name == "gauss":
        return moves.GaussianMove(0.3)
    mix = [(moves.StretchMove(**live), 0.4), (moves.DEMove(**live), 0.25), (moves.DESnookerMove(**live), 0.2)]
    return mix if name == "mix3" else mix + [(moves.GaussianMove(0.3), 0.15)]


def digest(a):
    a = np.ascontiguousarray(a)
    h = hashlib.sha256(("%s %s " % (a.dtype.str, a.shape)).encode())
    h.update(a.tobytes())
    return h.hexdigest()


def records(rs, members, D):
    """the user block of `members` members: mean, inverse variance, then the straight-line data"""
    rec = np.zeros((members, 2 * D + 3 * MAXDATA))
    rec[:, :D] = 0.1 * rs.randn(members, D)
    rec[:, D:2 * D] = 1.0 / (0.2 + rs.rand(members, D))
    t = np.linspace(-1.0, 1.0, MAXDATA)
    sigma = 2.0 * (1.0 + 0.5 * rs.rand(members, MAXDATA))
    rec[:, 2 * D:2 * D + MAXDATA] = t
    rec[:, 2 * D + MAXDATA:2 * D + 2 * MAXDATA] = 0.2 + 0.5 * t + sigma * rs.randn(members, MAXDATA)
    rec[:, 2 * D + 2 * MAXDATA:] = 1.0 / (sigma * sigma)
    return rec


def compile_all(cache):
    """every user library of the cases: {(kind, ndim): library}"""
    from concurrent.futures import ThreadPoolExecutor
    from emcee_amd.targets import compile_fused, compile_fused_pt

    def one(job):
        kind, D = job
        if kind == "fused":
            return compile_fused(SOURCE, "OwbQuad", D, name="owb_fused_%d" % D, cache_dir=cache)
        if kind == "blobs":
            return compile_fused(SOURCE, "OwbQuad", D, nblobs=NBLOBS, name="owb_blobs_%d" % D, cache_dir=cache)
        if kind == "data":
            return compile_fused(SOURCE, "OwbLine", D, name="owb_data_%d" % D, cache_dir=cache, data=True)
        if kind == "pt":
            return compile_fused_pt(SOURCE, "OwbQuad", D, name="owb_pt_%d" % D, cache_dir=cache)
        return compile_fused_pt(SOURCE, "OwbLine", D, prior="OwbPrior", name="owb_pt_data_%d" % D, cache_dir=cache, data=True)
    dims = sorted({D for _, D in SHAPES.values()})
    jobs = [(k, D) for D in dims for k in ("fused", "blobs", "data", "pt", "pt_data")] + [("pt", PT_CHUNKED[1])]
    with ThreadPoolExecutor(min(16, len(jobs))) as ex:
        return dict(zip(jobs, ex.map(one, jobs)))


def of_sampler(s):
    last = s.get_last_sample()
    return dict(coords=digest(last.coords), last_log_prob=digest(last.log_prob), chain=digest(s.get_chain()),
                log_prob=digest(s.get_log_prob()), acceptance=digest(s.acceptance_fraction))


def of_pt(pt):
    out = of_sampler(pt)
    out.update(log_like=digest(pt.get_log_likelihood()), betas=digest(pt.get_betas()), ladder=digest(pt.ladder),
               swaps=digest(pt.tswap_acceptance_fraction))
    return out


def run_all(libs, paths=None):
    """-> {case: {array: digest}}.  paths (a dict, optional) receives per case what the sampler reports of the path its run took --
    launches, plan steps, threads, the small kernel's steps -- for a caller that wants to check it; it is not part of the digests."""
    import torch
    from emcee_amd import EnsembleBatch, EnsembleSampler, PTSampler, targets
    from emcee_amd.targets import BatchCallable
    out = {}
    paths = {} if paths is None else paths

    def builtin(rs, D, dense):
        if dense:
            A = rs.randn(D, D)
            icov = np.linalg.inv(A @ A.T / D + 0.5 * np.eye(D))
            return targets.DenseGaussian(0.1 * rs.randn(D), 0.5 * (icov + icov.T))
        return targets.DiagGaussian(0.1 * rs.randn(D), 1.0 / (0.2 + rs.rand(D)))

    for path, runs in (("ensemble_diag", RUNS), ("ensemble_dense", RUNS), ("ensemble_mt19937", MT_RUNS)):
        for k, (name, shape, mv, nsteps, thin) in enumerate(runs):
            N, D = SHAPES[shape]
            rs = np.random.RandomState(100 + k)
            s = EnsembleSampler(N, D, builtin(rs, D, path == "ensemble_dense"), moves=make_moves(mv),
                                rng="mt19937" if path == "ensemble_mt19937" else "philox")
            s.random_state = np.random.RandomState(7 + k).get_state()
            s.run_mcmc(rs.randn(N, D), nsteps // thin, thin_by=thin, skip_initial_state_check=True)
            out["%s/%s" % (path, name)] = of_sampler(s)
            paths["%s/%s" % (path, name)] = dict(s._ens.small_info(), nsteps=nsteps) if hasattr(getattr(s, "_ens", None), "small_info") else {}

    for path in ("batch_diag", "batch_dense", "batch_fused", "batch_blobs", "batch_data", "batch_callback"):
        for k, (name, shape, mv, nsteps, thin) in enumerate(RUNS):
            N, D = SHAPES[shape]
            rs = np.random.RandomState(200 + k)
            rec = torch.from_numpy(records(rs, NBATCH, D)).cuda()
            if path in ("batch_diag", "batch_dense"):
                tg = [builtin(rs, D, path == "batch_dense") for _ in range(NBATCH)]
            elif path == "batch_callback":
                mu, iv = rec[:, None, :D], rec[:, None, D:2 * D]
                tg = BatchCallable(lambda q, mu=mu, iv=iv: -0.5 * (iv * (q - mu) * (q - mu)).sum(-1))
            else:
                kind = path.split("_")[1]
                tg = libs[(kind, D)].target(user=rec, ndata=NDATA) if kind == "data" else libs[(kind, D)].target(user=rec)
            if path == "batch_callback" and mv == "mix":
                mv = "mix3"              # (a batched callback target, and PTSampler, take a GaussianMove only as the one move of the schedule)
            bt = EnsembleBatch(NBATCH, N, D, tg, moves=make_moves(mv), seeds=[11 + 5 * b + k for b in range(NBATCH)])
            bt.run_mcmc(rs.randn(NBATCH, N, D), nsteps // thin, thin_by=thin, skip_initial_state_check=True)
            res = of_sampler(bt)
            if path == "batch_blobs":
                res["blobs"] = digest(bt.get_blobs())
            out["%s/%s" % (path, name)] = res
            paths["%s/%s" % (path, name)] = dict(bt.launch_info(), nsteps=nsteps)
            bt.close()

    G, T = PT_OBJECTS, NTEMPS
    pt_runs = [(name, SHAPES[shape], mv, nsteps, thin) for name, shape, mv, nsteps, thin in RUNS] + [("chunked", PT_CHUNKED, "stretch", 4, 1)]
    for path in ("pt_fused", "pt_fused_data"):
        for k, (name, (N, D), mv, nsteps, thin) in enumerate(pt_runs):
            if path == "pt_fused_data" and name == "chunked":
                continue
            rs = np.random.RandomState(300 + k)
            rec = torch.from_numpy(records(rs, G * T, D)).cuda()
            if path == "pt_fused":
                like, prior = libs[("pt", D)].target(user=rec), (-4.0 * np.ones(D), 4.0 * np.ones(D))
            else:
                like, prior = libs[("pt_data", D)].target(user=rec, ndata=PT_NDATA), None
            pt = PTSampler(T, N, D, like, log_prior=prior, nbatch=G, moves=make_moves("mix3" if mv == "mix" else mv), seeds=[21 + 3 * g + k for g in range(G)],
                           swap_every=2, adaptive=True, adaptation_lag=20, adaptation_time=2)
            pt.run_mcmc(0.5 * rs.randn(G, T, N, D), nsteps // thin, thin_by=thin, skip_initial_state_check=True)
            out["%s/%s" % (path, name)] = of_pt(pt)
            paths["%s/%s" % (path, name)] = dict(pt.launch_info(), nsteps=nsteps)
            pt.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compile-only", action="store_true")
    ap.add_argument("--cache", default=os.path.join(ROOT, "build", "one_workgroup_bits"))
    a = ap.parse_args()
    libs = compile_all(a.cache)
    if a.compile_only:
        print("%d user libraries under %s" % (len(libs), a.cache))
        return
    text = json.dumps(run_all(libs), indent=1, sort_keys=True) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
