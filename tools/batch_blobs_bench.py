"""What blobs cost an EnsembleBatch, and what they save (profiles/batch_blobs.md).  One model -- a per-member diagonal Gaussian with
K = 4 blobs {lp, x0 + x1, x0 * x1, member} -- compiled with targets.compile_fused once with blobs and once without, stored runs.

  (a) member-steps/s of the blob run of THIS tree against the same functor without blobs in the PARENT tree (`--parent PATH`: a
      built checkout of the parent commit), with the stored-bytes ratio (ndim + 1 + K) / (ndim + 1) beside it;
  (b) the functor without blobs in this tree against the parent's (the unchanged instantiation);
  (c) get_blobs() and get_blob_summary() against what a batch without blobs offers: get_chain() and the NumPy expression on the host.

Every figure of (a) / (b) comes from a child process of its own (`--child`), and the three legs ALTERNATE for `--rounds` rounds in
one call, so that drift of a shared machine lands on all of them; a leg's spread is the range of its rounds' medians.  A child
times emx_batch_run alone (state, initial evaluation and the chain's allocation are outside the window; the window ends with a
stream synchronise), `--repeats` times on fresh handles, after one warm-up run of the same length.
usage: python tools/batch_blobs_bench.py --parent PATH [--rounds R] [--repeats K] [--quick]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 4
SHAPES = [("1024 x (32 x 5)", 1024, 32, 5, 1500), ("256 x (64 x 32)", 256, 64, 32, 500)]      # name, B, N, D, stored steps a run
SOURCE = r"""
__device__ inline double diag(const double* x, int ndim, int member, const void* user) {
    const double* mu = (const double*)user + (long long)member * 2 * ndim;
    const double* ivar = mu + ndim;
    double acc = 0.0;
    for (int d = 0; d < ndim; ++d) {
        const double r = x[d] - mu[d];
        acc = acc + ivar[d] * r * r;
    }
    return -0.5 * acc;
}
struct Plain {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const { return diag(x, ndim, member, user); }
};
struct WithBlobs {
    __device__ double operator()(const double* x, int ndim, int member, const void* user, double* blobs) const {
        const double lp = diag(x, ndim, member, user);
        blobs[0] = lp;
        blobs[1] = x[0] + x[1];
        blobs[2] = x[0] * x[1];
        blobs[3] = (double)member;
        return lp;
    }
};
"""


def child(tree, leg, shape, repeats):
    """one leg of one shape in the package of `tree` -> a JSON line {rates: member-steps/s of every repeat}"""
    sys.path.insert(0, tree)
    import torch
    from emcee_amd import EnsembleBatch
    from emcee_amd.targets import compile_fused
    name, B, N, D, nsteps = next(s for s in SHAPES if s[0] == shape)
    rs = np.random.RandomState(1)
    user = torch.as_tensor(np.concatenate([0.1 * rs.randn(B, 1, D), 1.0 / (0.2 + rs.rand(B, 1, D))], axis=1), device="cuda").contiguous()
    p0 = rs.randn(B, N, D)
    lib = compile_fused(SOURCE, "WithBlobs", D, nblobs=K) if leg == "blobs" else compile_fused(SOURCE, "Plain", D)
    rates = []
    for rep in range(repeats + 1):                    # the first run warms up (code objects, allocator)
        bt = EnsembleBatch(B, N, D, lib.target(user=user), seeds=list(range(B)))
        clib, h = bt._lib(), bt._handle()
        bt._ck(clib.emx_batch_set_state(h, p0, None))
        bt._ck(clib.emx_batch_eval_state_log_prob(h))
        bt._ck(clib.emx_batch_chain_config(h, nsteps))
        bits = np.zeros(B, dtype=np.uint32)
        bt._ck(clib.emx_batch_status(h, bits))        # synchronises the stream
        t0 = time.perf_counter()
        bt._ck(clib.emx_batch_run(h, nsteps, 1, 1))
        bt._ck(clib.emx_batch_status(h, bits))
        dt = time.perf_counter() - t0
        assert not bits.any()
        if rep:
            rates.append(B * nsteps / dt)
        bt.close()
    print(json.dumps(dict(leg=leg, shape=shape, tree=os.path.basename(os.path.abspath(tree)), rates=rates)), flush=True)


def readers(shape, repeats):
    """(c): one stored blob run, then get_blobs / get_blob_summary against get_chain + NumPy on the host, seconds (median of repeats)"""
    sys.path.insert(0, HERE)
    import torch
    from emcee_amd import EnsembleBatch
    from emcee_amd.targets import compile_fused
    name, B, N, D, nsteps = next(s for s in SHAPES if s[0] == shape)
    rs = np.random.RandomState(1)
    user = torch.as_tensor(np.concatenate([0.1 * rs.randn(B, 1, D), 1.0 / (0.2 + rs.rand(B, 1, D))], axis=1), device="cuda").contiguous()
    bt = EnsembleBatch(B, N, D, compile_fused(SOURCE, "WithBlobs", D, nblobs=K).target(user=user), seeds=list(range(B)))
    bt.run_mcmc(rs.randn(B, N, D), nsteps)

    def med(f):
        ts = []
        for _ in range(repeats + 1):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts[1:]))

    def host_blobs():
        x = bt.get_chain()
        lp = bt.get_log_prob()
        return np.stack([lp, x[..., 0] + x[..., 1], x[..., 0] * x[..., 1], np.broadcast_to(np.arange(B, dtype=float)[:, None, None], lp.shape)], -1)

    def host_summary():
        b = host_blobs().reshape(B, -1, K)
        return b.mean(axis=1), np.stack([np.cov(b[m].T) for m in range(B)]), np.quantile(b, (0.16, 0.5, 0.84), axis=1)
    r = dict(shape=shape, chain_GB=B * nsteps * N * (D + 1) * 8 / 1e9, blobs_GB=B * nsteps * N * K * 8 / 1e9,
             get_blobs_s=med(bt.get_blobs), host_blobs_s=med(host_blobs), get_blob_summary_s=med(bt.get_blob_summary),
             host_summary_s=med(host_summary))
    assert np.array_equal(bt.get_blobs(), host_blobs())
    print(json.dumps(r), flush=True)
    bt.close()


def main():
    a = sys.argv[1:]
    opt = lambda k, d: a[a.index(k) + 1] if k in a else d  # noqa: E731
    repeats = int(opt("--repeats", 5))
    if "--child" in a:
        return child(opt("--tree", HERE), opt("--leg", "plain"), opt("--shape", SHAPES[0][0]), repeats)
    if "--readers" in a:
        return readers(opt("--shape", SHAPES[0][0]), repeats)
    parent, rounds = opt("--parent", None), int(opt("--rounds", 3))
    legs = [("this blobs", HERE, "blobs"), ("this plain", HERE, "plain")] + ([("parent plain", parent, "plain")] if parent else [])
    me = os.path.abspath(__file__)
    for name, B, N, D, nsteps in SHAPES[:1] if "--quick" in a else SHAPES:
        meds = {label: [] for label, _, _ in legs}
        for _ in range(rounds):                       # alternate the legs: drift lands on all of them
            for label, tree, leg in legs:
                out = subprocess.run([sys.executable, me, "--child", "--tree", tree, "--leg", leg, "--shape", name, "--repeats", str(repeats)],
                                     capture_output=True, text=True, timeout=900)
                if out.returncode != 0:
                    raise RuntimeError("%s failed:\n%s" % (label, out.stderr[-3000:]))
                r = json.loads(out.stdout.strip().splitlines()[-1])
                meds[label].append(float(np.median(r["rates"])))
                print(json.dumps(dict(shape=name, leg=label, median=meds[label][-1], low=min(r["rates"]), high=max(r["rates"]))), flush=True)
        row = {label: (float(np.median(v)), min(v), max(v)) for label, v in meds.items()}
        print("\n%s, stored runs of %d steps, K = %d: stored-bytes ratio (ndim + 1 + K) / (ndim + 1) = %.3f" % (name, nsteps, K, (D + 1 + K) / (D + 1.0)))
        for label, (m, lo, hi) in row.items():
            print("  %-13s %.4g member-steps/s (rounds' medians %.4g - %.4g, spread %.1f %%)" % (label, m, lo, hi, 100 * (hi - lo) / m))
        base = row.get("parent plain", row["this plain"])[0]
        print("  (a) plain(parent) / blobs = %.3f    (b) this plain / parent plain = %.3f" % (base / row["this blobs"][0], row["this plain"][0] / base))
        out = subprocess.run([sys.executable, me, "--readers", "--shape", name, "--repeats", "3"], capture_output=True, text=True, timeout=900)
        print("  (c) " + (out.stdout.strip().splitlines()[-1] if out.returncode == 0 else "failed: " + out.stderr[-2000:]), flush=True)


if __name__ == "__main__":
    main()
