"""WalkMove and KDEMove on the device (csrc/emx_walkkde.hip) against the double-double reference of tests/hiprec.py.

The reference sees only the device's plan (plan_get) and the host twin of its draws (emx_host_walk_kde_draws).  Every check is a
forward-error bound that scales with what the arithmetic really loses (the spread of the helpers, |L||z|, the whitened radius),
not with the magnitude of the coordinates.  Besides the shape sweep: conditioning edges, the updates one split hands the next,
exact power-of-two scale covariance of the affine-invariant moves on every kernel path, and a 20-step replay."""
import ctypes as C

import numpy as np
import pytest

import emcee_amd
from emcee_amd import _lib, moves, targets
from emcee_amd.device import DeviceEnsemble

import hiprec as hp

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SEED = 0x5EED2

# Bounds (u = EPS / 2 is the unit roundoff):
# walk s >= 2: |q - q_ref| <= C_WALK_S eps (|x| + s W max|c - x|), W = max|w| + max|z| / sqrt(s - 1).  The last rounding costs
#   u |q| <= u (|x| + s max|w| max|c - x|); each computed w_k is off by (log2(64) + s/64 + 3) u max|z| / sqrt(s - 1) (mean z, then
#   1/sqrt(s - 1)), c - x by one u, and the fma chain's s roundings are of partial sums of random sign (sqrt(s) growth) below
#   s max|w| max|c - x|: C_WALK_S = 2.
C_WALK_S = 2.0
# q = base + L z (whole-complement walk, KDE): |q - q_ref| <= eps |q_ref| + C_LIN eps (D + 8) kappa (|L||z|).  The centred sums give
#   the covariance to a few u per entry in units of sqrt(S_ii S_jj); Cholesky's backward error is gamma_(D+1) |L||L^T|, which moves
#   L by (D + 1) u kappa in units of |L| (kappa = sqrt(cond) of the correlation matrix); L z adds gamma_D |L||z|: C_LIN = 2.
C_LIN = 2.0
# KDE factor: |f - f_ref| <= C_KDE eps (D + 8) kappa (1 + R^2).  The GEMM expansion y.Y - |Y|^2/2 - |y|^2/2 loses gamma_D R^2 per
#   score (it is not a difference of nearby points); the whitening moves y by (D + 1) u kappa |y|, so |y - Y|^2 by 2 (D + 1) u
#   kappa R^2; the LSE's exp / log add a few u: C_KDE = 2.
C_KDE = 2.0


def walk(s, nsplits=2, rnd=1):
    return _lib.MoveDesc(_lib.MOVE_WALK, nsplits, rnd, 0 if s is None else s, 0.0, 0.0, 0.0, 0.0)


def kde(bw=None, nsplits=2, rnd=1):
    rule, a = {None: (0, 0.0), "silverman": (1, 0.0)}.get(bw, (2, bw))
    return _lib.MoveDesc(_lib.MOVE_KDE, nsplits, rnd, rule, float(a), 0.0, 0.0, 0.0)


def host_draws(md, N, D, split, step, seed=SEED):
    S = md.nsplits
    ns = (N - split + S - 1) // S
    s = md.reserved if md.kind == _lib.MOVE_WALK else 0
    nh = s if s >= 2 else (1 if md.kind == _lib.MOVE_KDE else 0)
    nz = s if s >= 2 else D
    h = np.zeros(max(ns * nh, 1), dtype=np.int32)
    z = np.empty(max(ns * nz, 1))
    assert _lib.load().emx_host_walk_kde_draws(seed, step, N, D, C.byref(md), split, h.ctypes.data_as(C.c_void_p), z) == ns
    return h[:ns * nh].reshape(ns, nh), z[:ns * nz].reshape(ns, nz)


def open_ens(x, md, step, lp=None, seed=SEED):
    N, D = x.shape
    ens = DeviceEnsemble(N, D)
    ens.set_target(_lib.TARGET_HOST)
    ens.set_moves([md], np.array([1.0]))
    ens.set_rng_mode(_lib.RNG_PHILOX)
    ens.set_philox(seed, step)
    ens.set_state(x, np.zeros(N) if lp is None else lp)
    return ens


def kappa_of(S):
    """sqrt(cond) of the correlation matrix of the columns that have a variance"""
    Sf = hp.to_float(S)
    keep = np.diag(Sf) > 0
    if not keep.any():
        return 1.0
    sd = np.sqrt(np.diag(Sf)[keep])
    Cr = Sf[np.ix_(keep, keep)] / sd[:, None] / sd[None, :]
    ev = np.linalg.eigvalsh(Cr)
    return float(np.sqrt(ev[-1] / max(ev[0], 1e-300))) if ev[0] > 0 else 1.0


def reference(md, x, plan, split, step, slots=None, seed=SEED):
    """-> dict(t (slot indices checked), q, qbound, and for KDE f, fbound) for split `split` of a step whose plan is `plan`,
    computed from the ensemble x the split saw"""
    N, D = x.shape
    off, order = plan["off"], plan["order"]
    members = order[off[split]:off[split + 1]]
    comp = np.concatenate([order[off[j]:off[j + 1]] for j in range(len(off) - 1) if j != split])
    h, z = host_draws(md, N, D, split, step, seed)
    ns = len(members)
    t = np.arange(ns) if slots is None or slots >= ns else np.sort(np.random.RandomState(ns + step).choice(ns, slots, replace=False))
    xm = x[members[t]]
    out = dict(t=t)
    if md.kind == _lib.MOVE_WALK and md.reserved >= 2:
        s = md.reserved
        c = x[h[t]]                                                  # (n, s, D)
        q, w = hp.walk_s_proposal(xm, c, z[t])
        spread = np.abs(c - xm[:, None, :]).max(axis=1)
        W = np.abs(w).max(axis=1) + np.abs(z[t]).max(axis=1) / np.sqrt(s - 1.0)
        out.update(q=q, qbound=C_WALK_S * EPS * (np.abs(xm) + s * W[:, None] * spread))
        return out
    mu, S = hp.complement_stats(x[comp])
    kap = kappa_of(S)
    if md.kind == _lib.MOVE_WALK:
        L = hp.cholesky(S, semidefinite=True)
        base = xm
    else:
        hb = hp.kde_bandwidth(md.reserved, len(comp), D, md.a)
        L = hp.mul(hp.cholesky(S, semidefinite=False), (np.full((D, D), hb[0]), np.full((D, D), hb[1])))
        base = x[h[t, 0]]
    q = hp.linear_proposal(base, L, z[t])
    LZ = np.abs(hp.to_float(L)) @ np.abs(z[t]).T
    out.update(q=q, qbound=EPS * np.abs(q) + C_LIN * EPS * (D + 8) * kap * LZ.T, L=hp.to_float(L), kappa=kap)
    if md.kind == _lib.MOVE_KDE:
        rank = np.empty(N, dtype=np.int64)
        rank[comp] = np.arange(len(comp))
        f, R = hp.kde_log_ratio(mu, L, x[comp], xm, rank[h[t, 0]], z[t])
        out.update(f=f, fbound=C_KDE * EPS * (D + 8) * kap * (1 + R * R), R=R)
    return out


def assert_split(md, x, plan, split, step, q, f, slots=48, seed=SEED, what=""):
    ref = reference(md, x, plan, split, step, slots, seed)
    t = ref["t"]
    err = np.abs(q[t] - ref["q"])
    bad = err > ref["qbound"]
    assert not bad.any(), "%s split %d: proposal off by %.3g x its bound (%d entries), max err %.3g" % (
        what, split, (err / np.maximum(ref["qbound"], 1e-300)).max(), bad.sum(), err.max())
    if "f" in ref:
        ferr = np.abs(f[t] - ref["f"])
        assert np.all(ferr <= ref["fbound"]), "%s split %d: KDE factor off by %.3g (bound %.3g, R %.3g)" % (
            what, split, ferr.max(), ref["fbound"], ref["R"])
    elif md.kind == _lib.MOVE_WALK:
        assert np.all(f == 0)
    return ref


def propose_all(x, md, step, slots=48, seed=SEED, what=""):
    """one step, every split rejected (each split sees x): the proposals against the reference"""
    ens = open_ens(x, md, step, seed=seed)
    try:
        _, nsplits = ens.step_begin(False)
        assert nsplits == md.nsplits
        plan = ens.plan_get(nsplits)
        qs = []
        for split in range(nsplits):
            q, f = ens.propose(split, with_factors=True)
            qs.append((q.copy(), f.copy()))
            ens.accept(split, np.full(len(q), -np.inf))
        ens.step_end()
        ens.raise_on_status()
    finally:
        ens.close()
    for split, (q, f) in enumerate(qs):
        assert_split(md, x, plan, split, step, q, f, slots, seed, what)
    return plan, qs


# ---- the shape sweep ---------------------------------------------------------------------------------------------------------
NDIMS = [1, 2, 3, 5, 8, 31, 32, 33, 63, 64, 65, 100, 127, 128]
S_VALUES = [2, 3, 63, 64, 65, 1024, "min"]
BWS = [None, "silverman", 0.05, 3.0]


def _sweep_cases():
    """every ndim with each move family; N, nsplits, randomize_split, s and the bandwidth drawn from a seeded stream"""
    rs = np.random.RandomState(20261016)
    cases = []
    for i, D in enumerate(NDIMS):
        lo = 2 * D + 3
        for fam in ("walk_s", "walk0", "kde"):
            nsplits = int(rs.choice([2, 3, 4]))
            rnd = int(rs.randint(2))
            if fam == "walk_s":
                s = S_VALUES[i % len(S_VALUES)]
                if s == 1024 and D > 33:
                    s = 65
                need = (1024 if s == 1024 else 65) + 2
            else:
                s, need = None, 0
            kind = rs.randint(3)            # near 2 ndim (odd), odd, not a multiple of 16
            N = [lo | 1, 2 * int(rs.randint(lo, 6 * D + 40)) + 1, int(rs.randint(lo, 8 * D + 60)) // 16 * 16 + 7][kind]
            if nsplits > 2:
                N = max(N, nsplits * (D + 2) + 1)
            if fam == "walk_s":
                N = max(N, nsplits * need // (nsplits - 1) + 3)
                if s == "min":
                    s = N - (N + nsplits - 1) // nsplits
                s = min(int(s), N - (N + nsplits - 1) // nsplits)
            cases.append((fam, D, N, nsplits, rnd, s, BWS[i % len(BWS)]))
    cases.append(("walk_s", 4, 66000, 2, 1, 64, None))              # complements above 32 768 rows: 128 slices
    cases.append(("walk0", 4, 66000, 2, 0, None, None))
    cases.append(("kde", 4, 66001, 2, 1, None, "silverman"))
    return cases


def _data(D, N, seed, offset=0.0):
    rs = np.random.RandomState(seed)
    A = np.eye(D) + 0.3 * rs.randn(D, D) / np.sqrt(D)
    return offset + rs.randn(N, D) @ A.T * (1 + np.arange(D) % 3)


@pytest.mark.parametrize("fam,D,N,nsplits,rnd,s,bw", _sweep_cases())
def test_shape_sweep_against_reference(fam, D, N, nsplits, rnd, s, bw):
    x = _data(D, N, D * 7919 + N)
    md = walk(s, nsplits, rnd) if fam == "walk_s" else walk(None, nsplits, rnd) if fam == "walk0" else kde(bw, nsplits, rnd)
    propose_all(x, md, step=N % 97, slots=48 if D <= 33 and N < 60000 else 16, what=fam)


# ---- conditioning edges --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [64, 1024])
def test_walk_offset_coordinates(s):
    """a common offset of 2^21 with a spread of 2^-13 (an epoch in days with a tight posterior): the step must be accurate to the
    spread, not to the offset"""
    N, D = 2 * s + 301, 3
    rs = np.random.RandomState(s)
    x = 2.0 ** 21 + rs.randn(N, D) * 2.0 ** -13
    propose_all(x, walk(s), step=5, slots=None, what="offset")


def test_walk_whole_complement_offset_and_scaled_coordinates():
    """standard deviations 1e4 and 1e-4 side by side, and an offset: every coordinate moves, by its own scale"""
    N, D = 301, 4
    rs = np.random.RandomState(11)
    x = rs.randn(N, D) * np.array([1e4, 1e-4, 1.0, 2.0 ** -13]) + np.array([0.0, 0.0, 0.0, 2.0 ** 21])
    plan, qs = propose_all(x, walk(None), step=3, slots=None, what="scaled")
    for split, (q, _) in enumerate(qs):
        members = plan["order"][plan["off"][split]:plan["off"][split + 1]]
        assert np.all(np.any(q != x[members], axis=0))


@pytest.mark.parametrize("fam", ["walk_s", "walk0", "kde"])
def test_outlying_walkers(fam):
    """a few walkers 50 sigma away from the rest"""
    N, D = 203, 5
    x = _data(D, N, 13)
    x[::40] += 50.0 * np.array([1, -1, 1, 1, -1])
    md = walk(8) if fam == "walk_s" else walk(None) if fam == "walk0" else kde()
    propose_all(x, md, step=9, slots=None, what="outliers")


@pytest.mark.parametrize("bw", [1e-3, 1e-2])
def test_kde_tiny_bandwidth_and_underflowing_terms(bw):
    """a tiny bandwidth: every LSE term but the nearest underflows against the maximum"""
    N, D = 157, 3
    x = _data(D, N, 17)
    propose_all(x, kde(bw), step=4, slots=None, what="tiny bw")


def test_constant_coordinate():
    """the walk keeps a constant coordinate fixed; KDE's covariance is singular (scipy: LinAlgError)"""
    N, D = 99, 4
    x = _data(D, N, 19)
    x[:, 2] = 0.75
    for md in (walk(None), walk(5)):
        plan, qs = propose_all(x, md, step=2, slots=None, what="constant")
        for q, _ in qs:
            assert np.all(q[:, 2] == 0.75)
    ens = open_ens(x, kde(), 2)
    try:
        ens.step_begin(False)
        ens.propose(0, with_factors=True)
        with pytest.raises(np.linalg.LinAlgError):
            ens.raise_on_status()
    finally:
        ens.close()


def test_collinear_coordinates_walk_keeps_the_column_space():
    N, D = 121, 4
    x = _data(D, N, 23)
    x[:, 3] = 2.0 * x[:, 1]                      # exactly collinear (doubling is exact: so are the centred rows)
    plan, qs = propose_all(x, walk(None), step=6, slots=None, what="collinear")
    for split, (q, _) in enumerate(qs):
        members = plan["order"][plan["off"][split]:plan["off"][split + 1]]
        d = q - x[members]
        scale = np.abs(d).max()
        assert np.all(np.abs(d[:, 3] - 2.0 * d[:, 1]) <= 64 * EPS * (scale + np.abs(x).max()))


# ---- updates between splits, decisions -------------------------------------------------------------------------------------------
def target_lp(x, mu, ivar):
    return -0.5 * np.sum((x - mu) ** 2 * ivar, axis=1)


def run_checked_step(ens, md, step, lp_fn, slots=None, choose=None):
    """one step through the step API: each split's proposals and factors against the reference from the ensemble it sees, then
    the Metropolis decisions against f_ref + lp_new - lp_old > log(u) (margins below 1e-9 excepted) and the committed state"""
    N, D = ens.nwalkers, ens.ndim
    _, nsplits = ens.step_begin(False)
    plan = ens.plan_get(nsplits)
    accepted = 0
    for split in range(nsplits):
        x, lp = ens.get_state()
        q, f = ens.propose(split, with_factors=True)
        q, f = q.copy(), f.copy()
        ref = assert_split(md, x, plan, split, step, q, f, slots, what="step %d" % step)
        members = plan["order"][plan["off"][split]:plan["off"][split + 1]]
        logu = np.log(plan["uacc"][plan["off"][split]:plan["off"][split + 1]])
        fr = f.copy()
        if "f" in ref:
            fr[ref["t"]] = ref["f"]
        lp_new = lp_fn(q) if choose is None else choose(f, lp[members], logu)
        ens.accept(split, lp_new)
        x2, lp2 = ens.get_state()
        margin = fr + lp_new - lp[members] - logu
        acc = np.any(x2[members] != x[members], axis=1) | (lp2[members] != lp[members])
        sure = np.abs(margin) > 1e-9
        assert np.array_equal(acc[sure], margin[sure] > 0), "decisions differ from the reference rule"
        want = x.copy()
        want[members[acc]] = q[acc]
        assert np.array_equal(x2, want)
        wl = lp.copy()
        wl[members[acc]] = lp_new[acc]
        assert np.array_equal(lp2, wl)
        accepted += int(acc.sum())
    ens.step_end()
    ens.raise_on_status()
    return accepted


@pytest.mark.parametrize("md", [walk(3), walk(None, 3), kde(nsplits=2), kde("silverman", 4)],
                         ids=["walk3", "walk0_3splits", "kde", "kde_4splits"])
def test_later_splits_see_earlier_updates(md):
    """accept a known subset of split 0 (finite log-probs placed 0.5 above or below the acceptance threshold): split 1's
    complement statistics and helpers must be those of the updated ensemble"""
    N, D = 157, 5
    x = _data(D, N, 29)
    rs = np.random.RandomState(31)

    def choose(f, lp_old, logu):
        return lp_old + logu - f + np.where(rs.rand(len(f)) < 0.5, 0.5, -0.5)
    ens = open_ens(x, md, 7)
    try:
        assert run_checked_step(ens, md, 7, None, choose=choose) > 0
    finally:
        ens.close()


@pytest.mark.parametrize("md,N,D", [(walk(4), 131, 6), (walk(None), 96, 7), (kde(), 203, 3)], ids=["walk4", "walk0", "kde"])
def test_twenty_step_replay(md, N, D):
    rs = np.random.RandomState(N)
    mu, ivar = rs.randn(D), rs.uniform(0.5, 2.0, D)
    x = mu + rs.randn(N, D) / np.sqrt(ivar) * 1.5
    lp_fn = lambda q: target_lp(q, mu, ivar)             # noqa: E731
    ens = open_ens(x, md, 0, lp=lp_fn(x))
    try:
        acc = sum(run_checked_step(ens, md, step, lp_fn) for step in range(20))
    finally:
        ens.close()
    assert 0.05 * 20 * N < acc < 0.99 * 20 * N


# ---- exact scale covariance ------------------------------------------------------------------------------------------------------
def _pow2_scales(D, seed):
    e = np.random.RandomState(seed).permutation(np.linspace(-24, 24, D).round().astype(int))
    return 2.0 ** e


@pytest.mark.parametrize("md,N,D", [(walk(3), 150, 6), (walk(None), 150, 6), (walk(None, 3), 97, 12), (kde(), 150, 5),
                                    (kde(0.3, 3), 121, 4)], ids=["walk3", "walk0", "walk0_3splits", "kde", "kde_bw"])
def test_walk_kde_scale_covariance(md, N, D):
    """coordinates scaled by powers of two from 2^-24 to 2^24, the target with them: the same chain times the scales, bit for bit"""
    p = _pow2_scales(D, N + D)
    rs = np.random.RandomState(D)
    mu, ivar = rs.randn(D), rs.uniform(0.5, 2.0, D)
    x0 = mu + rs.randn(N, D) / np.sqrt(ivar)
    runs = []
    for sc in (np.ones(D), p):
        m, iv = mu * sc, ivar / (sc * sc)
        x = x0 * sc
        ens = open_ens(x, md, 0, lp=target_lp(x, m, iv))
        rec = []
        try:
            for _ in range(6):
                _, nsplits = ens.step_begin(False)
                for split in range(nsplits):
                    q, f = ens.propose(split, with_factors=True)
                    lp_new = target_lp(q, m, iv)
                    ens.accept(split, lp_new)
                    rec.append((q.copy(), f.copy(), lp_new, ens.accepted_mask()))
                ens.step_end()
            ens.raise_on_status()
            rec.append(ens.get_state())
        finally:
            ens.close()
        runs.append(rec)
    for (qa, fa, la, aa), (qb, fb, lb, ab) in zip(runs[0][:-1], runs[1][:-1]):
        assert np.array_equal(qa * p, qb) and np.array_equal(fa, fb) and np.array_equal(la, lb) and np.array_equal(aa, ab)
    assert np.array_equal(runs[0][-1][0] * p, runs[1][-1][0]) and np.array_equal(runs[0][-1][1], runs[1][-1][1])
    assert any(r[3].any() for r in runs[0][:-1])


def _dense(D, seed):
    rs = np.random.RandomState(seed)
    A = rs.randn(D, D) / np.sqrt(D)
    cov = A @ A.T + np.eye(D)
    return rs.randn(D), np.linalg.inv(cov), cov


# (target, N, D, move, path) -- path: how persist_info must read after the run
PATHS = [("diag", 64, 5, "stretch", "small"), ("diag", 64, 5, "de", "small"),
         ("dense", 256, 24, "stretch", "launches"), ("dense", 256, 24, "de", "launches"),
         ("dense", 1024, 32, "stretch", "persist"), ("dense", 1024, 32, "de", "persist"),
         ("dense", 1024, 27, "stretch", "persist"), ("dense", 1024, 27, "de", "persist"),       # odd ndim: emx_podd.hip
         ("dense", 1024, 100, "stretch", "persist"), ("dense", 1024, 100, "de", "persist"),     # padded ndim 112: the slab form
         ("diag", 1024, 6, "stretch", "persist"), ("diag", 1024, 6, "de", "persist")]          # element-wise: emx_pvalu.hip


def _sampler_run(target, N, D, move, sc, nsteps=24):
    if target == "diag":
        rs = np.random.RandomState(D)
        mu, ivar = rs.randn(D), rs.uniform(0.5, 2.0, D)
        tgt = targets.DiagGaussian(mu * sc, ivar / (sc * sc))
        p0 = mu + rs.randn(N, D) / np.sqrt(ivar)
    else:
        mu, icov, cov = _dense(D, D)
        tgt = targets.DenseGaussian(mu * sc, icov / np.outer(sc, sc))
        p0 = mu + np.random.RandomState(D + 1).randn(N, D) @ np.linalg.cholesky(cov).T
    mv = moves.StretchMove() if move == "stretch" else moves.DEMove()
    s = emcee_amd.EnsembleSampler(N, D, tgt, moves=mv, rng="philox")
    s.random_state = np.random.RandomState(77).get_state()
    s.run_mcmc(p0 * sc, nsteps, skip_initial_state_check=True)
    return s


@pytest.mark.parametrize("target,N,D,move,path", PATHS)
def test_stretch_de_scale_covariance_on_every_path(target, N, D, move, path):
    """a coordinate mix-up in any kernel breaks this at once (an isotropic target would not show it)"""
    p = _pow2_scales(D, N + D)
    a = _sampler_run(target, N, D, move, np.ones(D))
    b = _sampler_run(target, N, D, move, p)
    info = b._ens.persist_info()
    if path == "persist":
        assert info["qualifies"] and info["launches"] >= 1, info
    else:
        assert info["launches"] == 0, info
    assert np.array_equal(a.get_chain() * p, b.get_chain())
    assert np.array_equal(a.get_log_prob(), b.get_log_prob())
    assert np.array_equal(a.acceptance_fraction, b.acceptance_fraction)
    assert 0 < np.mean(a.acceptance_fraction) < 1


@pytest.mark.parametrize("move", ["stretch", "de"])
def test_stretch_de_scale_covariance_in_a_batch(move):
    B, N, D = 3, 64, 5
    p = _pow2_scales(D, 5)
    rs = np.random.RandomState(41)
    mu, ivar = rs.randn(D), rs.uniform(0.5, 2.0, D)
    p0 = mu + rs.randn(B, N, D) / np.sqrt(ivar)
    out = []
    for sc in (np.ones(D), p):
        mv = moves.StretchMove() if move == "stretch" else moves.DEMove()
        b = emcee_amd.EnsembleBatch(B, N, D, targets.DiagGaussian(mu * sc, ivar / (sc * sc)), moves=mv, seeds=[1, 2, 3])
        b.run_mcmc(p0 * sc, 30, skip_initial_state_check=True)
        assert b.launch_info()["launches"] >= 1
        out.append((b.get_chain(), b.get_log_prob()))
    assert np.array_equal(out[0][0] * p, out[1][0]) and np.array_equal(out[0][1], out[1][1])
