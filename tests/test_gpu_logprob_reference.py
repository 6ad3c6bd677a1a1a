"""Every kernel that evaluates a built-in log-probability against the double-double reference of tests/hiprec.py, inside the
forward-error bounds derived in tests/lp_families.py (which scale with what the arithmetic loses, never with the magnitude of the
coordinates), on the input families of that file: benign, next to a mean of 2^21, ill-conditioned, asymmetric icov, the Rosenbrock
valley, power-of-two scaled, and out of the double range.

The eval kernel is swept over ndim (every padding edge of the row layouts and of the 16-column MFMA tiles, and the wide kernels
beyond padded ndim 128); every sampling path runs 24 stored Philox steps through EnsembleSampler / EnsembleBatch, and the log-probs
stored for the start state, two middle steps and the last step must lie within the bound of the reference at the coordinates stored
with them.  Each run asserts the path it took.  Every test prints its worst error / bound."""
import numpy as np
import pytest

import emcee_amd
from emcee_amd import _lib, moves, targets
from emcee_amd.device import DeviceEnsemble

import lp_families as lpf

pytestmark = pytest.mark.gpu

NDIMS = [1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 112, 113, 127, 128, 129, 200, 257]
NSTEPS = 24
CHECK_STEPS = (7, 15, NSTEPS - 1)


def report(path, family, r):
    print("logprob-reference: %-28s %-8s worst error / bound %.3g" % (path, family, float(np.max(r)) if len(r) else 0.0))


def set_target(ens, t):
    k = t["kind"]
    if k == "iso":
        ens.set_target(_lib.TARGET_ISO)
    elif k == "diag":
        ens.set_target(_lib.TARGET_DIAG, t["mu"], t["ivar"])
    elif k == "dense":
        ens.set_target(_lib.TARGET_DENSE, t["mu"], t["icov"])
    elif k == "rosenbrock":
        ens.set_target(_lib.TARGET_ROSENBROCK, scale=t["scale"])
    else:
        ens.set_target(_lib.TARGET_BOX)


def target_of(t):
    k = t["kind"]
    if k == "iso":
        return targets.IsoGaussian()
    if k == "diag":
        return targets.DiagGaussian(t["mu"], t["ivar"])
    if k == "dense":
        return targets.DenseGaussian(t["mu"], t["icov"])
    if k == "rosenbrock":
        return targets.Rosenbrock(t["scale"])
    return targets.UniformBox()


def assert_within(got, t, x, path):
    r = lpf.ratio(np.asarray(got), t, x)
    report(path, t["family"], r)
    assert r.max() <= 1.0, "%s, %s family, ndim %d: log-prob off by %.3g x its bound (%d of %d rows)" % (
        path, t["family"], t["D"], r.max(), int((r > 1).sum()), len(r))
    return r.max()


EVAL_CASES = [(k, f, D) for f in sorted(lpf.FAMILIES) for k in lpf.FAMILIES[f] for D in NDIMS if D <= 128 or f in ("benign", "offset")]


@pytest.mark.parametrize("kind,family,D", EVAL_CASES)
def test_eval_kernel_within_the_bound(kind, family, D):
    """eval_log_prob on 77 rows (a partial block) and eval_state_log_prob on 200"""
    t = lpf.make(kind, family, D, 200)
    x = t["x"]
    ens = DeviceEnsemble(200, D)
    try:
        set_target(ens, t)
        got77 = ens.eval_log_prob(x[:77])
        ens.set_state(x)
        ens.eval_state_log_prob()
        got = ens.get_state()[1]
        assert ens.status() == 0
    finally:
        ens.close()
    assert np.array_equal(got77, got[:77])
    assert_within(got, t, x, "eval %s %d" % (kind, D))


@pytest.mark.parametrize("kind", ["iso", "diag", "dense"])
@pytest.mark.parametrize("D", [1, 5, 17, 64, 100, 130])
def test_eval_kernel_out_of_range_is_minus_infinity_and_not_nan(kind, D):
    """|x| = 1e160: the log-prob is about -1e320.  The reference is taken on the rows scaled by 2^-600 (exact), where it is finite:
    times 2^1200 it exceeds the double range, so the device must return -inf, and no NaN bit, as NumPy does"""
    t = lpf.make(kind, "benign", D, 40)
    rs = np.random.RandomState(D)
    x = 1e160 * rs.choice([-1.0, 1.0], (40, D)) * rs.uniform(0.5, 2.0, (40, D))
    small = dict(t)
    if kind != "iso":
        small["mu"] = t["mu"] * 2.0 ** -600
    ref = lpf.reference(small, x * 2.0 ** -600)[0]
    assert np.all(np.log2(-ref) + 1200 > 1025)
    ens = DeviceEnsemble(40, D)
    try:
        set_target(ens, t)
        got = ens.eval_log_prob(x)
        ens.set_state(x)
        ens.eval_state_log_prob()
        got2 = ens.get_state()[1]
        status = ens.status()
    finally:
        ens.close()
    assert np.all(got == -np.inf) and np.all(got2 == -np.inf), got
    assert not status & 1, "NaN bit"


def test_role_split_wide_kernel_within_the_bound():
    """k_wide_lp_ws takes over from 8 row tiles a CU: the smallest ensemble whose half-steps reach it, ndim 130; a seeded sample of the
    rows (the ragged last tile among them) after the evaluation of the state and after two stretch steps"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    D, N = 130, 2 * (8 * cus * 16) + 32
    for family in ("benign", "offset"):
        t = lpf.make("dense", family, D, 256)
        rs = np.random.RandomState(5)
        x = t["mu"] + rs.randn(N, D) @ t["chol_cov"].T
        pick = np.concatenate([np.sort(rs.choice(N - 16, 600, replace=False)), np.arange(N - 16, N)])
        ens = DeviceEnsemble(N, D)
        try:
            set_target(ens, t)
            ens.set_moves([_lib.MoveDesc(_lib.MOVE_STRETCH, 2, 1, 0, 2.0, 0.0, 0.0, 0.0)], np.array([1.0]))
            ens.set_state(x)
            ens.eval_state_log_prob()
            lp0 = ens.get_state(coords=False)[1]
            ens.set_rng_mode(_lib.RNG_PHILOX)
            ens.set_philox(77, 0)
            ens.run(2, 1, False)
            assert ens.status() == 0 and ens.persist_info()["launches"] == 0
            x1, lp1 = ens.get_state()
        finally:
            ens.close()
        assert np.any(x1[pick] != x[pick]) and np.any(x1[pick] == x[pick])
        assert_within(lp0[pick], t, x[pick], "wide role-split, eval")
        assert_within(lp1[pick], t, x1[pick], "wide role-split, 2 steps")


# ---- the sampling paths -------------------------------------------------------------------------------------------------------
# name -> (target kind, N, D, move, tunings, the path persist_info / small_info must show)
PATHS = {
    "small dense 64x8": ("dense", 64, 8, "stretch", {}, "small"),
    "small diag 64x5": ("diag", 64, 5, "stretch", {}, "small"),
    "fused launches 256x24": ("dense", 256, 24, "stretch", {}, "launches"),
    "launch slab 256x100": ("dense", 256, 100, "stretch", {"slab": 1}, "launches"),
    "k_persist 1024x32 stretch": ("dense", 1024, 32, "stretch", {}, "persist"),
    "k_persist 1024x32 de": ("dense", 1024, 32, "de", {}, "persist"),
    "k_persist odd 1024x27": ("dense", 1024, 27, "stretch", {}, "persist"),
    "k_persist_slab 1024x100": ("dense", 1024, 100, "stretch", {}, "persist"),
    "k_persist_slab odd 1024x97": ("dense", 1024, 97, "stretch", {}, "persist"),
    "k_persist_mix 1024x32": ("dense", 1024, 32, "de+snooker", {}, "mix"),
    "k_persist_gauss 1024x16": ("dense", 1024, 16, "gauss", {}, "persist"),
    "k_persist_valu diag 1024x6": ("diag", 1024, 6, "stretch", {}, "persist"),
    "k_persist_valu diag 1024x5": ("diag", 1024, 5, "stretch", {}, "persist"),
    "k_persist_valu rosenbrock 1024x6": ("rosenbrock", 1024, 6, "stretch", {}, "persist"),
    "k_persist_valu iso 1024x10": ("iso", 1024, 10, "stretch", {}, "persist"),
    "wide multi-wave 48x130": ("dense", 48, 130, "stretch", {}, "launches"),               # k_wide_lp_ms: few row tiles, two macro blocks
    "wide single-role 48x130": ("dense", 48, 130, "stretch", {"dense_wide": 2}, "launches"),     # k_wide_lp
    "wide single-role 1024x32": ("dense", 1024, 32, "stretch", {"dense_wide": 2}, "launches"),   # k_wide_lp where the fused kernel would run
}
RUN_FAMILIES = {"dense": ("benign", "offset", "illcond", "asym"), "diag": ("benign", "offset"), "rosenbrock": ("benign", "valley"),
                "iso": ("benign",)}
RUN_CASES = [(name, f) for name, p in PATHS.items() for f in RUN_FAMILIES[p[0]]]


def _moves_for(move, t):
    D = t["D"]
    if move == "stretch":
        return moves.StretchMove(live_dangerously=True)
    if move == "de":
        return moves.DEMove(live_dangerously=True)
    if move == "de+snooker":
        return [(moves.DEMove(), 0.5), (moves.DESnookerMove(), 0.5)]
    # GaussianMove, vector mode: steps of the target's narrowest direction, so that some are accepted on every family
    A = 0.5 * (t["icov"] + t["icov"].T)
    return moves.GaussianMove(np.full(D, 1.0 / (D * np.linalg.eigvalsh(A)[-1])), mode="vector")


def _move_runs(sampler, nsteps, nmoves):
    """runs of consecutive steps of one move in the schedule the device drew"""
    lib = _lib.load()
    cdf = np.cumsum(np.full(nmoves, 1.0 / nmoves))
    cdf /= cdf[-1]
    seed = sampler._philox_seed()
    ks = [lib.emx_host_move_choice_philox(seed, step, cdf, len(cdf)) for step in range(nsteps)]
    return 1 + sum(1 for a, b in zip(ks, ks[1:]) if a != b), ks


@pytest.mark.parametrize("name,family", RUN_CASES)
def test_sampling_path_within_the_bound(name, family):
    kind, N, D, move, tune, path = PATHS[name]
    t = lpf.make(kind, family, D, N)
    p0 = t["x"]
    s = emcee_amd.EnsembleSampler(N, D, target_of(t), moves=_moves_for(move, t), rng="philox")
    s.random_state = np.random.RandomState(77).get_state()
    ens = s._device_ensemble()
    for k, v in tune.items():
        ens.set_tuning(k, v)
    s.run_mcmc(p0, NSTEPS, skip_initial_state_check=True)
    info, small = ens.persist_info(), ens.small_info()
    chain, lps = s.get_chain(), s.get_log_prob()
    lp0 = s.compute_log_prob(p0)[0]
    acc = s.acceptance_fraction
    assert chain.shape == (NSTEPS, N, D) and lps.shape == (NSTEPS, N)
    if path == "small":
        assert small["launches"] >= 1 and small["steps"] >= NSTEPS and info["launches"] == 0, (small, info)
    elif path == "launches":
        assert small["launches"] == 0 and info["launches"] == 0, (small, info)
    elif path == "persist":
        assert small["launches"] == 0 and info["qualifies"] and info["launches"] >= 1 and info["recovered"] == 0, (small, info)
        if kind == "dense":
            assert info["halfsteps"] == (1 if move == "gauss" else 2) * NSTEPS, info
        else:
            assert info["halfsteps"] >= NSTEPS, info
    else:
        runs, ks = _move_runs(s, NSTEPS, 2)
        assert small["launches"] == 0 and info["qualifies"] and info["recovered"] == 0, (small, info)
        assert NSTEPS < info["halfsteps"] <= sum(2 if k == 0 else 4 for k in ks) and runs >= 6, (info, runs)
        assert 1 <= info["launches"] < runs, (info, runs)             # steps of both moves shared launches: k_persist_mix
    assert 0 < acc.sum() and np.all(acc <= 1) and acc.mean() < 1, "the run must accept something and reject something"
    assert np.any(chain[-1] != p0)
    worst = assert_within(lp0, t, p0, name + ", start")
    for step in CHECK_STEPS:
        worst = max(worst, assert_within(lps[step], t, chain[step], name + ", step %d" % step))
    report(name + ", ALL", family, np.array([worst]))


BATCH_CASES = [(k, f) for k in ("dense", "diag") for f in RUN_FAMILIES[k]]


@pytest.mark.parametrize("kind,family", BATCH_CASES)
def test_ensemble_batch_within_the_bound(kind, family):
    """emx_batch.hip, B = 3 members of 64 x 5: steps 0 (walkers that did not move there carry the log-prob of the start state), 7, 15, 23"""
    B, N, D = 3, 64, 5
    t = lpf.make(kind, family, D, B * N)
    p0 = t["x"].reshape(B, N, D)
    b = emcee_amd.EnsembleBatch(B, N, D, target_of(t), moves=moves.StretchMove(), seeds=[1, 2, 3])
    b.run_mcmc(p0, NSTEPS, skip_initial_state_check=True)
    assert b.launch_info()["launches"] >= 1
    chain, lps = b.get_chain(), b.get_log_prob()
    acc = b.acceptance_fraction
    assert chain.shape == (B, NSTEPS, N, D) and 0 < acc.mean() < 1
    stayed = np.all(chain[:, 0] == p0, axis=2)
    assert stayed.any() and not stayed.all()
    for step in (0,) + CHECK_STEPS:
        assert_within(lps[:, step].reshape(-1), t, chain[:, step].reshape(-1, D), "EnsembleBatch %s, step %d" % (kind, step))
