"""The device's Philox stream against its NumPy definition (tests/philox_ref.py, which imports nothing of the library and is held
to the host twins, and shown to catch fifteen plausible mistakes, by tests/test_philox_ref_cpu.py).

The plans k_native_plan_batch evaluates (read back with emx_plan_get), the move step_begin chooses, the Gaussian move's column and
step-size factor and one tempering swap pass, compared under the reference's rules: integers, uacc and the stretch z bit for bit;
DE's s0 within the bound the reference derives for the platform's log, sqrt and cos (no rtol anywhere else); the swap pass's stored
logarithms within one ulp of the long-double logarithm.

Paths that make their entries in flight expose no plan -- k_persist, k_small_run, k_batch_cb, k_pt_run and the fused kernels -- and
are already held bit for bit to the path tested here; no run is added for them.  The links:
  k_persist      test_gpu_persist.py::test_persistent_kernel_gives_the_bits_of_the_launch_per_halfstep_path (and its siblings there),
                 test_gpu_persist.py::test_persistent_kernel_equals_the_oracle_at_the_headline_size
  k_small_run    test_gpu_small_run.py::test_small_run_equals_general_path, ..._de_and_snooker_..., ..._gaussian_move_...
  k_batch_cb     test_gpu_batch_callback.py::test_members_equal_single_sampler (k_batch: test_gpu_batch.py, the same name)
  k_pt_run       test_gpu_pt.py::test_without_swaps_every_rung_is_the_batch_member_of_its_tempered_callable
  fused kernels  test_gpu_batch_fused.py / test_gpu_pt_fused.py::test_fused_equals_the_callback_path,
                 test_gpu_ensemble_fused_small.py (k_small_run of a DeviceFused target against the launch per half-step),
                 test_gpu_one_workgroup_bits.py (the Philox-mode hashes of tests/golden/one_workgroup_bits.json)
The Walk/KDE helper, centre and normal draws of the device are held to emx_host_walk_kde_draws by test_gpu_walk_kde_reference.py,
and that twin to the reference by the CPU file.
"""
import numpy as np
import pytest

from emcee_amd import _lib
from emcee_amd.device import DeviceEnsemble

import gauss_noise_ref as gr
import philox_ref as pr
from emx_testlib import cdf_of

pytestmark = pytest.mark.gpu

KEYS = [(0xC0FFEE, 0), (2 ** 63 + 5, 2 ** 32 - 2)]
NSTEPS = 20                      # crosses a k_native_plan_batch boundary (16 steps) and, from 2^32 - 2, the carry into the high step word
SIGMA, G0 = 0.5, 0.4
WORST = {"de": 0.0}


def open_ens(N, D, descs, weights, seed, step0):
    ens = DeviceEnsemble(N, D)
    ens.set_target(_lib.TARGET_ISO)
    ens.set_moves(descs, cdf_of(weights, len(descs)))
    ens.set_state(0.5 * np.random.RandomState(N + D).randn(N, D))
    ens.eval_state_log_prob()
    ens.set_rng_mode(_lib.RNG_PHILOX)
    ens.set_philox(seed, step0)
    return ens


def desc(kind, S=2, a=2.0, s=0):
    code = dict(stretch=_lib.MOVE_STRETCH, de=_lib.MOVE_DE, snooker=_lib.MOVE_SNOOKER, walk=_lib.MOVE_WALK)[kind]
    if kind == "walk":
        return _lib.MoveDesc(code, S, 1, s, 0.0, 0.0, 0.0, 0.0)
    return _lib.MoveDesc(code, S, 1, 0, a, SIGMA, G0, 1.7)


def assert_plan(got, ref, kind, what):
    for key in ("off", "order", "p0", "p1", "p2"):
        assert np.array_equal(got[key], ref[key]), (what, key)
    assert np.array_equal(got["uacc"], ref["uacc"]), (what, "uacc")
    if kind == "de":
        err = np.abs(got["s0"].astype(pr.LD) - ref["s0_ref"]).astype(np.float64)
        ratio = float(np.max(err / ref["s0_bound"]))
        WORST["de"] = max(WORST["de"], ratio)
        assert ratio <= 1.0, "%s: DE s0 off by %.3g x its bound" % (what, ratio)
    else:
        assert np.array_equal(got["s0"], ref["s0"]), (what, "s0")


def run_steps(ens, nsteps, check):
    """per step: step_begin, the plan the device made, the half-steps"""
    for i in range(nsteps):
        k, S = ens.step_begin(store=False)
        check(i, k, S, ens.plan_get(S))
        for s in range(S):
            ens.halfstep(s)
        ens.step_end()
        assert ens.status() == 0


# ---- plans ----------------------------------------------------------------------------------------------------------------------
PLAN_CASES = [("stretch", 33, 3, 2, 2.0), ("stretch", 50, 3, 3, 3.0), ("de", 34, 4, 2, 2.0), ("snooker", 67, 4, 4, 2.0),
              ("walk", 40, 3, 2, 2.0)]


@pytest.mark.parametrize("seed,step0", KEYS)
@pytest.mark.parametrize("kind,N,D,S,a", PLAN_CASES)
def test_device_plans_equal_the_definition(kind, N, D, S, a, seed, step0):
    mv = pr.move("eval" if kind == "walk" else kind, S, a=a, sigma=SIGMA, g0=G0)
    ens = open_ens(N, D, [desc(kind, S, a, s=3)], None, seed, step0)

    def check(i, k, nsplits, plan):
        assert (k, nsplits) == (0, S)
        assert_plan(plan, pr.plan(seed, step0 + i, N, mv), mv["kind"], "%s %dx%d step %#x" % (kind, N, D, step0 + i))
    try:
        run_steps(ens, NSTEPS, check)
        assert ens.get_philox() == (seed, step0 + NSTEPS)
    finally:
        ens.close()
    if kind == "de":
        print("philox-reference: DE s0 on the device against the long-double reference: worst error / bound = %.3f" % WORST["de"])


def test_device_plans_of_a_split_key_wider_than_eight_bits():
    N, D, (seed, step0) = 4096, 2, KEYS[1]
    mv = pr.move("stretch", 2, a=2.0)
    ens = open_ens(N, D, [desc("stretch")], None, seed, step0)
    try:
        run_steps(ens, NSTEPS, lambda i, k, S, plan: assert_plan(plan, pr.plan(seed, step0 + i, N, mv), "stretch", "4096x2 step %d" % i))
    finally:
        ens.close()


@pytest.mark.parametrize("seed,step0", KEYS)
def test_gaussian_move_column_and_accept_uniform(seed, step0):
    N, D = 32, 5
    ens = open_ens(N, D, [_lib.MoveDesc(_lib.MOVE_GAUSS, 1, 0, 1, 0.0, 0.25, 0.0, 0.0)], None, seed, step0)          # `random` mode

    def check(i, k, S, plan):
        assert (k, S) == (0, 1)
        ref = pr.gauss_plan(seed, step0 + i, N, D, "random")
        for key in ("off", "order", "p0", "p1", "p2", "s0", "uacc"):
            assert np.array_equal(plan[key], ref[key]), (i, key)
    try:
        run_steps(ens, NSTEPS, check)
    finally:
        ens.close()


def test_gaussian_move_step_size_factor():
    """the 'FACT' word.  The factor is not read back: with the rows materialised, row = (f s) n with n the f32 noise, which
    test_gpu_gauss_noise_reference.py holds within 4096 2^-24 r of gauss_noise_ref's.  Where |n_ref| >= r / 2 that is a relative
    2 x 4096 x 2^-24 = 2^-11 of n, so every such element over (s n_ref) is the reference's f within 2^-11 (a wrong word gives an f
    anywhere in [1 / 1.5, 1.5])."""
    from test_gpu_gaussian_move import read_disp
    N, D, factor, sigma = 32, 5, 1.5, 0.25
    seed, step0 = KEYS[1]
    ens = open_ens(N, D, [_lib.MoveDesc(_lib.MOVE_GAUSS, 1, 0, 0, 1.0, sigma, float(np.log(factor)), 0.0)], None, seed, step0)
    try:
        ens.set_tuning("gauss_materialize", 1)
        fs = []
        for i in range(4):
            ens.step_begin(False)
            disp = read_disp(ens)
            ens.halfstep(0)
            ens.step_end()
            assert ens.status() == 0
            n, r = gr.noise(seed, step0 + i, N, D)
            sel = (np.abs(n) >= 0.5 * r) & (r > 0)
            assert sel.sum() > N
            f = pr.factor(seed, step0 + i, np.log(factor))
            assert 1.0 / factor <= f <= factor
            assert np.all(np.abs(disp[sel] / (sigma * n[sel]) / f - 1.0) <= 2.0 ** -11), (i, f)
            fs.append(f)
        assert len(set(fs)) == 4
    finally:
        ens.close()


# ---- the move choice --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,step0", KEYS)
def test_move_choice_of_a_three_move_mixture(seed, step0):
    N, D, weights = 32, 3, [0.5, 0.3, 0.2]
    kinds = [("stretch", 2), ("de", 2), ("snooker", 4)]
    ens = open_ens(N, D, [desc(k, S) for k, S in kinds], weights, seed, step0)
    cdf = cdf_of(weights, 3)
    seen = set()

    def check(i, k, S, plan):
        assert k == pr.move_choice(seed, step0 + i, cdf), i
        assert S == kinds[k][1]
        assert_plan(plan, pr.plan(seed, step0 + i, N, pr.move(kinds[k][0], S, sigma=SIGMA, g0=G0)), kinds[k][0], "mixture step %d" % i)
        seen.add(k)
    try:
        run_steps(ens, 40, check)
    finally:
        ens.close()
    assert seen == {0, 1, 2}


# ---- tempering --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,N", [(3, 20), (5, 64)])
def test_swap_pass_draws_equal_the_definition(T, N):
    """emx_host_pt_swap_draws against the definition (pairings bit for bit, the stored logarithm within one ulp of the long-double
    one), then one swap pass on a planted state against test_gpu_pt.py's oracle, unchanged and fed by the library's logu -- so a
    tie cannot flip a decision: state, L, P and counts identical."""
    pytest.importorskip("torch")
    from emcee_amd import PTSampler
    from emcee_amd.targets import BatchCallable
    from test_gpu_pt import draws, gauss_fn, group_seeds, pt_view, start, swap_oracle
    G, D = 2, 2
    rs = np.random.RandomState(T * 100 + N)
    lo, hi = -3.0 * np.ones(D), 3.0 * np.ones(D)
    betas = np.concatenate([np.geomspace(1.0, 0.05, T - 1), [0.0]])
    fn = gauss_fn(np.zeros((G * T, D)), np.ones((G * T, D)))
    s = PTSampler(T, N, D, BatchCallable(pt_view(fn, G, T)), log_prior=(lo, hi), betas=betas, nbatch=G, seeds=[11, 12], swap_every=0)
    s.run_mcmc(start(rs, G, T, N, D), 1, skip_initial_state_check=True)
    X = rs.uniform(-4, 4, size=(G, T, N, D))
    P = np.where(((X >= lo) & (X <= hi)).all(-1), 0.0, -np.inf)
    L = np.where(P == 0, -0.5 * (X * X).sum(-1) + rs.randn(G, T, N), -np.inf)
    s._set_pt_state(X.reshape(G * T, N, D), L.reshape(G * T, N), P.reshape(G * T, N))
    before = s._swap_counts()
    s._swap()
    step = s._b._step - 1
    seeds = group_seeds(s)
    assert seeds == [pr.philox_seed_of(int(s.member_seeds[g, 0])) for g in range(G)]
    for g in range(G):
        perm, logu = draws(seeds[g], step, N, T)
        rperm, u = pr.swap_draws(seeds[g], step, N, T)
        assert np.array_equal(perm, rperm)
        assert np.array_equal(logu[u == 0], np.full((u == 0).sum(), -np.inf))
        want = np.log(u[u > 0].astype(pr.LD)).astype(np.float64)
        assert np.all(np.abs(logu[u > 0].view(np.int64) - want.view(np.int64)) <= 1)
    wX, wL, wP, wlp, wacc = swap_oracle(X, L, P, betas, seeds, step)
    got = s.get_last_sample()
    gL, gP = s._pt_state()
    assert np.array_equal(got.coords, wX) and np.array_equal(gL, wL) and np.array_equal(gP, wP)
    assert np.array_equal(got.log_prob, wlp)
    att, acc = s._swap_counts()
    assert np.array_equal(att - before[0], np.full((G, T - 1), N, dtype=np.uint64))
    assert np.array_equal(acc - before[1], wacc) and wacc.sum() > 0
