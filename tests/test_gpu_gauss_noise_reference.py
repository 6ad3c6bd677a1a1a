"""Every path that makes the native Gaussian move's noise (gauss_disp_row / native_gauss_pair, emx_kernels.hpp) against the NumPy
reference of tests/gauss_noise_ref.py, which shares nothing with the device code (tests/test_gauss_noise_ref_cpu.py checks the
reference itself and that the gate below rejects every plausible kernel mistake).

Observation.  The target is flat -- DiagGaussian(0, 2^-200), DenseGaussian(0, 2^-200 I) or a callback that returns zeros -- so
every proposal is accepted whatever the accept uniform, and the walkers start at 0: the first stored row IS the displacement
(f scale_d) n, without the rounding of an addition, and later ones are differences of consecutive rows, up to
2^-52 (|x_t| + |x_t-1|), which is added to the bound.  A row equal to its predecessor counts as rejected and is skipped: at most
1 % of the rows of a flat-target case may be (the expected share is 0).  The Philox step of the first proposal has both of its
halves non-zero wherever the API lets a test set it, so that swapped halves show.

The bound.  |d - d_ref| <= |f s_d| K 2^-24 r + 2^-52 |d_ref| with d_ref = (f s_d) n_ref from radius r, K = 4096 fixed in advance
(twelve of f32's 24 bits kept; every mistake of indexing or mapping moves a coordinate by the order of r, 2^12 times the gate; an
honest f32 Box-Muller cannot lose 12 bits).  Every test prints its worst error in units of |f s_d| 2^-24 r.

K_MEAS, below, is the second, tighter constant: 8 times the worst such ratio measured on an MI355X over every case of this file
(profiles/gauss_noise_reference.md)."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import emcee_amd
from emcee_amd import _lib, moves, targets
from oracle import sampler_oracle as so

import gauss_noise_ref as gr
from test_gpu_gaussian_move import read_disp
from test_gpu_parity import make_ens

pytestmark = pytest.mark.gpu

K = gr.K_GATE
assert K == 4096.0
# The second constant: 8 x the worst error / (|f s_d| 2^-24 r) measured over every case of this file on an MI355X, 3.741 (k_persist_gauss
# 1024 x 64, 40 steps; profiles/gauss_noise_reference.md has every path's).  The cases see about 10^7 of the 2^56 input pairs and the
# error is a deterministic function of the inputs: hence a factor, not equality.
K_MEAS_WORST = 3.741
K_MEAS = 8.0 * K_MEAS_WORST

STEP0 = (3 << 32) | 0x80000005          # first Philox step of the runs: both halves non-zero and different
FLAT = 2.0 ** -200
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def report(path, worst, skipped=0, rows=0):
    print("gauss-noise-reference: %-44s worst error / (|f s| 2^-24 r) %.4g   rows skipped %d of %d" % (path, worst, skipped, rows))


def assert_gate(rt, path):
    worst = float(np.max(rt)) if rt.size else 0.0
    assert worst <= K, "%s: displacement off by %.4g units of |f s| 2^-24 r (gate %g), %d elements over" % (path, worst, K, int((rt > K).sum()))
    assert worst <= K_MEAS, "%s: %.4g units, above K_MEAS = %.4g" % (path, worst, K_MEAS)
    return worst


def assert_exact_f32(row, scale, path):
    """a first row from x = 0 with f = 1 and power-of-two scales: (scale n) / scale is the f32 the kernel computed"""
    q = row / gr.scale_row(scale, row.shape[-1])
    assert np.array_equal(q, q.astype(np.float32).astype(np.float64)), path + ": the first row is not scale x an f32"


def check_chain(chain, seed, step0, scale, path, thin_by=1, cap=0.01):
    """chain (T, N, D) from x = 0, vector mode, f = 1: every stored row minus its predecessor against the reference's
    displacements of the thin_by steps between them.  -> worst ratio"""
    T, N, D = chain.shape
    prev = np.zeros((N, D))
    worst, skipped = 0.0, 0
    for t in range(T):
        dref, den, mag = np.zeros((N, D)), np.zeros((N, D)), np.zeros((N, D))
        for j in range(thin_by):
            d, r = gr.displacement(seed, step0 + t * thin_by + j, N, D, scale)
            dref += d
            den += gr.unit(scale, D, r)
            mag += np.abs(d)
        moved = np.any(chain[t] != prev, axis=1)
        skipped += int(N - moved.sum())
        if t == 0 and thin_by == 1:
            extra = 0.0
            assert_exact_f32(chain[0][moved], scale, path)
        else:
            extra = 2.0 ** -52 * (np.abs(chain[t]) + np.abs(prev) + (mag if thin_by > 1 else 0.0))
        rt = gr.ratio_units(chain[t] - prev, dref, den, extra)[moved]
        worst = max(worst, assert_gate(rt, "%s, stored step %d" % (path, t)))
        prev = chain[t]
    report(path, worst, skipped, T * N)
    assert skipped <= cap * T * N, "%s: %d of %d rows did not move" % (path, skipped, T * N)
    return worst


def pow2_scales(D):
    return 2.0 ** -(np.arange(D) % 9).astype(np.float64)


# ---- k_gauss_disp: the materialised rows ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D", [(33, 7), (32, 34), (40, 1)])
@pytest.mark.parametrize("mode", ["vector", "random", "sequential"])
@pytest.mark.parametrize("diag", [False, True])
@pytest.mark.parametrize("factor", [None, 1.5])
def test_materialised_rows(N, D, mode, diag, factor):
    scale = 2.0 ** -np.arange(D).astype(np.float64) if diag else 0.25           # distinct for every d
    seed = 0x1234567 << 32 | 0x89abcdef
    mv = so.MoveSpec("gaussian", cov=scale ** 2, mode=mode, factor=factor)
    spec = dict(N=N, D=D, moves=[mv], weights=None, desc={"kind": "iso"})
    ens = make_ens(spec, np.zeros((N, D)))
    path = "k_gauss_disp %dx%d %s%s%s" % (N, D, mode, " diag" if diag else "", " factor" if factor else "")
    worst = 0.0
    try:
        ens.set_rng_mode(_lib.RNG_PHILOX)
        ens.set_philox(seed, STEP0)
        ens.set_tuning("gauss_materialize", 1)
        for t in range(5):
            ens.step_begin(False)
            col = ens.plan_get(1)["p0"].copy()
            disp = read_disp(ens)
            ens.halfstep(0)
            ens.step_end()
            assert ens.status() == 0
            n, r = gr.noise(seed, STEP0 + t, N, D)
            if mode == "vector":
                assert np.all(col == -1)
                sel = np.ones((N, D), dtype=bool)
            else:
                assert np.all((col >= 0) & (col < D)) and (mode == "random" or np.all(col == t % D))
                sel = np.arange(D)[None, :] == col[:, None]          # only that coordinate of a row is written
            f = 1.0
            if factor is not None:
                with np.errstate(divide="ignore", invalid="ignore"):
                    q = disp / (gr.scale_row(scale, D) * n)
                f = float(np.median(q[sel & (n != 0)]))
                assert 1.0 / factor <= f <= factor, f
            else:
                assert_exact_f32(np.where(sel, disp, 0.0), scale, path)
            dref = (np.float64(f) * gr.scale_row(scale, D)) * n
            # (with a factor, f is the median of ratios that each carry the f32 error of their normal: the estimate's own error,
            # of the order of 2^-24, is part of what is measured here; the elements must agree with ONE f)
            rt = gr.ratio_units(disp, dref, gr.unit(scale, D, r, f))[sel]
            worst = max(worst, assert_gate(rt, "%s, step %d" % (path, t)))
        assert ens.get_philox() == (seed, STEP0 + 5)
    finally:
        ens.close()
    report(path, worst)


# ---- k_halfstep: rows made in registers ----------------------------------------------------------------------------------------
# (target, ndim): the (G, V, CH) of pick_shape (emx_small_host.hpp) and the branch of gauss_disp_row it takes.  Element-wise target:
# cols = ceil(ndim / V); dense: cols = Dp / V with Dp the ndim padded to 16.
HALFSTEP = [
    # diag, even ndim: V = 2
    ("diag", 2),       # G 4, V 2, CH 1    V2, odd CH
    ("diag", 8),       # G 4, V 2, CH 1
    ("diag", 16),      # G 8, V 2, CH 1
    ("diag", 18),      # G 8, V 2, CH 2    DPP exchange
    ("diag", 22),      # G 8, V 2, CH 2    DPP
    ("diag", 30),      # G 8, V 2, CH 2    DPP
    ("diag", 32),      # G 8, V 2, CH 2    DPP, full row
    ("diag", 34),      # G 8, V 2, CH 4    DPP
    ("diag", 66),      # G 16, V 2, CH 4   DPP
    ("diag", 130),     # G 32, V 2, CH 4   DPP
    ("diag", 258),     # G 64, V 2, CH 4   DPP
    ("diag", 514),     # G 64, V 2, CH 8   DPP
    ("diag", 1026),    # G 64, V 2, CH 16  DPP
    # diag, odd ndim: V = 1
    ("diag", 1),       # G 4, V 1, CH 1
    ("diag", 3),       # G 4, V 1, CH 1
    ("diag", 5),       # G 8, V 1, CH 1
    ("diag", 17),      # G 8, V 1, CH 4
    ("diag", 33),      # G 16, V 1, CH 4
    ("diag", 65),      # G 32, V 1, CH 4
    ("diag", 129),     # G 64, V 1, CH 4
    ("diag", 257),     # G 64, V 1, CH 8
    ("diag", 1023),    # G 64, V 1, CH 16
    # dense
    ("dense", 6),      # Dp 16: G 8, V 2, CH 1
    ("dense", 16),     # Dp 16: G 8, V 2, CH 1
    ("dense", 18),     # Dp 32: G 8, V 2, CH 2    DPP
    ("dense", 32),     # Dp 32: G 8, V 2, CH 2    DPP
    ("dense", 34),     # Dp 48: G 8, V 2, CH 4    DPP
    ("dense", 64),     # Dp 64: G 8, V 2, CH 4    DPP
    ("dense", 100),    # Dp 112: G 16, V 2, CH 4  DPP
    ("dense", 128),    # Dp 128: G 16, V 2, CH 4  DPP
    ("dense", 15),     # Dp 16: G 8, V 1, CH 2
    ("dense", 33),     # Dp 48: G 16, V 1, CH 4
    ("dense", 127),    # Dp 128: G 32, V 1, CH 4
    ("dense", 130),    # beyond padded ndim 128: the wide path (proposal kernel + emx_wide.hip)
]


def flat_target(kind, D):
    if kind == "diag":
        return targets.DiagGaussian(np.zeros(D), np.full(D, FLAT))
    return targets.DenseGaussian(np.zeros(D), FLAT * np.eye(D))


def run_sampler(kind, N, D, scale, tune, calls, seed=2024, mode="vector", target=None):
    """-> (the sampler after its runs from x = 0, its Philox seed, persist_info, small_info)"""
    cov = np.asarray(scale, dtype=np.float64) ** 2
    s = emcee_amd.EnsembleSampler(N, D, flat_target(kind, D) if target is None else target,
                                  moves=moves.GaussianMove(cov if cov.size > 1 else float(cov.reshape(-1)[0]), mode=mode), rng="philox")
    s.random_state = np.random.RandomState(seed).get_state()
    s._philox_step = STEP0
    ens = s._device_ensemble()
    for k, v in tune.items():
        ens.set_tuning(k, v)
    state = np.zeros((N, D))
    for nsteps, kw in calls:
        state = s.run_mcmc(state, nsteps, skip_initial_state_check=True, **kw)
    pseed = s._philox_seed()
    assert pseed == gr.philox_seed_of(seed)
    assert ens.get_philox()[0] == pseed
    return s, pseed, ens.persist_info(), ens.small_info()


@pytest.mark.parametrize("kind,D", HALFSTEP)
def test_rows_made_in_registers_by_the_half_step_kernel(kind, D):
    N, T = 32, 3
    scale = pow2_scales(D) if D % 3 else 0.5                # per-coordinate scales at most shapes, the scalar at some of each branch
    s, seed, info, small = run_sampler(kind, N, D, scale, {"small_kernel": 0, "persist": 0}, [(T, {})])
    assert small["launches"] == 0 and info["launches"] == 0, (small, info)
    assert s._philox_step == STEP0 + T
    check_chain(s.get_chain(), seed, STEP0, scale, "k_halfstep %s %dx%d" % (kind, N, D))


@pytest.mark.parametrize("kind,D", [("diag", 34), ("diag", 7), ("dense", 18)])
def test_one_coordinate_branch_of_the_half_step_kernel(kind, D):
    """sequential mode: step t moves coordinate t % ndim of every walker by that coordinate's normal, the others not at all"""
    N, T = 32, D + 2
    scale = pow2_scales(D)
    s, seed, info, small = run_sampler(kind, N, D, scale, {"small_kernel": 0, "persist": 0}, [(T, {})], mode="sequential")
    assert small["launches"] == 0 and info["launches"] == 0, (small, info)
    chain, prev, worst = s.get_chain(), np.zeros((N, D)), 0.0
    for t in range(T):
        dref, r = gr.displacement(seed, STEP0 + t, N, D, scale, col=np.full(N, t % D))
        extra = 2.0 ** -52 * (np.abs(chain[t]) + np.abs(prev))
        worst = max(worst, assert_gate(gr.ratio(chain[t] - prev, dref, r, scale, extra=extra), "k_halfstep sequential, step %d" % t))
        other = np.arange(D) != t % D
        assert np.array_equal(chain[t][:, other], prev[:, other])
        prev = chain[t]
    report("k_halfstep %s %dx%d sequential" % (kind, N, D), worst)


# ---- k_persist_gauss: 16 steps a launch, the walkers in registers --------------------------------------------------------------
@pytest.mark.parametrize("D,calls,thin_by", [(16, (40,), 1), (32, (40,), 1), (64, (40,), 1), (32, (20,), 2), (16, (13, 27), 1)])
def test_persistent_gaussian_kernel(D, calls, thin_by):
    N = 1024
    scale = pow2_scales(D)
    s, seed, info, small = run_sampler("dense", N, D, scale, {}, [(n, dict(thin_by=thin_by)) for n in calls])
    steps = sum(calls) * thin_by
    assert small["launches"] == 0 and info["qualifies"] and info["recovered"] == 0, (small, info)
    assert info["halfsteps"] == steps and info["launches"] >= (steps + 15) // 16, info
    assert s._philox_step == STEP0 + steps
    chain = s.get_chain()
    assert chain.shape == (sum(calls), N, D)
    check_chain(chain, seed, STEP0, scale, "k_persist_gauss %dx%d %s thin %d" % (N, D, "+".join(map(str, calls)), thin_by), thin_by=thin_by)


# ---- k_small_run ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N,D,tune", [("diag", 32, 5, {}), ("dense", 64, 8, {}), ("diag", 32, 34, {"small_kernel": 2})])
def test_one_workgroup_kernel(kind, N, D, tune):
    T = 20
    scale = pow2_scales(D)
    s, seed, info, small = run_sampler(kind, N, D, scale, tune, [(T, {})])
    assert small["launches"] >= 1 and small["steps"] >= T and info["launches"] == 0, (small, info)
    check_chain(s.get_chain(), seed, STEP0, scale, "k_small_run %s %dx%d" % (kind, N, D))


# ---- EnsembleBatch -------------------------------------------------------------------------------------------------------------
def check_members(chain, seeds, scale, path):
    """chain (B, T, N, D), member b under philox_seed(RandomState(seeds[b])), steps from STEP0"""
    worst = 0.0
    for b, sd in enumerate(seeds):
        worst = max(worst, check_chain(chain[b], gr.philox_seed_of(sd), STEP0, scale, "%s, member %d" % (path, b)))
    return worst


@pytest.mark.parametrize("N,D", [(32, 4), (32, 18)])
def test_ensemble_batch_builtin_target(N, D):
    B, T, seeds = 3, 20, [11, 12, 13]
    scale = pow2_scales(D)
    b = emcee_amd.EnsembleBatch(B, N, D, targets.DiagGaussian(np.zeros(D), np.full(D, FLAT)), moves=moves.GaussianMove(scale ** 2), seeds=seeds)
    b._step = STEP0                 # the batch's common step counter: the first proposal's step
    try:
        b.run_mcmc(np.zeros((B, N, D)), T, skip_initial_state_check=True)
        assert b._step == STEP0 + T
        assert b.launch_info()["launches"] >= 1
        assert [int(x) for x in b._philox] == [gr.philox_seed_of(sd) for sd in seeds]
        chain = b.get_chain()
    finally:
        b.close()
    assert chain.shape == (B, T, N, D)
    check_members(chain, seeds, scale, "EnsembleBatch %dx%dx%d" % (B, N, D))


def test_ensemble_batch_callback_target():
    import torch
    B, N, D, T, seeds = 3, 32, 4, 12, [21, 22, 23]
    calls = []

    def zeros(q):
        calls.append(tuple(q.shape))
        return torch.zeros(q.shape[:-1], dtype=torch.float64, device=q.device)
    b = emcee_amd.EnsembleBatch(B, N, D, targets.BatchCallable(zeros), moves=moves.GaussianMove(0.25), seeds=seeds)
    b._step = STEP0                 # the batch's common step counter: the first proposal's step
    try:
        b.run_mcmc(np.zeros((B, N, D)), T, skip_initial_state_check=True)
        assert b._step == STEP0 + T
        chain = b.get_chain()
    finally:
        b.close()
    assert len(calls) >= T and all(c[0] == B and c[-1] == D for c in calls)
    check_members(chain, seeds, 0.5, "EnsembleBatch callback %dx%dx%d" % (B, N, D))


# ---- PTSampler -----------------------------------------------------------------------------------------------------------------
def pt_seeds(seeds, T):
    """PTSampler's rule (pt.py): chain (g, t) is the batch member seeded with RandomState(seeds[g]).randint(0, 2^32, T, uint64)[t]"""
    return [[int(v) for v in np.random.RandomState(sd).randint(0, 2 ** 32, size=T, dtype=np.uint64)] for sd in seeds]


def test_pt_sampler_callback_likelihood():
    import torch
    G, T, N, D, nsteps, seeds = 2, 3, 32, 4, 12, [5, 6]

    def zeros(q):
        return torch.zeros(q.shape[:-1], dtype=torch.float64, device=q.device)
    pt = emcee_amd.PTSampler(T, N, D, targets.BatchCallable(zeros), nbatch=G, moves=moves.GaussianMove(0.25), seeds=seeds, swap_every=0)
    pt._b._step = STEP0
    try:
        pt.run_mcmc(np.zeros((G, T, N, D)), nsteps, skip_initial_state_check=True)
        assert pt._b._step == STEP0 + nsteps
        chain = pt.get_chain()
        member_seeds = [int(x) for x in pt._b._philox]
    finally:
        pt.close()
    _check_pt_chain(chain, member_seeds, seeds, G, T, 0.5, "PTSampler callback %dx%dx%dx%d" % (G, T, N, D))


def _check_pt_chain(chain, member_seeds, seeds, G, T, scale, path):
    rule = pt_seeds(seeds, T)
    for g in range(G):
        for t in range(T):
            pseed = gr.philox_seed_of(rule[g][t])
            assert member_seeds[g * T + t] == pseed, "the per-rung seed rule of pt.py"
            check_chain(chain[g, t], pseed, STEP0, scale, "%s, object %d rung %d" % (path, g, t))


def _pt_fused_lib(ndim):
    """tests/c/user_pt_fused.hip at `ndim`, cached under build/ by the hash of the source and of every header it includes"""
    import test_gpu_pt_fused as tp
    from emcee_amd import _build
    src = os.path.join(ROOT, "tests", "c", "user_pt_fused.hip")
    h = hashlib.sha256(open(src, "rb").read() + str(ndim).encode())
    for d in _build.DEPS:
        if d.endswith((".hpp", ".h")):
            h.update(open(d, "rb").read())
    work = os.path.join(ROOT, "build", "test_user_pt")
    so_path = os.path.join(work, "libuser_pt_%d_%s.so" % (ndim, h.hexdigest()[:16]))
    if not os.path.exists(so_path):
        os.makedirs(work, exist_ok=True)
        tmp = "%s.%d.tmp" % (so_path, os.getpid())
        subprocess.run(tp._compile_cmd(ndim, tmp), check=True, timeout=900, capture_output=True)
        os.replace(tmp, so_path)
    return tp._load(so_path)


def test_pt_sampler_fused_likelihood():
    """likelihood (a) of tests/c/user_pt_fused.hip with mean 0 and inverse variance 2^-200 compiled into k_pt_run"""
    from emcee_amd.targets import PTFused
    G, T, N, D, nsteps, seeds = 2, 3, 32, 4, 12, [7, 8]
    user = _pt_fused_lib(D)
    mu, ivar = np.zeros((G * T, D)), np.full((G * T, D), FLAT)
    h = user.user_setup(mu.ctypes.data, ivar.ctypes.data, G * T, D, -1, 0.0, 3.0)
    assert h
    pt = emcee_amd.PTSampler(T, N, D, PTFused(user.pt_fused_a, D, user=user.user_device_pointer(h)), nbatch=G,
                             moves=moves.GaussianMove(0.25), seeds=seeds, swap_every=0)
    pt._b._step = STEP0
    try:
        pt.run_mcmc(np.zeros((G, T, N, D)), nsteps, skip_initial_state_check=True)
        assert pt._b._step == STEP0 + nsteps
        assert pt.launch_info()["launches"] >= 1
        chain = pt.get_chain()
        member_seeds = [int(x) for x in pt._b._philox]
    finally:
        pt.close()
        user.user_teardown(h)
    _check_pt_chain(chain, member_seeds, seeds, G, T, 0.5, "PTSampler fused %dx%dx%dx%d" % (G, T, N, D))


# ---- DeviceFused ---------------------------------------------------------------------------------------------------------------
def test_device_fused_half_step():
    """the functor of tests/c/user_ensemble_fused.hip (model a, a diagonal Gaussian of unit scale) compiled into the half-step;
    steps of 2^-16 from 0 change its log-prob by about 2^-16, so nearly every proposal is accepted: rejected rows are skipped, at
    most 5 % of them"""
    from test_gpu_ensemble_fused import Model
    N, D, T = 1000, 5, 8
    m = Model(D)
    try:
        s, seed, info, small = run_sampler(None, N, D, 2.0 ** -16, {}, [(T, {})], target=m.fused())
        assert s._ens._target_kind == _lib.TARGET_FUSED_ENSEMBLE and small["launches"] == 0, small
        check_chain(s.get_chain(), seed, STEP0, 2.0 ** -16, "DeviceFused %dx%d" % (N, D), cap=0.05)
    finally:
        m.close()
