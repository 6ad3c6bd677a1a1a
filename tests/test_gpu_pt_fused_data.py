"""PTSampler with a fused tempered likelihood that sums over an object's data (targets.PTFused(..., ndata=); emx_pt_fused_data.hpp;
k_pt_run's DATA form) on the GPU.  The oracle is a path the project already has: the SAME inline base and term wrapped as a plain
one-lane PTFused functor that computes  base + S  in the defined order (64 partials in ascending k, the pairwise tree) -- the
EMX_FUSED_PT_TARGET kernel, itself pinned to the BatchKernel path and through it to NumPy by tests/test_gpu_pt_fused.py.  The data
form must equal it BIT FOR BIT in everything a run leaves behind.  The value itself is pinned by NumPy (targets.fused_data_sum), and
with one rung the run is pinned to EnsembleBatch's data target.  No tolerance anywhere.

One model source: the straight-line fit of tests/test_gpu_batch_fused_data.py, base and term of + - * only.  `user` is an array of
per-OBJECT records; member / ntemps selects the record."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from emcee_amd import EnsembleBatch, PTSampler, _lib, moves, targets  # noqa: E402
from emcee_amd.targets import PTFused, compile_fused, compile_fused_pt  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CACHE = os.path.join(ROOT, "build", "test_pt_fused_data")
NDIMS = (1, 5, 16)
BASE = 0.005                 # base = -BASE * |theta|^2 inside the record's box
PRIOR = 0.02                 # the prior functor: -PRIOR * |theta|^2 inside its own box

SOURCE = r"""
// an object's record: its data (device pointers), the box of base, the threshold above which a term is NaN, the prior functor's box,
// the rungs an object (member / ntemps is the object) and the number of data (the one-lane functor's loop bound)
struct line_rec { const double* x; const double* y; const double* ivar; double box; double nan_above; double pbox; long long ntemps; long long ndata; };
__device__ inline const line_rec* line_of(const void* user, int member) {
    const line_rec* r = (const line_rec*)user;
    return r + member / r->ntemps;
}
__device__ inline double line_base(const double* th, int ndim, const line_rec* r) {
    double acc = 0.0;
    for (int d = 0; d < ndim; ++d) {
        if (th[d] > r->box || th[d] < -r->box) return -__builtin_inf();
        acc = acc + th[d] * th[d];
    }
    return -0.005 * acc;
}
__device__ inline double line_term(const double* th, int ndim, const line_rec* r, long long k) {
    if (th[0] > r->nan_above) return __builtin_nan("");
    double m = th[0];
    if (ndim > 1) m = m + th[1] * r->x[k];
    const double d = r->y[k] - m;
    return -0.5 * (r->ivar[k] * d * d);
}
struct LineData {            // (a) EMX_FUSED_PT_DATA_TARGET and (c) EMX_FUSED_BATCH_DATA_TARGET (ntemps = 1 in the records)
    __device__ double base(const double* x, int ndim, int member, const void* user) const { return line_base(x, ndim, line_of(user, member)); }
    __device__ double term(const double* x, int ndim, int member, long long k, const void* user) const {
        return line_term(x, ndim, line_of(user, member), k);
    }
};
struct LineOneLane {         // (b) EMX_FUSED_PT_TARGET: base + S in the defined order, in one lane; no term where base is -inf or NaN
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const {
        const line_rec* r = line_of(user, member);
        const double b = line_base(x, ndim, r);
        if (b != b || b == -__builtin_inf()) return b;
        double p[64];
        for (int l = 0; l < 64; ++l) p[l] = 0.0;
        for (long long k = 0; k < r->ndata; ++k) p[k & 63] = p[k & 63] + line_term(x, ndim, r, k);
        for (int w = 1; w < 64; w *= 2)
            for (int i = 0; i < 64; i += 2 * w) p[i] = p[i] + p[i + w];
        return b + p[0];
    }
};
struct LinePrior {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const {
        const line_rec* r = line_of(user, member);
        double acc = 0.0;
        for (int d = 0; d < ndim; ++d) {
            if (x[d] > r->pbox || x[d] < -r->pbox) return -__builtin_inf();
            acc = acc + x[d] * x[d];
        }
        return -0.02 * acc;
    }
};
"""
REC_WORDS = 8


@pytest.fixture(scope="module")
def libs():
    """the model compiled once a module for every ndim, every wrapping, side by side (cached under build/ by source and headers)"""
    def one(job):
        kind, D, prior = job
        pf = "LinePrior" if prior else None
        tag = "%d%s" % (D, "p" if prior else "")
        if kind == "data":
            return compile_fused_pt(SOURCE, "LineData", D, prior=pf, name="line_data_" + tag, cache_dir=CACHE, data=True)
        if kind == "lane":
            return compile_fused_pt(SOURCE, "LineOneLane", D, prior=pf, name="line_lane_" + tag, cache_dir=CACHE)
        return compile_fused(SOURCE, "LineData", D, name="line_batch_" + tag, cache_dir=CACHE, data=True)
    jobs = [(k, D, p) for D in NDIMS for k in ("data", "lane") for p in (False, True)] + [("batch", 5, False)]
    with ThreadPoolExecutor(len(jobs)) as ex:
        return dict(zip(jobs, ex.map(one, jobs)))


class Catalogue(object):
    """G objects with ndata[g] points each on the device, and their records.  The noise grows with sqrt(ndata) so that a proposal
    from a start cloud of scale 0.1 changes the log-likelihood by about one whatever the count: a rate of acceptance, not 0 or 1."""

    def __init__(self, libs, D, ndata, seed, ntemps, box=1e300, nan_above=1e300, pbox=3.0, noise=0.75):
        G = len(ndata)
        rs = np.random.RandomState(seed)
        self.libs, self.D, self.G, self.T, self.ndata = libs, D, G, int(ntemps), [int(n) for n in ndata]
        box, nan_above = np.broadcast_to(np.float64(box), (G,)), np.broadcast_to(np.float64(nan_above), (G,))
        self.host, self.dev = [], []
        rec = np.zeros((G, REC_WORDS), dtype=np.int64)
        for g, n in enumerate(self.ndata):
            x = np.linspace(-1.0, 1.0, max(n, 2))[:n]
            sigma = noise * np.sqrt(max(n, 16) / 200.0) * (1.0 + 0.5 * rs.rand(n))
            d = np.ascontiguousarray(np.stack([x, 0.2 + 0.5 * x + sigma * rs.randn(n), 1.0 / (sigma * sigma)]))
            t = torch.from_numpy(np.ascontiguousarray(d if n else np.zeros((3, 1)))).cuda()
            self.host.append(d)
            self.dev.append(t)
            rec[g, :3] = [t.data_ptr() + 8 * k * max(n, 1) for k in range(3)]
            rec[g, 3:6] = np.array([box[g], nan_above[g], pbox]).view(np.int64)
            rec[g, 6:] = [self.T, n]
        self.box, self.pbox = box, pbox
        self.rec = torch.from_numpy(rec).cuda()

    def data(self, prior=False, ndata=None):
        """(a) the data form"""
        return self.libs[("data", self.D, prior)].target(user=self.rec, ndata=self.ndata if ndata is None else ndata)

    def lane(self, prior=False):
        """(b) the oracle: the plain one-lane functor"""
        return self.libs[("lane", self.D, prior)].target(user=self.rec)

    def batch(self):
        """(c) EnsembleBatch's data target (records with ntemps = 1)"""
        assert self.T == 1
        return self.libs[("batch", self.D, False)].target(user=self.rec, ndata=self.ndata)

    def log_like(self, g, theta):
        """NumPy's transcription of the model on one row: base + fused_data_sum(terms), in the model's operation order"""
        if (np.abs(theta) > self.box[g]).any():
            return -np.inf
        acc = 0.0
        for d in range(self.D):
            acc = acc + theta[d] * theta[d]
        x, y, ivar = self.host[g]
        m = np.full(x.shape, theta[0])
        if self.D > 1:
            m = m + theta[1] * x
        d = y - m
        return -BASE * acc + targets.fused_data_sum(-0.5 * (ivar * d * d))


def outputs(pt, stored=True):
    """tests/test_gpu_pt_fused.py's dictionary: everything a run leaves behind"""
    last = pt.get_last_sample()
    L, P = pt._pt_state()
    att, acc = pt._swap_counts()
    out = dict(coords=last.coords, last_log_prob=last.log_prob, L=L, P=P, ladder=pt.ladder, updates=np.array(pt.adaptation_updates),
               accepted=pt._b._accepted().reshape(L.shape), attempts=att, swaps=acc, step=np.array(pt._b._step))
    if stored:
        out.update(chain=pt.get_chain(), log_prob=pt.get_log_prob(), log_like=pt.get_log_likelihood(), betas=pt.get_betas())
    return out


def assert_equal_runs(x, y):
    assert sorted(x) == sorted(y)
    for k in x:
        assert x[k].shape == y[k].shape and np.array_equal(x[k], y[k]), k


def assert_not_vacuous(oracle, what, swaps):
    """conditions on the ORACLE run: every (object, rung) accepts some proposals and rejects some; with swap passes, some swaps are
    accepted and some rejected overall"""
    f = oracle.acceptance_fraction.mean(axis=-1)
    att, acc = oracle._swap_counts()
    print("%s: acceptance by (object, rung) %s; swaps %d of %d" % (what, np.round(f, 3).tolist(), int(acc.sum()), int(att.sum())))
    assert (f > 0).all() and (f < 1).all(), f
    if swaps:
        assert 0 < acc.sum() < att.sum(), (acc, att)


LIVE = dict(live_dangerously=True)       # 32 walkers at ndim 16 are two a dimension: the comparison is of arithmetic, not of sampling quality
MOVES = {
    "stretch": lambda: moves.StretchMove(**LIVE),
    "de_snooker": lambda: [(moves.DEMove(**LIVE), 0.6), (moves.DESnookerMove(**LIVE), 0.4)],
    "gauss": lambda: moves.GaussianMove(0.01, mode="vector"),
}
# (nbatch, ntemps, nwalkers, ndim) -> the objects' data counts: around the lane stride, one case ragged down to no datum
SHAPES = {(3, 4, 32, 1): [1, 63, 200], (2, 8, 32, 5): [64, 65], (2, 3, 33, 5): [0, 200], (2, 8, 64, 16): [65, 1]}
BOX = 3.0


def counts_of(shape, mv):
    """the symmetric Gaussian move accepts every proposal of a flat likelihood: there the object without data gets one datum"""
    return [max(n, 1) for n in SHAPES[shape]] if mv == "gauss" else SHAPES[shape]


CASES = []
for i, shape in enumerate(sorted(SHAPES)):
    for j, mv in enumerate(sorted(MOVES)):
        for every in (0, 1, 3):
            k = i + j + every
            CASES.append((shape, mv, every, (1, 3)[k % 2], ("box", "functor", "none")[k % 3]))


def pair(libs, shape, mv, prior, seed, ndata=None, cat=None, **kw):
    """-> (data-form sampler, one-lane sampler, catalogue) of one configuration"""
    G, T, N, D = shape
    cat = cat or Catalogue(libs, D, counts_of(shape, mv) if ndata is None else ndata, seed + 1, T)
    common = dict(nbatch=G, seeds=[seed + 10 * g for g in range(G)], log_prior=(-BOX * np.ones(D), BOX * np.ones(D)) if prior == "box" else None)
    common.update(kw)
    mk = (lambda: MOVES[mv]()) if isinstance(mv, str) else mv
    f = PTSampler(T, N, D, cat.data(prior == "functor"), **dict(common, moves=mk()))
    k = PTSampler(T, N, D, cat.lane(prior == "functor"), **dict(common, moves=mk()))
    return f, k, cat


def start(seed, shape, scale=0.1):
    return scale * np.random.RandomState(seed).randn(*shape)


def close(*things):
    for s in things:
        s.close()


# ---------------------------------------------------------------------------------------------------------------- 1. bit equality
@pytest.mark.parametrize("shape,mv,every,thin_by,prior", CASES, ids=["%s-%s-swap%d-thin%d-%s" % ("x".join(map(str, c[0])), c[1], c[2], c[3], c[4])
                                                                      for c in CASES])
def test_the_data_form_equals_the_one_lane_functor(libs, shape, mv, every, thin_by, prior):
    G, T, N, D = shape
    seed = 100 * G + 7 * T + N + D + every + thin_by
    f, k, cat = pair(libs, shape, mv, prior, seed, swap_every=every)
    p0 = start(seed, shape)
    nsteps = 16
    f.run_mcmc(p0, nsteps, thin_by=thin_by, skip_initial_state_check=True)
    k.run_mcmc(p0, nsteps, thin_by=thin_by, skip_initial_state_check=True)
    x, y = outputs(f), outputs(k)
    assert x["chain"].shape == (G, T, nsteps, N, D) and x["step"] == nsteps * thin_by
    assert_not_vacuous(k, "%s %s swap %d thin %d %s" % (shape, mv, every, thin_by, prior), every > 0)
    assert_equal_runs(x, y)
    assert np.array_equal(f.acceptance_fraction, k.acceptance_fraction)
    assert f.launch_info()["threads"] == 512           # a wave a row: every shape here stages more rows than a workgroup has waves
    close(f, k)


# ---------------------------------------------------------------------------------------------------------------- 2. the value
def test_the_final_log_likelihoods_equal_a_numpy_transcription(libs):
    shape = G, T, N, D = 2, 3, 33, 5
    cat = Catalogue(libs, D, [65, 200], 3, T)
    pt = PTSampler(T, N, D, cat.data(), nbatch=G, seeds=[4, 5], moves=MOVES["stretch"]())
    pt.run_mcmc(start(6, shape), 12, skip_initial_state_check=True)
    chain, L = pt.get_chain(), pt.get_log_likelihood()
    for step in (0, -1):
        want = np.array([[[cat.log_like(g, chain[g, t, step, i]) for i in range(N)] for t in range(T)] for g in range(G)])
        assert np.isfinite(want).all() and np.array_equal(L[:, :, step], want)
    assert np.array_equal(pt._pt_state()[0], L[:, :, -1])
    pt.close()


@pytest.mark.parametrize("ndata", [[0, 1, 63], [64, 65, 200]])
def test_the_initial_state_equals_a_numpy_transcription_at_every_count(libs, ndata):
    """the eval0 pass: base's box cuts the cloud (L = -inf without a term evaluated), the handle's box prior cuts it elsewhere"""
    shape = G, T, N, D = 3, 4, 32, 5
    cat = Catalogue(libs, D, ndata, 11, T, box=0.15)
    lo, hi = -0.2 * np.ones(D), 0.2 * np.ones(D)
    pt = PTSampler(T, N, D, cat.data(), log_prior=(lo, hi), nbatch=G, seeds=[1, 2, 3])
    p0 = start(12, shape)
    pt.run_mcmc(p0, 0, skip_initial_state_check=True)
    L, P = pt._pt_state()
    inside = (np.abs(p0) <= 0.2).all(axis=-1)
    assert np.array_equal(P, np.where(inside, 0.0, -np.inf)) and (~inside).any()
    want = np.array([[[cat.log_like(g, p0[g, t, i]) if inside[g, t, i] else -np.inf for i in range(N)] for t in range(T)] for g in range(G)])
    assert np.isneginf(want[inside]).any() and np.isfinite(want).sum() > want.size // 4
    assert np.array_equal(L, want)
    assert pt.launch_info()["launches"] == 1
    pt.close()


# ---------------------------------------------------------------------------------------------------------------- 3. the batch
def test_with_one_rung_and_no_swaps_the_run_is_the_batch_of_the_same_model(libs):
    G, T, N, D, nsteps = 3, 1, 32, 5, 16
    cat = Catalogue(libs, D, [0, 65, 200], 21, T)
    for mv in ("stretch", "de_snooker"):
        pt = PTSampler(T, N, D, cat.data(), betas=np.array([1.0]), nbatch=G, seeds=[7, 8, 9], swap_every=0, moves=MOVES[mv]())
        p0 = start(22, (G, T, N, D))
        pt.run_mcmc(p0, nsteps, skip_initial_state_check=True)
        eb = EnsembleBatch(G, N, D, cat.batch(), moves=MOVES[mv](), seeds=pt.member_seeds.reshape(-1))
        eb.run_mcmc(p0.reshape(G, N, D), nsteps, skip_initial_state_check=True)
        assert np.array_equal(pt.get_chain().reshape(G, nsteps, N, D), eb.get_chain())
        assert np.array_equal(pt.get_log_prob().reshape(G, nsteps, N), eb.get_log_prob())
        assert np.array_equal(pt.acceptance_fraction.reshape(G, N), eb.acceptance_fraction)
        f = eb.acceptance_fraction.mean(axis=-1)
        assert (f > 0).all() and (f < 1).all(), f
        close(pt, eb)


# ---------------------------------------------------------------------------------------------------------------- 4. launch shape
def test_launch_shape_changes_no_bit(libs):
    shape = G, T, N, D = 2, 3, 33, 5

    def run(tuning):
        f, k, cat = pair(libs, shape, "de_snooker", "box", 32, swap_every=1)
        for key, v in tuning.items():
            f.set_tuning(key, v)
        f.run_mcmc(start(31, shape), 12, skip_initial_state_check=True)
        out, info = outputs(f), f.launch_info()
        close(f, k)
        return out, info
    ref, info0 = run({})
    assert info0["threads"] == 512                     # 3 x 17 rows: more than the 8 waves, and no multiple of them
    for threads in (64, 192, 512):
        for plan_steps in (1, 4):
            out, info = run(dict(batch_threads=threads, batch_plan_steps=plan_steps))
            assert info["threads"] == threads and info["plan_steps"] == plan_steps
            assert_equal_runs(ref, out)


@pytest.mark.parametrize("T,N,threads", [(1, 8, 256), (3, 4, 384), (1, 2, 64), (4, 32, 512)])
def test_the_default_shape_is_a_wave_a_row(libs, T, N, threads):
    """64 x ntemps x the rows of the largest split, at most 512; the one-lane form takes G lanes a row"""
    G, D = 2, 1
    cat = Catalogue(libs, D, [65, 1], 35, T)
    for target, want in ((cat.data(), threads), (cat.lane(), None)):
        pt = PTSampler(T, N, D, target, nbatch=G, seeds=[1, 2], moves=MOVES["stretch"]())
        pt.run_mcmc(start(36, (G, T, N, D)), 3, skip_initial_state_check=True)
        if want is not None:
            assert pt.launch_info()["threads"] == want
            out = outputs(pt)
        else:
            assert pt.launch_info()["threads"] < threads or threads == 64
            assert_equal_runs(out, outputs(pt))
        pt.close()


# ---------------------------------------------------------------------------------------------------------------- 5. composition
def test_a_run_in_three_calls_equals_one_and_unstored_runs_leave_the_same_state(libs):
    shape = G, T, N, D = 3, 4, 32, 1
    p0 = start(41, shape)
    one, k, cat = pair(libs, shape, "de_snooker", "functor", 42, swap_every=3)
    one.run_mcmc(p0, 18, skip_initial_state_check=True)
    k.run_mcmc(p0, 18, skip_initial_state_check=True)
    assert_not_vacuous(k, "composition", True)
    assert_equal_runs(outputs(one), outputs(k))
    three, k2, _ = pair(libs, shape, "de_snooker", "functor", 42, swap_every=3, cat=cat)
    three.run_mcmc(p0, 5, skip_initial_state_check=True)
    three.run_mcmc(None, 6)
    three.run_mcmc(None, 7)
    assert_equal_runs(outputs(one), outputs(three))
    blind, k3, _ = pair(libs, shape, "de_snooker", "functor", 42, swap_every=3, cat=cat)
    blind.run_mcmc(p0, 18, store=False, skip_initial_state_check=True)
    k2.run_mcmc(p0, 18, store=False, skip_initial_state_check=True)
    assert_equal_runs(outputs(blind, stored=False), outputs(k2, stored=False))
    assert np.array_equal(blind.get_last_sample().coords, one.get_last_sample().coords)
    assert np.array_equal(blind._pt_state()[0], one._pt_state()[0])
    close(one, k, three, k2, blind, k3)


# ---------------------------------------------------------------------------------------------------------------- 6. adaptation
def test_adaptive_ladder_then_frozen(libs):
    shape = G, T, N, D = 2, 8, 32, 5
    f, k, cat = pair(libs, shape, "stretch", "box", 51, swap_every=1, adaptive=True, adaptation_lag=20, adaptation_time=2)
    p0 = start(52, shape)
    for s in (f, k):
        s.run_mcmc(p0, 20, skip_initial_state_check=True)
    assert f.adaptation_updates == 20 and not np.array_equal(f.ladder, np.tile(f.betas, (G, 1)))      # the ladder visibly moved
    assert_not_vacuous(k, "adaptive", True)
    assert_equal_runs(outputs(f), outputs(k))
    for s in (f, k):
        s.adaptive = False
        s.run_mcmc(None, 12)
    x, y = outputs(f), outputs(k)
    assert_equal_runs(x, y)
    assert x["updates"] == 20 and np.array_equal(x["betas"][:, 20:], np.broadcast_to(x["ladder"][:, None, :], x["betas"][:, 20:].shape))
    close(f, k)


# ---------------------------------------------------------------------------------------------------------------- 7. NaN
def test_a_nan_term_raises_the_reference_error_naming_object_and_rung(libs):
    G, T, N, D, bad = 3, 4, 32, 5, 1
    shape = (G, T, N, D)
    p0 = start(61, shape, scale=0.05)
    nan_above = np.full(G, 1e300)
    nan_above[bad] = 0.3                              # no walker starts above 0.3; the weakly constrained object's proposals get there
    cat = Catalogue(libs, D, [20] * G, 62, T, nan_above=nan_above, noise=40.0)
    said = []
    for target in (cat.data(), cat.lane()):           # inside the prior (flat): the error is the oracle's, word for word
        pt = PTSampler(T, N, D, target, nbatch=G, seeds=[1, 2, 3])
        with pytest.raises(ValueError) as e:
            pt.run_mcmc(p0, 300, skip_initial_state_check=True)
        said.append(str(e.value))
        pt.close()
    assert said[0] == said[1]
    assert said[0].startswith("(object %d, rung " % bad) and "Probability function returned NaN" in said[0]
    nan_above[bad] = -1e300                           # every row of the object, the initial ones included
    cat = Catalogue(libs, D, [20] * G, 62, T, nan_above=nan_above, noise=40.0)
    pt = PTSampler(T, N, D, cat.data(), nbatch=G, seeds=[1, 2, 3])
    with pytest.raises(ValueError) as e:
        pt.run_mcmc(p0, 10, skip_initial_state_check=True)
    assert str(e.value).startswith("(object %d, rung 0): The initial log_prob was NaN" % bad)
    pt.close()


# ---------------------------------------------------------------------------------------------------------------- 8. the prior's rules
def test_a_walker_outside_the_box_never_reaches_term(libs):
    """every term above the box's upper edge in coordinate 0 is NaN: a row outside the prior that reached the model would raise"""
    shape = G, T, N, D = 2, 8, 32, 5
    hi = 0.12
    cat = Catalogue(libs, D, [65, 200], 71, T, nan_above=hi)
    pt = PTSampler(T, N, D, cat.data(), log_prior=(-hi * np.ones(D), hi * np.ones(D)), nbatch=G, seeds=[1, 2], swap_every=1)
    p0 = start(72, shape)
    assert (p0[..., 0] > hi).sum() > 10 and (np.abs(p0) <= hi).all(axis=-1).sum() > G * T * 4
    pt.run_mcmc(p0, 20, skip_initial_state_check=True)
    L, P = pt.get_log_likelihood(), pt._pt_state()[1]
    assert not np.isnan(L).any() and not np.isnan(pt.get_log_prob()).any()
    assert np.isneginf(pt.get_log_prob()[:, :, 0]).any() and np.isfinite(P).any()      # rows outside were carried, without a NaN
    f = pt.acceptance_fraction.mean(axis=-1)
    assert (f > 0).all() and (f < 1).all()
    pt.close()


def test_a_ladder_down_to_beta_zero_with_walkers_outside_the_box(libs):
    shape = G, T, N, D = 3, 4, 32, 1
    f, k, cat = pair(libs, shape, "stretch", "box", 81, swap_every=1, betas=np.array([1.0, 0.3, 0.05, 0.0]))
    p0 = start(82, shape, scale=2.0)                  # the box is |x| <= 3: some walkers start outside (P = -inf)
    f.run_mcmc(p0, 0, skip_initial_state_check=True)
    assert np.isneginf(f._pt_state()[1]).any()
    f.run_mcmc(None, 20)
    k.run_mcmc(p0, 20, skip_initial_state_check=True)
    assert_not_vacuous(k, "beta = 0", True)
    assert_equal_runs(outputs(f), outputs(k))
    close(f, k)


# ---------------------------------------------------------------------------------------------------------------- 9. launches
def test_one_launch_per_chunk(libs):
    """a chunk is up to 4 096 proposal steps; the runs below stay under it"""
    shape = G, T, N, D = 3, 4, 32, 1
    f, k, cat = pair(libs, shape, "stretch", "box", 91, swap_every=1)
    f.run_mcmc(start(92, shape), 1, store=False, skip_initial_state_check=True)
    for n in (10, 100):
        n0 = f.launch_info()["launches"]
        f.run_mcmc(None, n, store=False)
        assert f.launch_info()["launches"] - n0 == 1
    close(f, k)


# ---------------------------------------------------------------------------------------------------------------- 10. refusals
def test_a_launcher_of_another_header_version_is_refused_at_bind_time(libs, tmp_path):
    G, T, N, D = 2, 4, 32, 5
    wrong = compile_fused_pt(SOURCE, "LineData", D, name="line_wrong", flags=["-DEMX_FUSED_PT_DATA_ABI=4242u"], cache_dir=str(tmp_path), data=True)
    cat = Catalogue(libs, D, [5, 9], 101, T)
    p0 = start(102, (G, T, N, D))
    # another EMX_FUSED_PT_DATA_ABI; the data launcher handed to the plain setter; a plain launcher handed to the data setter
    for target, header in ((wrong.target(user=cat.rec, ndata=cat.ndata), "emx_pt_fused_data.hpp"),
                           (PTFused(libs[("data", D, False)].launcher, D, user=cat.rec), "emx_pt_fused.hpp"),
                           (PTFused(libs[("lane", D, False)].launcher, D, user=cat.rec, ndata=cat.ndata), "emx_pt_fused_data.hpp")):
        pt = PTSampler(T, N, D, target, nbatch=G, seeds=[1, 2])
        with pytest.raises(_lib.EmxError) as e:
            pt.run_mcmc(p0, 10, skip_initial_state_check=True)
        assert "another version of %s" % header in str(e.value) and "(code -8)" in str(e.value)
        assert pt.launch_info()["launches"] == 0
        pt.close()


def test_the_setter_refuses_a_count_out_of_range_naming_the_member(libs):
    G, T, N, D = 2, 4, 32, 5
    cat = Catalogue(libs, D, [5, 9], 111, T)
    pt = PTSampler(T, N, D, cat.data(), nbatch=G, seeds=[1, 2])
    h = pt._b._handle()
    lib = _lib.load()
    fn = C.cast(libs[("data", D, False)].launcher, _lib.PT_FUSED_FN)
    counts = np.repeat(np.array([5, 9], dtype=np.int64), T)
    counts[5] = 2 ** 31
    assert lib.emx_pt_set_target_fused_data(h, fn, D, None, counts) == -1
    assert b"member 5 has 2147483648" in lib.emx_batch_last_error(h)
    counts[5] = -1
    assert lib.emx_pt_set_target_fused_data(h, fn, D, None, counts) == -1 and b"member 5 has -1" in lib.emx_batch_last_error(h)
    pt.close()
