"""EnsembleBatch with a fused user target that sums over per-member data (targets.BatchFused(..., ndata=); emx_fused_target_data.hpp;
k_small_run's DATA form) on the GPU.  The oracle is a kernel the project already has: member b of the batch must equal, BIT FOR BIT,
EnsembleSampler(nwalkers, ndim, DeviceFused(..., ndata=ndata[b]), rng="philox") seeded seeds[b] -- the single sampler's
k_halfstep_user_data, itself pinned to DeviceKernel and to NumPy by tests/test_gpu_ensemble_fused_data.py -- in chain, log-probs,
accept counts and final state.  The value itself is pinned by NumPy (targets.fused_data_sum).  No tolerance anywhere.

One model source: a straight-line fit whose base and term use + - * only.  `user` is an array of per-member records; the batch model
reads rec[member], the single sampler's wrapping of the same inline functions reads rec[0] of a `user` that points at member b's
record."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from emcee_amd import EnsembleBatch, EnsembleSampler, PTSampler, _lib, moves, targets  # noqa: E402
from emcee_amd.targets import compile_fused, compile_fused_ensemble  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CACHE = os.path.join(ROOT, "build", "test_batch_fused_data")
NDIMS = (1, 3, 5, 33)
PRIOR = 0.005                # base = -PRIOR * |theta|^2 inside the box

SOURCE = r"""
// a member's record: its data (device pointers), the box of the prior, and the threshold above which a term is NaN
struct line_rec { const double* x; const double* y; const double* ivar; double box; double nan_above; };
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
struct LineBatch {           // EMX_FUSED_BATCH_DATA_TARGET: rec[member]
    __device__ double base(const double* x, int ndim, int member, const void* user) const { return line_base(x, ndim, (const line_rec*)user + member); }
    __device__ double term(const double* x, int ndim, int member, long long k, const void* user) const {
        return line_term(x, ndim, (const line_rec*)user + member, k);
    }
};
struct LineSingle {          // EMX_FUSED_ENSEMBLE_DATA_TARGET: rec[0] of a user that points at the member's record
    __device__ double base(const double* x, int ndim, const void* user) const { return line_base(x, ndim, (const line_rec*)user); }
    __device__ double term(const double* x, int ndim, long long k, const void* user) const { return line_term(x, ndim, (const line_rec*)user, k); }
};
"""
REC_BYTES = 40


@pytest.fixture(scope="module")
def libs():
    """the model compiled once a session for every ndim, both wrappings, side by side (cached under build/ by source and headers)"""
    def one(job):
        kind, D = job
        if kind == "batch":
            return compile_fused(SOURCE, "LineBatch", D, name="line_batch_%d" % D, cache_dir=CACHE, data=True)
        return compile_fused_ensemble(SOURCE, "LineSingle", D, name="line_single_%d" % D, cache_dir=CACHE, data=True)
    jobs = [(k, D) for D in NDIMS for k in ("batch", "single")]
    with ThreadPoolExecutor(len(jobs)) as ex:
        return dict(zip(jobs, ex.map(one, jobs)))


class Catalogue(object):
    """B objects with ndata[b] points each on the device, and their records.  The noise grows with sqrt(ndata) so that a proposal
    from a start cloud of scale 0.1 changes the log-probability by about one whatever the count: a rate of acceptance, not 0 or 1."""

    def __init__(self, libs, D, ndata, seed, box=1e300, nan_above=1e300, noise=1.5):
        B = len(ndata)
        rs = np.random.RandomState(seed)
        self.libs, self.D, self.B, self.ndata = libs, D, B, [int(n) for n in ndata]
        box, nan_above = np.broadcast_to(np.float64(box), (B,)), np.broadcast_to(np.float64(nan_above), (B,))
        self.host, self.dev = [], []
        rec = np.zeros((B, 5), dtype=np.int64)
        for b, n in enumerate(self.ndata):
            x = np.linspace(-1.0, 1.0, max(n, 2))[:n]
            sigma = noise * np.sqrt(max(n, 16) / 200.0) * (1.0 + 0.5 * rs.rand(n))
            d = np.ascontiguousarray(np.stack([x, 0.2 + 0.5 * x + sigma * rs.randn(n), 1.0 / (sigma * sigma)]))
            t = torch.from_numpy(np.ascontiguousarray(d if n else np.zeros((3, 1)))).cuda()
            self.host.append(d)
            self.dev.append(t)
            rec[b, :3] = [t.data_ptr() + 8 * k * max(n, 1) for k in range(3)]
            rec[b, 3:] = np.array([box[b], nan_above[b]]).view(np.int64)
        self.box = box
        self.rec = torch.from_numpy(rec).cuda()
        assert self.rec.element_size() * 5 == REC_BYTES

    def batch_target(self, ndata=None):
        return self.libs[("batch", self.D)].target(user=self.rec, ndata=self.ndata if ndata is None else ndata)

    def single_target(self, b):
        t = self.libs[("single", self.D)].target(user=self.rec.data_ptr() + REC_BYTES * b, ndata=self.ndata[b])
        t._keep = self                                # the records and the data live as long as the target
        return t

    def log_prob(self, b, theta):
        """NumPy's transcription of the model on one row: base + fused_data_sum(terms), in the model's operation order"""
        if (np.abs(theta) > self.box[b]).any():
            return -np.inf
        acc = 0.0
        for d in range(self.D):
            acc = acc + theta[d] * theta[d]
        x, y, ivar = self.host[b]
        m = np.full(x.shape, theta[0])
        if self.D > 1:
            m = m + theta[1] * x
        d = y - m
        return -PRIOR * acc + targets.fused_data_sum(-0.5 * (ivar * d * d))


def start(rs, B, N, D, scale=0.1):
    return scale * rs.randn(B, N, D)


def run_batch(cat, N, p0, mf, seeds, calls=((12, {}),), tuning=None, ndata=None):
    bt = EnsembleBatch(cat.B, N, cat.D, cat.batch_target(ndata), moves=mf(), seeds=seeds)
    for k, v in (tuning or {}).items():
        bt.set_tuning(k, v)
    st = p0
    for nsteps, kw in calls:
        bt.final = bt.run_mcmc(st, nsteps, skip_initial_state_check=True, **kw)
        st = None
    return bt


def run_single(cat, b, N, p0, mf, seed, calls=((12, {}),)):
    s = EnsembleSampler(N, cat.D, cat.single_target(b), moves=mf(), rng="philox")
    s.random_state = np.random.RandomState(seed).get_state()
    st = p0
    for nsteps, kw in calls:
        s.final = s.run_mcmc(st, nsteps, skip_initial_state_check=True, **kw)
        st = None
    return s


def assert_member_equal(bt, b, s, store=True):
    last, ref = bt.get_last_sample(), s.final
    assert np.array_equal(last.coords[b], ref.coords), "member %d: final coordinates" % b
    assert np.array_equal(last.log_prob[b], ref.log_prob), "member %d: final log-probs" % b
    assert bt._step == s._philox_step, "member %d: Philox step" % b
    if store:
        assert bt.iteration == s.iteration
        assert np.array_equal(bt[b].get_chain(), s.get_chain()), "member %d: chain" % b
        assert np.array_equal(bt[b].get_log_prob(), s.get_log_prob()), "member %d: log-prob chain" % b
        assert np.array_equal(bt[b].acceptance_fraction, s.acceptance_fraction), "member %d: accept counts" % b


def outputs(bt):
    last = bt.get_last_sample()
    out = dict(coords=last.coords, last_log_prob=last.log_prob, step=np.array(bt._step))
    if bt.iteration > 0:
        out.update(chain=bt.get_chain(), log_prob=bt.get_log_prob(), accepted=bt._accepted())
    return out


def assert_equal_runs(x, y):
    assert sorted(x) == sorted(y)
    for k in x:
        assert x[k].shape == y[k].shape and np.array_equal(x[k], y[k]), k


def assert_moves_and_rejects(bt, what):
    """every member's acceptance fraction strictly inside (0.02, 0.98): the equalities are not vacuous"""
    f = np.array([bt[b].acceptance_fraction.mean() for b in range(bt.nbatch)])
    print("acceptance %s: %s" % (what, np.round(f, 3)))
    assert (f > 0.02).all() and (f < 0.98).all(), f


LIVE = dict(live_dangerously=True)       # 8 walkers, or 32 walkers at ndim 33: the comparison is of arithmetic, not of sampling quality
MOVES = {
    "stretch": lambda: moves.StretchMove(**LIVE),
    "de+snooker": lambda: [(moves.DEMove(**LIVE), 0.6), (moves.DESnookerMove(**LIVE), 0.4)],
    "gauss": lambda: moves.GaussianMove(0.002, mode="vector"),
}


def against_the_single_sampler(libs, D, N, ndata, move, calls=((12, {}),), seed=0, store=True):
    cat = Catalogue(libs, D, ndata, seed + 1)
    rs = np.random.RandomState(seed)
    p0 = start(rs, cat.B, N, D)
    seeds = [int(s) for s in rs.randint(1, 2 ** 31, size=cat.B)]
    bt = run_batch(cat, N, p0, MOVES[move], seeds, calls)
    for b in range(cat.B):
        assert_member_equal(bt, b, run_single(cat, b, N, p0[b], MOVES[move], seeds[b], calls), store=store)
    if store:
        assert_moves_and_rejects(bt, "%s %dx%d ndata %s" % (move, N, D, list(ndata)))
    return bt


# ---------------------------------------------------------------------------------------------------------------- 1. bit equality
def test_ragged_counts_around_the_lane_stride(libs):
    """no datum, one, a partial stride, a whole one, one more, several, and 64 whole strides and one, in ONE batch"""
    bt = against_the_single_sampler(libs, 3, 16, [0, 1, 63, 64, 65, 200, 4097], "stretch", seed=1)
    assert bt.launch_info()["launches"] == 2
    bt.close()


def test_a_uniform_int_ndata(libs):
    cat = Catalogue(libs, 3, [130] * 4, 3)
    rs = np.random.RandomState(4)
    p0, seeds = start(rs, 4, 16, 3), [5, 6, 7, 8]
    one = run_batch(cat, 16, p0, MOVES["stretch"], seeds, ndata=130)
    assert one._targets[0].ndata == 130
    for b in range(4):
        assert_member_equal(one, b, run_single(cat, b, 16, p0[b], MOVES["stretch"], seeds[b]))
    assert_equal_runs(outputs(one), outputs(run_batch(cat, 16, p0, MOVES["stretch"], seeds, ndata=[130] * 4)))
    one.close()


@pytest.mark.parametrize("ndim", [1, 5, 33])
@pytest.mark.parametrize("N", [8, 32, 100])
def test_every_row_layout_and_walker_count(libs, ndim, N):
    """odd ndim, G at both ends, and splits of 4, 16 and 50 rows: below, at and above the waves of a workgroup"""
    against_the_single_sampler(libs, ndim, N, [70, 200, 33], "stretch", seed=10 * ndim + N).close()


@pytest.mark.parametrize("move", sorted(MOVES))
@pytest.mark.parametrize("thin_by", [1, 3])
def test_every_schedule_thinned_and_not(libs, move, thin_by):
    against_the_single_sampler(libs, 5, 32, [70, 200, 33], move, calls=((8, dict(thin_by=thin_by)),), seed=20 + thin_by).close()


def test_an_unstored_run(libs):
    against_the_single_sampler(libs, 5, 32, [70, 200, 33], "stretch", calls=((9, dict(store=False)),), seed=30, store=False).close()


def test_a_run_in_two_calls_equals_one(libs):
    cat = Catalogue(libs, 5, [70, 200, 33], 41)
    rs = np.random.RandomState(42)
    p0, seeds = start(rs, 3, 32, 5), [43, 44, 45]
    one = run_batch(cat, 32, p0, MOVES["de+snooker"], seeds, calls=((11, {}),))
    two = run_batch(cat, 32, p0, MOVES["de+snooker"], seeds, calls=((5, {}), (6, {})))
    assert_equal_runs(outputs(one), outputs(two))
    assert_moves_and_rejects(one, "two calls")
    one.close()
    two.close()


# ---------------------------------------------------------------------------------------------------------------- 2. the launch shape
def test_launch_shape_changes_no_bit(libs):
    cat = Catalogue(libs, 5, [70, 200, 33, 64, 1], 51)
    rs = np.random.RandomState(52)
    p0, seeds = start(rs, 5, 100, 5), list(range(60, 65))

    def run(tuning):
        bt = run_batch(cat, 100, p0, MOVES["de+snooker"], seeds, calls=((10, {}),), tuning=tuning)
        out, info = outputs(bt), bt.launch_info()
        bt.close()
        return out, info
    ref, info0 = run({})
    for key, field, values in (("batch_threads", "threads", (64, 256, 1024)), ("batch_plan_steps", "plan_steps", (1,))):
        for v in values:
            out, info = run({key: v})
            assert info[field] == v
            assert_equal_runs(ref, out)
    assert info0["plan_steps"] != 1                   # the default is another shape than the one asked for


def test_members_that_share_cus_get_a_wave_a_row(libs):
    """more members than CUs: the workgroup is cut to a wave a row of the largest split, and the bits are those of one member a CU"""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    B, N, D = ncu + 3, 8, 3
    cat = Catalogue(libs, D, [40 + (7 * b) % 90 for b in range(B)], 55)
    rs = np.random.RandomState(56)
    p0, seeds = start(rs, B, N, D), list(range(100, 100 + B))
    bt = run_batch(cat, N, p0, MOVES["stretch"], seeds, calls=((6, {}),))
    assert bt.launch_info()["threads"] == 64 * 4      # 64 x the 4 rows of a split, where G lanes a row would take one wave
    few = [0, 1, B - 1]
    sub = Catalogue(libs, D, [cat.ndata[b] for b in few], 55)
    sub.host, sub.dev, sub.rec = [cat.host[b] for b in few], cat.dev, cat.rec[few].contiguous()
    small = run_batch(sub, N, p0[few], MOVES["stretch"], [seeds[b] for b in few], calls=((6, {}),))
    assert small.launch_info()["threads"] != 64 * 4
    for i, b in enumerate(few):
        assert np.array_equal(bt[b].get_chain(), small[i].get_chain()) and np.array_equal(bt[b].get_log_prob(), small[i].get_log_prob())
    bt.close()
    small.close()


# ---------------------------------------------------------------------------------------------------------------- 3. NumPy
def test_initial_log_probs_equal_a_numpy_transcription(libs):
    ndata = [0, 1, 63, 64, 65, 200, 4097]
    B, N, D = len(ndata), 16, 5
    cat = Catalogue(libs, D, ndata, 61, box=0.15)     # the box cuts the cloud: some rows are -inf without a term evaluated
    p0 = start(np.random.RandomState(62), B, N, D)
    bt = EnsembleBatch(B, N, D, cat.batch_target(), seeds=list(range(B)))
    st = bt.run_mcmc(p0, 0)
    want = np.array([[cat.log_prob(b, p0[b, i]) for i in range(N)] for b in range(B)])
    assert np.isneginf(want).any() and np.isfinite(want).sum() > B * N // 4
    assert np.array_equal(st.log_prob, want)
    assert np.array_equal(st.coords, p0)
    assert bt.launch_info()["launches"] == 1
    bt.close()


# ---------------------------------------------------------------------------------------------------------------- 4. edges
def test_nan_terms_behind_a_base_of_minus_infinity_run_clean(libs):
    B, N, D = 3, 32, 5
    cat = Catalogue(libs, D, [70, 200, 33], 71, box=0.15, nan_above=0.15)      # a term is NaN only where base is -inf
    p0 = start(np.random.RandomState(72), B, N, D)
    assert (np.abs(p0) > 0.15).any(axis=2).sum() > 5 and (p0[:, :, 0] > 0.15).any() and (np.abs(p0) <= 0.15).all(axis=2).sum() > 5
    bt = EnsembleBatch(B, N, D, cat.batch_target(), seeds=[1, 2, 3])
    st = bt.run_mcmc(p0, 30)
    first = np.array([[cat.log_prob(b, p0[b, i]) for i in range(N)] for b in range(B)])
    assert np.isneginf(first).any() and not np.isnan(bt.get_log_prob()).any() and not np.isnan(st.log_prob).any()
    assert_moves_and_rejects(bt, "NaN behind -inf")
    bt.close()


def test_a_nan_term_raises_the_reference_error_naming_the_member(libs):
    B, N, D, k = 5, 32, 5, 3
    p0 = 0.05 * np.random.RandomState(81).randn(B, N, D)
    nan_above = np.full(B, 1e300)
    nan_above[k] = 0.3                                # no walker starts above 0.3; the weakly constrained member's proposals get there
    cat = Catalogue(libs, D, [20] * B, 82, nan_above=nan_above, noise=40.0)
    bt = EnsembleBatch(B, N, D, cat.batch_target(), seeds=list(range(B)))
    with pytest.raises(ValueError) as e:
        bt.run_mcmc(p0, 300)
    assert str(e.value).startswith("member %d: Probability function returned NaN" % k)
    bt.close()
    nan_above[k] = -1e300                             # every row of member k, the initial ones included
    cat = Catalogue(libs, D, [20] * B, 82, nan_above=nan_above, noise=40.0)
    bt = EnsembleBatch(B, N, D, cat.batch_target(), seeds=list(range(B)))
    with pytest.raises(ValueError) as e:
        bt.run_mcmc(p0, 10)
    assert str(e.value).startswith("member %d: The initial log_prob was NaN" % k)
    bt.close()


def test_a_member_without_data_has_the_log_prob_of_base(libs):
    B, N, D = 3, 16, 3
    cat = Catalogue(libs, D, [0, 50, 0], 91)
    p0 = start(np.random.RandomState(92), B, N, D, scale=3.0)
    bt = EnsembleBatch(B, N, D, cat.batch_target(), seeds=[1, 2, 3])
    bt.run_mcmc(p0, 10)
    chain, lp = bt.get_chain(), bt.get_log_prob()
    base = np.zeros(chain.shape[:-1])
    for d in range(D):
        base = base + chain[..., d] * chain[..., d]
    base = -PRIOR * base + 0.0
    assert np.array_equal(lp[0], base[0]) and np.array_equal(lp[2], base[2])
    assert not np.array_equal(lp[1], base[1])
    bt.close()


# ---------------------------------------------------------------------------------------------------------------- 5. launches
def test_one_launch_per_chunk(libs):
    B, N, D = 4, 8, 3
    cat = Catalogue(libs, D, [5, 9, 0, 70], 101)
    bt = EnsembleBatch(B, N, D, cat.batch_target(), moves=MOVES["stretch"](), seeds=list(range(B)))
    bt.run_mcmc(start(np.random.RandomState(102), B, N, D), 300)
    assert bt.launch_info()["launches"] == 2          # the initial evaluation + one chunk of up to 4 096 steps, as a built-in target
    bt.run_mcmc(None, 4200, store=False)
    assert bt.launch_info()["launches"] == 4          # 4 096 + 104
    bt.close()


# ---------------------------------------------------------------------------------------------------------------- 6. what hangs off the handle
def test_summary_histograms_and_autocorr_on_the_data_handle(libs):
    B, N, D, nsteps = 3, 32, 3, 300
    cat = Catalogue(libs, D, [70, 200, 33], 111)
    p0 = start(np.random.RandomState(112), B, N, D)
    bt = EnsembleBatch(B, N, D, cat.batch_target(), seeds=[1, 2, 3])
    bt.run_mcmc(p0, nsteps)
    chain = bt.get_chain(discard=50)
    s = bt.get_summary(discard=50)
    np.testing.assert_allclose(s.mean, chain.reshape(B, -1, D).mean(axis=1), rtol=1e-10, atol=1e-12)
    tau = bt.get_autocorr_time(discard=50, on_device=True, quiet=True)
    assert tau.shape == (B, D) and np.isfinite(tau).all()
    h = bt.get_histograms(bins=8, discard=50)
    assert h is not None
    bt.close()


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
def test_a_wrong_ndata_length_is_refused_when_the_batch_takes_the_target(libs):
    cat = Catalogue(libs, 3, [5, 9, 7], 121)
    with pytest.raises(ValueError) as e:
        EnsembleBatch(4, 16, 3, cat.batch_target())
    assert "nbatch = 4" in str(e.value) and "got 3" in str(e.value)


def test_a_launcher_of_another_header_version_is_refused_at_bind_time(libs, tmp_path):
    wrong = compile_fused(SOURCE, "LineBatch", 3, name="line_wrong", flags=["-DEMX_FUSED_BATCH_DATA_ABI=4242u"], cache_dir=str(tmp_path), data=True)
    cat = Catalogue(libs, 3, [5, 9, 7], 131)
    p0 = start(np.random.RandomState(132), 3, 16, 3)
    bt = EnsembleBatch(3, 16, 3, wrong.target(user=cat.rec, ndata=cat.ndata), seeds=[1, 2, 3])
    with pytest.raises(_lib.EmxError) as e:
        bt.run_mcmc(p0, 10)
    assert "another version of emx_fused_target_data.hpp" in str(e.value) and "(code -8)" in str(e.value)
    assert bt.launch_info()["launches"] == 0
    bt.close()
    # the data launcher handed to the plain setter, and a plain launcher handed to the data setter: each answers 1
    plain_of_data = targets.BatchFused(libs[("batch", 3)].launcher, 3, user=cat.rec)
    bt = EnsembleBatch(3, 16, 3, plain_of_data, seeds=[1, 2, 3])
    with pytest.raises(_lib.EmxError) as e:
        bt.run_mcmc(p0, 10)
    assert "another version of emx_fused_target.hpp" in str(e.value) and bt.launch_info()["launches"] == 0
    bt.close()
    src = "struct Flat { __device__ double operator()(const double* x, int ndim, int member, const void* user) const { return 0.0; } };"
    flat = compile_fused(src, "Flat", 3, cache_dir=str(tmp_path))
    bt = EnsembleBatch(3, 16, 3, targets.BatchFused(flat.launcher, 3, ndata=[1, 2, 3]), seeds=[1, 2, 3])
    with pytest.raises(_lib.EmxError) as e:
        bt.run_mcmc(p0, 10)
    assert "another version of emx_fused_target_data.hpp" in str(e.value) and bt.launch_info()["launches"] == 0
    bt.close()


def test_ptsampler_and_tempering_refuse_a_data_target(libs):
    cat = Catalogue(libs, 3, [5, 9, 7, 11], 141)
    with pytest.raises(TypeError) as e:
        PTSampler(2, 16, 3, cat.batch_target(), nbatch=2)
    assert "BatchCallable" in str(e.value) and "BatchKernel" in str(e.value)
    bt = EnsembleBatch(4, 16, 3, cat.batch_target(), seeds=[1, 2, 3, 4])
    h = bt._handle()
    rc = _lib.load().emx_pt_set_tempering(h, 2, np.array([1.0, 0.5]), None, None)
    assert rc != 0 and b"fused user target" in _lib.load().emx_batch_last_error(h)
    bt.close()
