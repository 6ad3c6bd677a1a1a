"""get_rhat on the device (emx_rhat / emx_rhat_batch, csrc/emx_rhat.hip) for EnsembleSampler, EnsembleBatch, a batch member and
PTSampler, on the chain families of tests/chain_families.py and the shapes of tests/test_gpu_chain_offset_reference.py.

  bounds      within and between inside the bounds that tests/rhat_ref.py derives, against fractions.Fraction on the chain that
              get_chain returns; rhat the NumPy expression of the two, bit for bit; both groupings and the log-prob column.  The
              worst error / bound is printed for every case.
  agreement   bt[b] is row b of the batch, PTSampler is its underlying batch, a sub-range of members is the same rows: bit for bit.
  launch      a half of 300 rows spans three slices (RH_SLICE_ROWS = 128 in csrc/emx_rhat.hip: 128 + 128 + 44); members in
              passes of 1, 2 and all: no bit changes.  There is no tuning key for the launch shape.
  scaled      rhat of the scaled family's chain is the centred family's, bit for bit.
  meaning     two members 20 sd apart: the pooled R-hat is large, the members' own are not.
  host chain  a user-written move keeps the chain on the host: get_rhat is split_rhat(get_chain())."""
import numpy as np
import pytest

import chain_families as cf
import rhat_ref as rr
from emcee_amd import EnsembleBatch, EnsembleSampler, PTSampler, moves, summary, targets
from emcee_amd.targets import BatchCallable

from test_gpu_chain_offset_reference import BATCH, SELECTIONS, run_batch, run_single

pytestmark = pytest.mark.gpu

SINGLE = {"66x7": (66, 7, 37), "48x17": (48, 17, 12)}
PT = (3, 32, 4, 40, 2)             # rungs, walkers, ndim, steps, objects
SLICE_ROWS = 128                   # RH_SLICE_ROWS of csrc/emx_rhat.hip
_PT_RUNS = {}


def selected(steps, discard, thin):
    return len(range(min(discard + thin - 1, steps), steps, thin))


def run_pt(name):
    if name in _PT_RUNS:
        return _PT_RUNS[name]
    import torch
    T, N, D, steps, objects = PT
    seed = sum(ord(c) for c in repr(PT)) % 100000
    fam = cf.family(name, D, seed)
    mu_t, iv_t = torch.as_tensor(fam["mu"], device="cuda"), torch.as_tensor(fam["ivar"], device="cuda")

    def loglike(q):
        r = q - mu_t
        return -0.5 * (iv_t * r * r).sum(-1)
    s = PTSampler(T, N, D, BatchCallable(loglike), Tmax=8.0, nbatch=objects, seeds=[seed + 1 + b for b in range(objects)])
    s.run_mcmc(cf.start_cloud(fam, (objects, T, N), seed + 2), steps, skip_initial_state_check=True)
    _PT_RUNS[name] = (s, fam)
    return s, fam


def same(a, b):
    return all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a[:3], b[:3])) and tuple(a[3:]) == tuple(b[3:])


def row(r, i):
    return summary.RHat(r.rhat[i], r.within[i], r.between[i], r.nchains, r.length)


def without_log_prob(r):
    return summary.RHat(r.rhat[..., :-1], r.within[..., :-1], r.between[..., :-1], r.nchains, r.length)


# ---------------------------------------------------------------------------------------------------------------- bounds
@pytest.mark.parametrize("name", cf.FAMILIES)
@pytest.mark.parametrize("shape", sorted(SINGLE))
def test_single_sampler_bounds(shape, name):
    N, D, steps = SINGLE[shape]
    s, fam = run_single(N, D, steps, name)
    for discard, thin in SELECTIONS:
        what = "single %s %s discard=%d thin=%d" % (shape, name, discard, thin)
        if selected(steps, discard, thin) < 4:
            with pytest.raises(ValueError, match="at least 4"):
                s.get_rhat(discard=discard, thin=thin)
            continue
        r = s.get_rhat(discard=discard, thin=thin, log_prob=True)
        assert r.rhat.shape == (D + 1,) and r.nchains == 2 * N
        rr.check(r, rr.chains_of(s.get_chain(discard=discard, thin=thin), s.get_log_prob(discard=discard, thin=thin)), what)
        assert np.array_equal(r.rhat, np.sqrt((r.length - 1) / r.length + r.between / r.within)), what
        assert same(s.get_rhat(discard=discard, thin=thin), without_log_prob(r)), what
        assert np.isfinite(r.rhat).all() and (r.rhat > 0.5).all(), what


@pytest.mark.parametrize("name", cf.FAMILIES)
@pytest.mark.parametrize("shape", sorted(BATCH))
def test_batch_bounds_and_agreement(shape, name):
    B, N, D, steps = BATCH[shape]
    bt, fam = run_batch(B, N, D, steps, name)
    for discard, thin in SELECTIONS:
        what = "batch %s %s discard=%d thin=%d" % (shape, name, discard, thin)
        if selected(steps, discard, thin) < 4:
            for get in (bt.get_rhat, bt[0].get_rhat):
                with pytest.raises(ValueError, match="at least 4"):
                    get(discard=discard, thin=thin)
            continue
        x = bt.get_chain(discard=discard, thin=thin).transpose(1, 0, 2, 3)
        lp = bt.get_log_prob(discard=discard, thin=thin).transpose(1, 0, 2)
        r = bt.get_rhat(discard=discard, thin=thin, log_prob=True)
        assert r.rhat.shape == (B, D + 1) and r.nchains == 2 * N
        rr.check(r, rr.chains_of(x, lp), what + " walkers")
        pooled = bt.get_rhat(discard=discard, thin=thin, chains="members", log_prob=True)
        assert pooled.rhat.shape == (D + 1,) and pooled.nchains == 2 * N * B
        rr.check(pooled, rr.chains_of(x, lp, pool=True), what + " members")
        for q in (r, pooled):
            assert np.array_equal(q.rhat, np.sqrt((q.length - 1) / q.length + q.between / q.within)), what
        assert same(bt.get_rhat(discard=discard, thin=thin), without_log_prob(r)), what
        assert same(bt.get_rhat(discard=discard, thin=thin, chains="members"), without_log_prob(pooled)), what
        # a member on its own, a sub-range of members, members in passes of one: the same bits
        for b in range(B):
            assert same(bt[b].get_rhat(discard=discard, thin=thin, log_prob=True), row(r, b)), (what, b)
        if B > 2:
            sub = bt._rhat(discard, thin, 1, B, 0, True)
            assert same(sub, row(r, slice(1, B))), what
        bt.set_tuning("batch_rhat_members", 1)
        again, pooled_again = bt.get_rhat(discard=discard, thin=thin, log_prob=True), bt.get_rhat(discard=discard, thin=thin, chains="members", log_prob=True)
        bt.set_tuning("batch_rhat_members", 0)
        assert same(again, r) and same(pooled_again, pooled), what


@pytest.mark.parametrize("name", cf.FAMILIES)
def test_ptsampler_bounds_and_its_batch(name):
    s, fam = run_pt(name)
    T, N, D, steps, objects = PT
    M = T * objects
    for discard, thin in SELECTIONS:
        what = "pt %s discard=%d thin=%d" % (name, discard, thin)
        x = s.get_chain(discard=discard, thin=thin)                 # (objects, T, nt, N, D)
        lp = s.get_log_prob(discard=discard, thin=thin)
        r = s.get_rhat(discard=discard, thin=thin, log_prob=True)
        assert r.rhat.shape == (objects, T, D + 1) and r.nchains == 2 * N
        flat = summary.RHat(*[a.reshape(M, D + 1) for a in r[:3]], r.nchains, r.length)
        rr.check(flat, rr.chains_of(x.reshape((M,) + x.shape[2:]).transpose(1, 0, 2, 3), lp.reshape((M,) + lp.shape[2:]).transpose(1, 0, 2)),
                 what + " walkers")
        assert same(flat, s._b.get_rhat(discard=discard, thin=thin, log_prob=True)), what
        pooled = s.get_rhat(discard=discard, thin=thin, chains="members", log_prob=True)
        assert pooled.rhat.shape == (T, D + 1) and pooled.nchains == 2 * N * objects
        assert same(pooled, s._b._rhat(discard, thin, 0, M, T, True)), what
        for t in range(T):
            rr.check(row(pooled, t), rr.chains_of(x[:, t].transpose(1, 0, 2, 3), lp[:, t].transpose(1, 0, 2), pool=True), what + " rung %d pooled" % t)
        assert same(s.get_rhat(discard=discard, thin=thin), without_log_prob(r)), what


# ---------------------------------------------------------------------------------------------------------------- the launch
@pytest.mark.parametrize("name", ["centred", "offset_34"])
def test_no_bit_depends_on_the_pass_size_when_a_half_spans_several_slices(name):
    B, N, D, steps = 3, 32, 5, 601
    bt, fam = run_batch(B, N, D, steps, name, cache=False)
    assert steps // 2 > 2 * SLICE_ROWS
    ref = {}
    for members in (0, 1, 2):
        bt.set_tuning("batch_rhat_members", members)
        for discard, thin in ((0, 1), (1, 1), (5, 3)):              # halves of 300 rows (odd nt, then even) and of 99
            got = (bt.get_rhat(discard=discard, thin=thin, log_prob=True), bt.get_rhat(discard=discard, thin=thin, chains="members", log_prob=True),
                   bt[1].get_rhat(discard=discard, thin=thin, log_prob=True))
            if members == 0:
                ref[discard, thin] = got
                assert same(got[2], row(got[0], 1))
                # the slices add up to the right numbers (the bounds are held at the short shapes above)
                x = bt.get_chain(discard=discard, thin=thin).transpose(1, 0, 2, 3) - fam["mu"]
                lp = bt.get_log_prob(discard=discard, thin=thin).transpose(1, 0, 2)
                for q, pool in ((got[0], False), (got[1], True)):
                    host = summary.split_rhat(x, log_prob=lp, pool=pool)
                    assert (q.nchains, q.length) == (host.nchains, host.length)
                    np.testing.assert_allclose(q.within, host.within, rtol=1e-11)
                    np.testing.assert_allclose(q.between, host.between, rtol=1e-9)
            else:
                assert all(same(u, v) for u, v in zip(got, ref[discard, thin])), (name, members, discard, thin)
    bt.set_tuning("batch_rhat_members", 0)
    bt.close()


# ---------------------------------------------------------------------------------------------------------------- scale covariance
def _scaled_same(a, b, sc):
    assert np.array_equal(a.get_chain() * sc, b.get_chain()) and np.array_equal(a.get_log_prob(), b.get_log_prob())       # the premise
    scw = np.concatenate([sc, [1.0]])
    for discard, thin in SELECTIONS:
        for kw in ({}, {"chains": "members"}) if isinstance(a, EnsembleBatch) else ({},):
            ra = a.get_rhat(discard=discard, thin=thin, log_prob=True, **kw)
            rb = b.get_rhat(discard=discard, thin=thin, log_prob=True, **kw)
            assert np.array_equal(ra.rhat, rb.rhat) and np.isfinite(ra.rhat).all()
            assert np.array_equal(ra.within * scw * scw, rb.within) and np.array_equal(ra.between * scw * scw, rb.between)


def test_scaled_against_centred_single():
    N, D, steps = SINGLE["66x7"]
    (a, _), (b, fam) = run_single(N, D, steps, "centred"), run_single(N, D, steps, "scaled")
    _scaled_same(a, b, fam["scale"])


def test_scaled_against_centred_batch():
    B, N, D, steps = BATCH["3_of_32x5"]
    (a, _), (b, fam) = run_batch(B, N, D, steps, "centred"), run_batch(B, N, D, steps, "scaled")
    _scaled_same(a, b, fam["scale"])


# ---------------------------------------------------------------------------------------------------------------- what it measures
def test_pooled_rhat_sees_members_that_disagree():
    N, D, steps = 32, 2, 40
    sd = np.array([0.7, 1.3])
    mus = [np.array([-10.0 * sd[0], 0.0]), np.array([10.0 * sd[0], 0.0])]            # 20 sd apart in parameter 0
    rs = np.random.RandomState(3)
    bt = EnsembleBatch(2, N, D, [targets.DiagGaussian(mu, 1.0 / sd ** 2) for mu in mus], seeds=[11, 12])
    bt.run_mcmc(np.stack([mu + sd * rs.randn(N, D) for mu in mus]), steps)
    pooled = bt.get_rhat(chains="members")
    own = bt.get_rhat()
    print("pooled rhat %s, members' own %s" % (pooled.rhat, own.rhat))
    assert pooled.rhat[0] > 2
    assert pooled.rhat[1] < pooled.rhat[0]
    assert (own.rhat[:, 0] < pooled.rhat[0]).all()
    assert pooled.nchains == 4 * N and own.nchains == 2 * N and pooled.length == own.length == steps // 2
    bt.close()


# ---------------------------------------------------------------------------------------------------------------- a chain on the host
def test_user_written_move_goes_through_split_rhat():
    class MyStretch(moves.RedBlueMove):
        def get_proposal(self, s, c, random):
            c = np.concatenate(c, axis=0)
            zz = ((2.0 - 1.0) * random.rand(len(s)) + 1) ** 2.0 / 2.0
            rint = random.randint(len(c), size=(len(s),))
            return c[rint] - (c[rint] - s) * zz[:, None], (s.shape[1] - 1.0) * np.log(zz)

    s = EnsembleSampler(32, 3, lambda p: -0.5 * np.sum(p ** 2), moves=MyStretch())
    s._random.seed(8)
    s.run_mcmc(np.random.RandomState(4).randn(32, 3), 15)
    assert s.backend._dev is None
    for discard, thin in ((0, 1), (2, 2)):
        for lp in (False, True):
            got = s.get_rhat(discard=discard, thin=thin, log_prob=lp)
            ref = summary.split_rhat(s.get_chain(discard=discard, thin=thin), log_prob=s.get_log_prob(discard=discard, thin=thin) if lp else None)
            assert isinstance(got, summary.RHat) and same(got, ref) and got.rhat.shape == (3 + lp,)
    with pytest.raises(ValueError, match="chains"):
        s.get_rhat(chains="members")
