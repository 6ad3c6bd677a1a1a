"""EnsembleBatch: B independent ensembles in one launch a chunk.  Every member must be bit for bit the single Philox-mode
EnsembleSampler with the same seed, target and initial state; the launch shape must not change a bit."""
import time

import numpy as np
import pytest

import emcee_amd
from emcee_amd import EnsembleBatch, EnsembleSampler, moves, targets

pytestmark = pytest.mark.gpu


def p0_for(rs, B, N, D, kind):
    if kind == "box":
        return rs.rand(B, N, D)
    if kind == "rosen":
        return 1.0 + 0.1 * rs.randn(B, N, D)
    return rs.randn(B, N, D)


def member_targets(kind, B, D, rs, per_member):
    def one():
        if kind == "iso":
            return targets.IsoGaussian()
        if kind == "rosen":
            return targets.Rosenbrock(20.0)
        if kind == "box":
            return targets.UniformBox()
        if kind == "diag":
            return targets.DiagGaussian(0.1 * rs.randn(D), 1.0 / (0.2 + rs.rand(D)))
        A = rs.randn(D, D)
        icov = np.linalg.inv(A @ A.T / D + 0.5 * np.eye(D))
        return targets.DenseGaussian(0.1 * rs.randn(D), 0.5 * (icov + icov.T))
    if per_member:
        return [one() for _ in range(B)]
    return one()


def single(N, D, target, move_factory, seed, p0, nsteps, thin_by=1, store=True, skip=False, chunks=None):
    s = EnsembleSampler(N, D, target, moves=move_factory(), rng="philox")
    s.random_state = np.random.RandomState(seed).get_state()
    if chunks is None:
        s.final = s.run_mcmc(p0, nsteps, thin_by=thin_by, store=store, skip_initial_state_check=skip)
    else:
        s.final = s.run_mcmc(p0, chunks[0], thin_by=thin_by, store=store, skip_initial_state_check=skip)
        for n in chunks[1:]:
            s.final = s.run_mcmc(None, n, thin_by=thin_by, store=store, skip_initial_state_check=skip)
    return s


def assert_member_equal(batch, b, s, store=True):
    last, ref = batch.get_last_sample(), s.final
    assert np.array_equal(last.coords[b], ref.coords), "member %d: final coordinates" % b
    assert np.array_equal(last.log_prob[b], ref.log_prob), "member %d: final log-probs" % b
    assert batch._step == s._philox_step, "member %d: Philox step" % b
    if store:
        assert batch.iteration == s.iteration
        assert np.array_equal(batch[b].get_chain(), s.get_chain()), "member %d: chain" % b
        assert np.array_equal(batch[b].get_log_prob(), s.get_log_prob()), "member %d: log-prob chain" % b
        assert np.array_equal(batch[b].acceptance_fraction, s.acceptance_fraction), "member %d: accept counts" % b


def members_to_check(B):
    return list(range(B)) if B <= 8 else sorted({0, 1, B // 3, B // 2, B - 2, B - 1})


stretch = lambda: moves.StretchMove()  # noqa: E731

CASES = {
    # name: (N, D, target kind, per-member target, moves, B, skip the conditioning check)
    "iso_32x5": (32, 5, "iso", False, stretch, 3, False),
    "iso_45x2_3splits": (45, 2, "iso", False, lambda: moves.StretchMove(nsplits=3), 3, False),
    "rosen_64x8": (64, 8, "rosen", False, stretch, 3, False),
    "diag_66x7_members": (66, 7, "diag", True, lambda: moves.DEMove(), 3, False),
    "box_32x1": (32, 1, "box", False, stretch, 3, False),
    "diag_40x130": (40, 130, "diag", True, lambda: moves.StretchMove(nsplits=5, live_dangerously=True), 2, True),
    "iso_1024x8": (1024, 8, "iso", False, stretch, 2, False),
    "iso_2x1": (2, 1, "iso", False, stretch, 3, True),
    "dense_128x16_members": (128, 16, "dense", True, stretch, 3, False),
    "dense_64x32_members_mix": (64, 32, "dense", True, lambda: [moves.StretchMove(), moves.DEMove(), moves.DESnookerMove()], 3, False),
    "snooker_50x3": (50, 3, "iso", False, lambda: moves.DESnookerMove(), 3, False),
    "gauss_vector": (32, 4, "diag", True, lambda: moves.GaussianMove(0.3), 3, False),
    "gauss_random_factor": (32, 4, "iso", False, lambda: moves.GaussianMove([0.5, 0.3, 0.4, 0.2], mode="random", factor=2.0), 3, False),
    "gauss_sequential": (32, 4, "iso", False, lambda: moves.GaussianMove(0.5, mode="sequential"), 3, False),
    "gauss_sequential_factor": (32, 4, "iso", False, lambda: moves.GaussianMove(0.5, mode="sequential", factor=1.5), 3, False),
    "mix_32x5": (32, 5, "iso", False, lambda: [(moves.StretchMove(), 0.5), (moves.DEMove(), 0.3), (moves.DESnookerMove(), 0.2)], 3, False),
    "mix_gauss_stretch": (32, 5, "rosen", False, lambda: [(moves.StretchMove(), 0.7), (moves.GaussianMove(0.05), 0.3)], 3, False),
    "iso_32x5_B1": (32, 5, "iso", False, stretch, 1, False),
    "iso_32x5_B37": (32, 5, "iso", True, stretch, 37, False),
    "diag_32x5_B300": (32, 5, "diag", True, lambda: [moves.StretchMove(), moves.DEMove()], 300, False),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_members_equal_single_sampler(name):
    N, D, kind, per_member, mf, B, skip = CASES[name]
    rs = np.random.RandomState(len(name))
    tg = member_targets(kind, B, D, rs, per_member)
    p0 = p0_for(rs, B, N, D, kind)
    seeds = [1000 + 17 * b for b in range(B)]
    nsteps = 12 if N * D > 4000 else 25
    batch = EnsembleBatch(B, N, D, tg, moves=mf(), seeds=seeds)
    batch.run_mcmc(p0, nsteps, skip_initial_state_check=skip)
    for b in members_to_check(B):
        s = single(N, D, tg[b] if per_member else tg, mf, seeds[b], p0[b], nsteps, skip=skip)
        assert_member_equal(batch, b, s)
    assert batch.launch_info()["launches"] == 2        # the initial log-probs, then the run
    batch.close()


def test_permuting_members_permutes_outputs():
    B, N, D = 6, 32, 5
    rs = np.random.RandomState(7)
    tg = member_targets("diag", B, D, rs, True)
    p0 = p0_for(rs, B, N, D, "diag")
    seeds = list(range(50, 50 + B))
    perm = [3, 0, 5, 1, 4, 2]
    a = EnsembleBatch(B, N, D, tg, moves=[moves.StretchMove(), moves.DEMove()], seeds=seeds)
    a.run_mcmc(p0, 30)
    b = EnsembleBatch(B, N, D, [tg[k] for k in perm], moves=[moves.StretchMove(), moves.DEMove()], seeds=[seeds[k] for k in perm])
    b.run_mcmc(p0[perm], 30)
    assert np.array_equal(a.get_chain()[perm], b.get_chain())
    assert np.array_equal(a.get_log_prob()[perm], b.get_log_prob())
    assert np.array_equal(a.acceptance_fraction[perm], b.acceptance_fraction)
    # one member's p0 and seed changed: only that member's outputs change
    p1 = p0.copy()
    p1[2] += 0.01
    seeds2 = list(seeds)
    seeds2[4] = 999
    c = EnsembleBatch(B, N, D, tg, moves=[moves.StretchMove(), moves.DEMove()], seeds=seeds2)
    c.run_mcmc(p1, 30)
    ca, cc = a.get_chain(), c.get_chain()
    for k in range(B):
        assert np.array_equal(ca[k], cc[k]) == (k not in (2, 4)), k


@pytest.mark.parametrize("kind,N,D,B", [("iso", 32, 5, 300), ("dense", 64, 16, 20), ("diag", 100, 10, 40)])
def test_launch_shape_does_not_change_bits(kind, N, D, B):
    rs = np.random.RandomState(3)
    tg = member_targets(kind, B, D, rs, kind != "iso")
    p0 = p0_for(rs, B, N, D, kind)
    outs, shapes = [], []
    for threads, plan_steps in ((0, 0), (64, 1), (256, 7), (1024, 0)):
        bt = EnsembleBatch(B, N, D, tg, moves=[moves.StretchMove(), moves.DESnookerMove()], seeds=list(range(B)))
        bt.set_tuning("batch_threads", threads)
        bt.set_tuning("batch_plan_steps", plan_steps)
        bt.run_mcmc(p0, 40)
        shapes.append(bt.launch_info())
        outs.append((bt.get_chain(), bt.get_log_prob(), bt.acceptance_fraction))
        bt.close()
    assert len({(s["threads"], s["plan_steps"]) for s in shapes}) >= 3, shapes
    for o in outs[1:]:
        for x, y in zip(outs[0], o):
            assert np.array_equal(x, y)


def test_chunking_resume_thinning_and_growth():
    B, N, D = 4, 32, 5
    rs = np.random.RandomState(11)
    tg = targets.IsoGaussian()
    p0 = p0_for(rs, B, N, D, "iso")
    seeds = [5, 6, 7, 8]
    one = EnsembleBatch(B, N, D, tg, seeds=seeds)
    one.run_mcmc(p0, 50)
    two = EnsembleBatch(B, N, D, tg, seeds=seeds)
    two.run_mcmc(p0, 30)
    two.run_mcmc(None, 20)                  # the chain grows across the calls and keeps what it stored
    assert np.array_equal(one.get_chain(), two.get_chain()) and np.array_equal(one.get_log_prob(), two.get_log_prob())
    assert np.array_equal(one.acceptance_fraction, two.acceptance_fraction)
    for b in range(B):
        s = single(N, D, tg, stretch, seeds[b], p0[b], None, chunks=(30, 20))
        assert_member_equal(two, b, s)
        for kw in (dict(discard=7, thin=3), dict(flat=True), dict(discard=5, thin=2, flat=True)):
            assert np.array_equal(two[b].get_chain(**kw), s.get_chain(**kw))
            assert np.array_equal(two.get_chain(**kw)[b], s.get_chain(**kw))
            assert np.array_equal(two.get_log_prob(**kw)[b], s.get_log_prob(**kw))
        np.testing.assert_array_equal(two.get_autocorr_time(quiet=True)[b],
                                      emcee_amd.autocorr.integrated_time(s.get_chain(), quiet=True))
    # thin_by and store=False
    th = EnsembleBatch(B, N, D, tg, seeds=seeds)
    th.run_mcmc(p0, 10, thin_by=3)
    ns = EnsembleBatch(B, N, D, tg, seeds=seeds)
    ns.run_mcmc(p0, 10, store=False)
    for b in range(B):
        assert_member_equal(th, b, single(N, D, tg, stretch, seeds[b], p0[b], 10, thin_by=3))
        assert_member_equal(ns, b, single(N, D, tg, stretch, seeds[b], p0[b], 10, store=False), store=False)
    assert ns.iteration == 0


def test_nan_member_is_named_and_others_untouched():
    B, N, D = 5, 32, 5
    rs = np.random.RandomState(2)
    p0 = p0_for(rs, B, N, D, "iso")
    bt = EnsembleBatch(B, N, D, targets.IsoGaussian(), seeds=list(range(B)))
    bt.run_mcmc(p0, 10)
    before = (bt.get_chain(), bt.get_last_sample().coords)
    bad = bt.get_last_sample().coords.copy()
    bad[3, 7, 2] = np.nan
    with pytest.raises(ValueError, match="member 3"):
        bt.run_mcmc(bad, 10)
    assert np.array_equal(bt.get_chain(), before[0]) and np.array_equal(bt.get_last_sample().coords, before[1])


def test_throughput_512_members():
    N, D, nsteps = 32, 5, 2000
    rs = np.random.RandomState(0)
    tg = targets.IsoGaussian()
    s = EnsembleSampler(N, D, tg, rng="philox")
    s.run_mcmc(rs.randn(N, D), 50, store=False)             # warm-up
    t0 = time.perf_counter()
    s.run_mcmc(None, nsteps, store=False)
    t_single = time.perf_counter() - t0
    p0 = rs.randn(512, N, D)
    bt = EnsembleBatch(512, N, D, tg, seeds=list(range(512)))
    bt.run_mcmc(p0, 50, store=False)                          # warm-up
    t0 = time.perf_counter()
    bt.run_mcmc(None, nsteps, store=False)
    t_batch = time.perf_counter() - t0
    print("single %.3f ms, batch of 512 %.3f ms (%.0fx the single rate)" % (1e3 * t_single, 1e3 * t_batch, 512 * t_single / t_batch))
    assert t_batch < 512 * t_single / 20
