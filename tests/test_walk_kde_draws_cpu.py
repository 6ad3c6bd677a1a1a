"""Host twin of the WalkMove / KDEMove native draws (emx_host_walk_kde_draws; csrc/emx_rng.hpp wk_*): no GPU needed."""
import ctypes as C

import numpy as np
import pytest
from scipy import stats

from emcee_amd import _lib
from emx_testlib import philox_plan

SEED, STEP = 0x5EED1234, 7


def walk(s, nsplits=2):
    return _lib.MoveDesc(_lib.MOVE_WALK, nsplits, 1, 0 if s is None else s, 0.0, 0.0, 0.0, 0.0)


def kde(rule=0, a=0.0, nsplits=2):
    return _lib.MoveDesc(_lib.MOVE_KDE, nsplits, 1, rule, a, 0.0, 0.0, 0.0)


def draws(md, N, D, split, seed=SEED, step=STEP):
    lib = _lib.load()
    S = md.nsplits
    ns = (N - split + S - 1) // S
    s = md.reserved if md.kind == _lib.MOVE_WALK else 0
    nh = s if s >= 2 else (1 if md.kind == _lib.MOVE_KDE else 0)
    nz = s if s >= 2 else D
    helpers = np.full(max(ns * nh, 1), -7, dtype=np.int32)
    normals = np.empty(ns * nz)
    got = lib.emx_host_walk_kde_draws(seed, step, N, D, C.byref(md), split,
                                      helpers.ctypes.data_as(C.c_void_p) if nh else None, normals)
    assert got == ns
    return helpers[:ns * nh].reshape(ns, nh), normals.reshape(ns, nz)


def complement(plan, split):
    off, order = plan["off"], plan["order"]
    return np.concatenate([order[off[j]:off[j + 1]] for j in range(len(off) - 1) if j != split])


@pytest.mark.parametrize("md", [walk(3), walk(None), kde(), walk(4, nsplits=3), kde(1, nsplits=4)])
def test_plan_split_and_uacc_equal_the_stretch_move(md):
    N = 1000
    ref = philox_plan(SEED, STEP, N, _lib.MoveDesc(_lib.MOVE_STRETCH, md.nsplits, 1, 0, 2.0, 0.0, 0.0, 0.0))
    got = philox_plan(SEED, STEP, N, md)
    for k in ("off", "order", "uacc"):
        assert np.array_equal(got[k], ref[k]), k


@pytest.mark.parametrize("s", [2, 3, 8])
def test_walk_helpers_distinct_in_the_complement_and_uniform(s):
    N, D = 4096, 4
    counts = np.zeros(N)
    for step in range(6):
        plan = philox_plan(SEED, step, N, walk(s))
        for split in range(2):
            comp = set(complement(plan, split).tolist())
            h, _ = draws(walk(s), N, D, split, step=step)
            assert all(len(set(row)) == s for row in h)
            assert set(h.ravel().tolist()) <= comp
            np.add.at(counts, h.ravel(), 1)
    # every walker is in the complement of exactly one split per step: expected count 6 * 2048 * s / 2048 per walker
    expected = counts.sum() / N
    chi2 = ((counts - expected) ** 2 / expected).sum()
    assert stats.chi2.sf(chi2, N - 1) > 1e-4, chi2


def test_walk_whole_draw_of_small_complement_is_a_permutation():
    # s == Nc: Floyd returns every complement member once
    N = 10
    plan = philox_plan(SEED, STEP, N, walk(5))
    h, _ = draws(walk(5), N, 3, 1)
    comp = sorted(complement(plan, 1).tolist())
    for row in h:
        assert sorted(row.tolist()) == comp


@pytest.mark.parametrize("md,D", [(walk(8), 4), (walk(None), 16), (kde(), 64)])
def test_normals_are_standard(md, D):
    z = np.concatenate([draws(md, 4096, D, sp, step=st)[1].ravel() for st in range(3) for sp in range(2)])
    assert abs(z.mean()) < 5 / np.sqrt(z.size)
    assert abs(z.var() - 1) < 6 * np.sqrt(2 / z.size)
    assert stats.kstest(z, "norm").pvalue > 1e-4


def test_kde_centre_uniform_over_the_complement():
    N = 4096
    counts = np.zeros(N)
    for step in range(40):
        plan = philox_plan(SEED, step, N, kde())
        for split in range(2):
            h, _ = draws(kde(), N, 2, split, step=step)
            assert set(h[:, 0].tolist()) <= set(complement(plan, split).tolist())
            np.add.at(counts, h[:, 0], 1)
    expected = counts.sum() / N
    chi2 = ((counts - expected) ** 2 / expected).sum()
    assert stats.chi2.sf(chi2, N - 1) > 1e-4, chi2


def test_draws_are_a_pure_function_of_seed_and_step():
    a = draws(walk(3), 512, 4, 0)
    b = draws(walk(3), 512, 4, 0)
    c = draws(walk(3), 512, 4, 0, step=STEP + 1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[1], c[1])


def test_bad_arguments_are_refused():
    lib = _lib.load()
    z = np.empty(64)
    for md in (walk(1), _lib.MoveDesc(_lib.MOVE_STRETCH, 2, 1, 0, 2.0, 0.0, 0.0, 0.0)):
        assert lib.emx_host_walk_kde_draws(SEED, STEP, 16, 2, C.byref(md), 0, None, z) == -1
    assert lib.emx_host_walk_kde_draws(SEED, STEP, 16, 2, C.byref(walk(9)), 0, None, z) == -1     # s > Nc = 8


def test_native_desc_gates_the_new_kinds_on_philox():
    from emcee_amd import moves
    from emcee_amd.ensemble import _native_desc
    for mv in (moves.WalkMove(), moves.WalkMove(s=3), moves.KDEMove(), moves.KDEMove(bw_method="silverman"),
               moves.KDEMove(bw_method=0.5)):
        assert _native_desc(mv, 4) is None
        d = _native_desc(mv, 4, philox=True)
        assert d is not None and d.kind in (_lib.MOVE_WALK, _lib.MOVE_KDE)
        assert not mv._is_native()          # propose() keeps the host get_proposal (MT19937 plans)
    assert _native_desc(moves.WalkMove(s=3), 4, philox=True).reserved == 3
    assert _native_desc(moves.KDEMove(bw_method=0.5), 4, philox=True).a == 0.5
    for mv, nd in ((moves.WalkMove(s=1), 4), (moves.KDEMove(bw_method=lambda k: 0.3), 4), (moves.KDEMove(), 130),
                   (moves.WalkMove(), 130)):
        assert _native_desc(mv, nd, philox=True) is None

    class MyWalk(moves.WalkMove):
        def get_proposal(self, s, c, random):
            return super().get_proposal(s, c, random)
    assert _native_desc(MyWalk(), 4, philox=True) is None
