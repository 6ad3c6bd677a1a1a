"""tests/hiprec.py, the double-double reference of the walk / KDE GPU tests: its kernels against exact rational arithmetic
(fractions.Fraction) and mpmath, its covariance against np.cov and its KDE log ratio against scipy's gaussian_kde."""
from fractions import Fraction

import mpmath
import numpy as np
import pytest
from scipy.stats import gaussian_kde

import hiprec as hp

REL = 2.0 ** -100


def F(x):
    return Fraction(float(x))


def ddF(x, i=()):
    return F(x[0][i]) + F(x[1][i])


def _inputs(rs, n=400):
    """ordinary, cancelling and extreme-exponent operands"""
    a = rs.randn(n) * 2.0 ** rs.randint(-40, 40, n)
    b = rs.randn(n) * 2.0 ** rs.randint(-40, 40, n)
    b[:50] = -a[:50] * (1 + rs.randn(50) * 2.0 ** -40)                # near-total cancellation
    b[50:60] = -a[50:60]                                             # exact cancellation
    a[60:80] = rs.uniform(1, 2, 20) * 2.0 ** 1000                    # near overflow (sums, products of one large and one small)
    b[60:80] = rs.uniform(1, 2, 20) * 2.0 ** rs.randint(-60, 20, 20)
    a[80:100] = rs.uniform(1, 2, 20) * 2.0 ** -480                   # small: products near 2^-960 stay exact
    b[80:100] = rs.uniform(1, 2, 20) * 2.0 ** -480
    return a, b


def test_two_sum_and_two_prod_are_exact():
    rs = np.random.RandomState(0)
    a, b = _inputs(rs)
    s, e = hp.two_sum(a, b)
    p, f = hp.two_prod(a, b)
    for i in range(len(a)):
        assert F(s[i]) + F(e[i]) == F(a[i]) + F(b[i]), i
        assert F(p[i]) + F(f[i]) == F(a[i]) * F(b[i]), i
        assert s[i] == a[i] + b[i] and p[i] == a[i] * b[i]


def test_split_is_exact_near_overflow():
    x = np.array([2.0 ** 1022 * 1.9999, -2.0 ** 1000 * 1.2345, 2.0 ** 997 * 1.5, 3.0, 2.0 ** -1000])
    h, l = hp.split(x)
    for i in range(len(x)):
        assert F(h[i]) + F(l[i]) == F(x[i])
    p, f = hp.two_prod(np.array([2.0 ** 1000 * 1.3]), np.array([2.0 ** 20 * 1.1]))
    assert np.isfinite(p[0]) and F(p[0]) + F(f[0]) == F(2.0 ** 1000 * 1.3) * F(2.0 ** 20 * 1.1)


def _dd_operands(rs, n=300):
    a, b = _inputs(rs, n)
    x = hp.fast_two_sum(a, a * rs.uniform(-1, 1, n) * 2.0 ** -54)
    y = hp.fast_two_sum(b, b * rs.uniform(-1, 1, n) * 2.0 ** -54)
    return x, y


@pytest.mark.parametrize("op", ["add", "sub", "mul", "div"])
def test_double_double_ops_against_fractions(op):
    rs = np.random.RandomState(1 + len(op))
    x, y = _dd_operands(rs)
    if op in ("mul", "div"):                              # keep the results inside the range where products are exact
        keep = np.abs(np.log2(np.abs(x[0])) + (1 if op == "mul" else -1) * np.log2(np.abs(y[0]))) < 900
        keep &= np.abs(np.log2(np.abs(x[0]))) < 900
        x = (x[0][keep], x[1][keep])
        y = (y[0][keep], y[1][keep])
    r = getattr(hp, op)(x, y)
    for i in range(len(x[0])):
        xf, yf = ddF(x, i), ddF(y, i)
        want = {"add": xf + yf, "sub": xf - yf, "mul": xf * yf, "div": xf / yf if yf else None}[op]
        if want is None:
            continue
        got = ddF(r, i)
        scale = abs(xf) + abs(yf) if op in ("add", "sub") else abs(want)
        assert abs(got - want) <= REL * scale, (op, i)
        assert r[0][i] == r[0][i] + r[1][i]               # normalised


def test_sqrt_and_sum_against_mpmath():
    mpmath.mp.prec = 300
    rs = np.random.RandomState(3)
    v = rs.uniform(0.5, 2, 200) * 2.0 ** rs.randint(-900, 900, 200)
    x = hp.fast_two_sum(v, v * rs.uniform(-1, 1, 200) * 2.0 ** -54)
    r = hp.sqrt(x)
    for i in range(200):
        want = mpmath.sqrt(mpmath.mpf(x[0][i]) + mpmath.mpf(x[1][i]))
        got = mpmath.mpf(r[0][i]) + mpmath.mpf(r[1][i])
        assert abs(got - want) <= REL * want, i
    assert hp.sqrt(hp.dd(np.array([0.0])))[0][0] == 0.0
    # a sum with heavy cancellation: the exact value is what remains
    t = rs.randn(1001) * 2.0 ** rs.randint(-30, 30, 1001)
    t = np.concatenate([t, -t[:1000], [2.0 ** -70]])
    rs.shuffle(t)
    s = hp.dsum(hp.dd(t))
    want = sum(F(u) for u in t)
    assert abs(ddF(s) - want) <= REL * sum(abs(F(u)) for u in t)


def test_rowdot_against_fractions():
    """ordinary rows, rows that cancel almost completely, and an odd number of columns"""
    rs = np.random.RandomState(5)
    n, D = 12, 37
    a = rs.randn(n, D) * 2.0 ** rs.randint(-20, 20, (n, D))
    b = rs.randn(n, D) * 2.0 ** rs.randint(-20, 20, (n, D))
    a[:4, 18:36], b[:4, 18:36] = a[:4, :18], -b[:4, :18] * (1 + rs.randn(4, 18) * 2.0 ** -45)
    x = hp.fast_two_sum(a, a * rs.uniform(-1, 1, (n, D)) * 2.0 ** -54)
    y = hp.fast_two_sum(b, b * rs.uniform(-1, 1, (n, D)) * 2.0 ** -54)
    r = hp.rowdot(x, y)
    assert r[0].shape == (n,)
    for i in range(n):
        terms = [ddF(x, (i, d)) * ddF(y, (i, d)) for d in range(D)]
        assert abs(ddF(r, i) - sum(terms)) <= REL * sum(abs(t) for t in terms), i


def test_walk_weights_sum_to_zero_and_proposal_exact():
    rs = np.random.RandomState(4)
    ns, s, D = 5, 7, 3
    z = rs.randn(ns, s)
    w = hp.walk_weights(z)
    for t in range(ns):
        zs = [F(u) for u in z[t]]
        zbar = sum(zs) / s
        want = [(u - zbar) for u in zs]
        k = mpmath.mpf(1) / mpmath.sqrt(s - 1)
        for j in range(s):
            got = mpmath.mpf(w[0][t, j]) + mpmath.mpf(w[1][t, j])
            ref = mpmath.mpf(want[j].numerator) / want[j].denominator * k
            assert abs(got - ref) <= REL * (abs(ref) + 1e-300) * 8
    x = 2.0 ** 21 + rs.randn(ns, D) * 2.0 ** -13
    c = 2.0 ** 21 + rs.randn(ns, s, D) * 2.0 ** -13
    q, wf = hp.walk_s_proposal(x, c, z)
    for t in range(ns):
        for d in range(D):
            ref = sum((mpmath.mpf(w[0][t, j]) + mpmath.mpf(w[1][t, j])) * (mpmath.mpf(c[t, j, d]) - mpmath.mpf(x[t, d]))
                      for j in range(s)) + mpmath.mpf(x[t, d])
            assert q[t, d] == float(ref)                  # correctly rounded: the reference is 2^-100 from it


@pytest.mark.parametrize("N,D,offset", [(40, 1, 0.0), (57, 3, 0.0), (200, 8, 1e6), (31, 30, 0.0)])
def test_complement_stats_against_np_cov(N, D, offset):
    rs = np.random.RandomState(N)
    x = offset + rs.randn(N, D) @ (np.eye(D) + 0.3 * rs.randn(D, D))
    mu, S = hp.complement_stats(x)
    np.testing.assert_allclose(hp.to_float(mu), x.mean(0), rtol=1e-14, atol=1e-14 * np.abs(x).max())
    ref = np.atleast_2d(np.cov(x, rowvar=False))
    np.testing.assert_allclose(hp.to_float(S), ref, rtol=1e-9, atol=1e-12 * np.abs(ref).max())
    # exactly: Fraction covariance on one small case
    if N == 57:
        xs = [[F(v) for v in row] for row in x]
        m = [sum(r[d] for r in xs) / N for d in range(D)]
        for i in range(D):
            for j in range(D):
                want = sum((r[i] - m[i]) * (r[j] - m[j]) for r in xs) / (N - 1)
                assert abs(ddF(S, (i, j)) - want) <= 2.0 ** -95 * sum(abs((r[i] - m[i]) * (r[j] - m[j])) for r in xs) / (N - 1)
    L = hp.cholesky(S, semidefinite=False)
    np.testing.assert_allclose(hp.to_float(L), np.linalg.cholesky(ref), rtol=1e-9, atol=1e-12 * np.sqrt(np.abs(ref).max()))


def test_cholesky_rules():
    rs = np.random.RandomState(6)
    x = rs.randn(50, 3)
    x[:, 1] = 0.75                                        # constant coordinate
    _, S = hp.complement_stats(x)
    with pytest.raises(np.linalg.LinAlgError):
        hp.cholesky(S, semidefinite=False)
    L = hp.to_float(hp.cholesky(S, semidefinite=True))
    assert np.all(L[:, 1] == 0) and np.all(L[1, :] == 0) and L[2, 2] > 0
    x = rs.randn(50, 3) * np.array([1e4, 1.0, 1e-4])
    x[:, 1] = 2 * x[:, 0]                                 # exactly collinear: column 1 zeroed, scale-invariant threshold keeps col 2
    _, S = hp.complement_stats(x)
    L = hp.to_float(hp.cholesky(S, semidefinite=True))
    assert np.all(L[:, 1] == 0) and L[2, 2] > 0 and L[2, 2] < 1e-3


@pytest.mark.parametrize("rule,bw", [(0, None), (1, "silverman"), (2, 0.05), (2, 3.0)])
def test_kde_bandwidth_and_log_ratio_against_scipy(rule, bw):
    rs = np.random.RandomState(7)
    Nc, D, n = 90, 4, 25
    C = rs.randn(Nc, D) @ (np.eye(D) + 0.3 * rs.randn(D, D)) + 0.5
    dens = gaussian_kde(C.T, bw_method=bw)
    h = hp.kde_bandwidth(rule, Nc, D, bw or 0.0)
    mpmath.mp.prec = 200
    if rule < 2:
        a = mpmath.mpf(Nc) * (D + 2) / 4 if rule == 1 else mpmath.mpf(Nc)
        want = a ** (-mpmath.mpf(1) / (D + 4))
        assert abs(mpmath.mpf(h[0]) + mpmath.mpf(h[1]) - want) <= REL * want
    assert abs(hp.to_float(h) - dens.factor) <= 1e-15 * dens.factor
    mu, S = hp.complement_stats(C)
    Lh = hp.mul(hp.cholesky(S, semidefinite=False), (np.full((D, D), h[0]), np.full((D, D), h[1])))
    np.testing.assert_allclose(hp.to_float(Lh), np.linalg.cholesky(dens.covariance), rtol=1e-10, atol=1e-13)
    s_rows = rs.randn(n, D)
    k = rs.randint(0, Nc, n)
    z = rs.randn(n, D)
    q = hp.linear_proposal(C[k], Lh, z)
    f, R = hp.kde_log_ratio(mu, Lh, C, s_rows, k, z)
    want = dens.logpdf(s_rows.T) - dens.logpdf(q.T)
    np.testing.assert_allclose(f, want, rtol=0, atol=1e-9)
    assert R > 0


# ---- the built-in log-probabilities (hp.*_logprob, lp_families): references against mpmath, and what the bounds detect ---------------
import lp_families as lpf  # noqa: E402

LP_CASES = [(k, f) for f in sorted(lpf.FAMILIES) for k in lpf.FAMILIES[f]]


def _mp_logprob(t, row):
    mp = mpmath.mpf
    D, kind = t["D"], t["kind"]
    if kind == "iso":
        return -sum(mp(v) ** 2 for v in row) / 2
    if kind == "diag":
        return -sum(mp(t["ivar"][d]) * (mp(row[d]) - mp(t["mu"][d])) ** 2 for d in range(D)) / 2
    if kind == "dense":
        r = [mp(row[d]) - mp(t["mu"][d]) for d in range(D)]
        A = t["icov"]
        return -sum(r[i] * (mp(A[i, j]) + mp(A[j, i])) / 2 * r[j] for i in range(D) for j in range(D)) / 2
    return -sum(100 * (mp(row[d + 1]) - mp(row[d]) ** 2) ** 2 + (1 - mp(row[d])) ** 2 for d in range(D - 1)) / mp(t["scale"])


@pytest.mark.parametrize("D", [1, 2, 5, 17])
@pytest.mark.parametrize("kind,family", LP_CASES)
def test_logprob_references_against_mpmath(kind, family, D):
    """300 bits: the reference's own error is at most 1 % of the bound it is paired with"""
    mpmath.mp.prec = 300
    t = lpf.make(kind, family, D, 6)
    ref, bound, refdd = lpf.reference(t, t["x"])
    if kind == "box":
        want = np.where(np.any((t["x"] > 1) | (t["x"] < 0), axis=1), -np.inf, 0.0)
        assert np.array_equal(ref, want) and not np.all(np.isfinite(want)) and np.any(want == 0)
        return
    for i in range(len(ref)):
        want = _mp_logprob(t, t["x"][i])
        got = mpmath.mpf(refdd[0][i]) + mpmath.mpf(refdd[1][i])
        assert abs(got - want) <= mpmath.mpf(0.01 * bound[i]), (i, float(abs(got - want)), bound[i])
        assert bound[i] > 0 or (kind == "rosenbrock" and D == 1 and got == 0)
        if family not in ("illcond", "valley"):           # (there the bound is honestly far above eps |lp|: r L cancels, a1 does)
            assert bound[i] <= 1e-12 * abs(float(want))
    if kind == "dense" and family == "illcond" and D > 1:
        ev = np.linalg.eigvalsh(t["corr"])
        assert np.allclose(np.diag(t["corr"]), 1.0) and ev[0] > 0 and 1e9 <= ev[-1] / ev[0] <= 1e11
    if kind == "dense":                                     # the factorised form against the term-by-term one
        d2 = hp.dense_logprob_direct(t["x"], t["mu"], t["icov"])
        assert np.all(np.abs(hp.to_float(hp.sub(refdd, d2))) <= 0.01 * bound)


def test_offset_does_not_loosen_a_bound():
    """the same differences next to a mean of 0 and of 2^21 (the draws are on the grid of the large mean): the same bound"""
    for kind in ("diag", "dense"):
        t = lpf.make(kind, "offset", 5, 8)
        near = dict(t, mu=t["mu"] - 2.0 ** 21)
        b0 = lpf.reference(t, t["x"])[1]
        b1 = lpf.reference(near, t["x"] - 2.0 ** 21)[1]
        assert np.array_equal(b0, b1)


def _twin_dense(t, x, mistake=None):
    """the kernels' arithmetic in host float64: r = x - mu, y = r L, -1/2 sum y^2 -- or one plausible mistake"""
    icov = t["icov"]
    A = 0.5 * (icov + icov.T)
    if mistake == "lower":
        A = np.tril(icov) + np.tril(icov, -1).T
    L = np.linalg.cholesky(A)
    if mistake == "folded":
        y = x @ L - t["mu"] @ L
    elif mistake == "f32":
        r = x - t["mu"]
        y = np.sum((r[:, :, None] * L[None]).astype(np.float32), axis=1, dtype=np.float32).astype(np.float64)
    else:
        y = (x - t["mu"]) @ L
    return -0.5 * np.sum(y * y, axis=1)


def _twin_rosen(t, x, mistake=None):
    sq = x[:, :-1] * x[:, :-1]
    if mistake == "f32":
        sq = sq.astype(np.float32).astype(np.float64)
    a1, b1 = x[:, 1:] - sq, 1.0 - x[:, :-1]
    return -np.sum(100.0 * a1 * a1 + b1 * b1, axis=1) / t["scale"]


@pytest.mark.parametrize("kind,family,mistake", [("dense", "offset", "folded"), ("dense", "benign", "f32"), ("dense", "asym", "lower"),
                                                 ("rosenbrock", "valley", "f32")])
@pytest.mark.parametrize("D", [5, 17])
def test_bounds_catch_plausible_kernel_mistakes(kind, family, mistake, D):
    """a host float64 twin with the mistake exceeds the bound by a factor of 100 at least; the correct twin stays inside it"""
    t = lpf.make(kind, family, D, 64)
    twin = _twin_dense if kind == "dense" else _twin_rosen
    good = lpf.ratio(twin(t, t["x"]), t, t["x"])
    bad = lpf.ratio(twin(t, t["x"], mistake), t, t["x"])
    assert good.max() <= 1.0, good.max()
    assert bad.max() >= 100.0, bad.max()
    assert np.median(bad) >= 100.0, np.median(bad)


@pytest.mark.parametrize("kind,family", LP_CASES)
def test_correct_float64_twins_stay_inside_their_bounds(kind, family):
    for D in (1, 2, 5, 17, 33):
        t = lpf.make(kind, family, D, 40)
        x = t["x"]
        if kind == "dense":
            got = _twin_dense(t, x)
        elif kind == "rosenbrock":
            got = _twin_rosen(t, x)
        elif kind == "diag":
            r = x - t["mu"]
            got = -0.5 * np.sum(t["ivar"] * r * r, axis=1)
        elif kind == "iso":
            got = -0.5 * np.sum(x * x, axis=1)
        else:
            got = hp.box_logprob(x)
        assert lpf.ratio(got, t, x).max() <= 1.0, D
