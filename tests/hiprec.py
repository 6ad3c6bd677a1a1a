"""Double-double reference arithmetic for the device WalkMove / KDEMove proposals (csrc/emx_walkkde.hip) and for the built-in
log-probabilities (every kernel that evaluates one: tests/test_gpu_logprob_reference.py), test-side only.

A double-double value is a pair (hi, lo) of float64 arrays, hi = fl(hi + lo), carrying about 106 significant bits.  Everything is
built on two error-free transformations: Knuth's TwoSum and Dekker's TwoProduct with Veltkamp's split.  No fused multiply-add is
used, so every result is the same on any IEEE-754 host.  TwoProduct is exact while |a b| >= 2^-968 (the error term and the split
products stay normal) and |a|, |b| < 2^1023; inputs above 2^996 are split after a scaling by 2^-28, so the split cannot overflow.

On top of that, the references the GPU tests compare against:
  * walk_s_proposal: WalkMove(s >= 2), q = x + sum_k w_k (c_k - x), w_k = (z_k - mean z) / sqrt(s - 1) from the exact normals;
  * complement_stats / cholesky: the centred two-pass mean and covariance (ddof 1, np.cov) and its Cholesky factor, with the
    device's rule for the whole-complement walk (a pivot <= 1e-12 S_jj zeroes column j) or scipy's (a pivot <= 0 is singular);
  * linear_proposal: q = base + L z (whole-complement walk, KDE);
  * kde_bandwidth / kde_log_ratio: gaussian_kde's bandwidth factor and logpdf(s) - logpdf(q) from direct whitened distances
    |y - Y_j|^2, then a log-sum-exp.  Only that last exp / log is float64: its absolute error is a few ulps of 1.
The inputs are the device's plan (DeviceEnsemble.plan_get) and the host twin of its draws (emx_host_walk_kde_draws).
  * iso_logprob / diag_logprob / dense_logprob / rosenbrock_logprob / box_logprob: the built-in targets on rows x (n, D), each with
    the running-error quantity its forward-error bound is made of (tests/lp_families.py holds the bounds and their derivations)."""
import numpy as np

_SPLITTER = 134217729.0             # 2^27 + 1
_SPLIT_BIG = 2.0 ** 996


# ---- error-free transformations ---------------------------------------------------------------------------------------------
def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fast_two_sum(a, b):
    """|a| >= |b| (or a == 0)"""
    s = a + b
    return s, b - (s - a)


def split(a):
    a = np.asarray(a, dtype=np.float64)
    big = np.abs(a) > _SPLIT_BIG
    a_s = np.where(big, a * 2.0 ** -28, a)
    c = _SPLITTER * a_s
    hi = c - (c - a_s)
    lo = a_s - hi
    return np.where(big, hi * 2.0 ** 28, hi), np.where(big, lo * 2.0 ** 28, lo)


def two_prod(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    p = a * b
    ah, al = split(a)
    bh, bl = split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


# ---- double-double operations: x = (xh, xl) -----------------------------------------------------------------------------------
def dd(a):
    a = np.asarray(a, dtype=np.float64)
    return a, np.zeros_like(a)


def neg(x):
    return -x[0], -x[1]


def add(x, y):
    s, e = two_sum(x[0], y[0])
    t, f = two_sum(x[1], y[1])
    s, e = fast_two_sum(s, e + t)
    return fast_two_sum(s, e + f)


def sub(x, y):
    return add(x, neg(y))


def mul(x, y):
    p, e = two_prod(x[0], y[0])
    return fast_two_sum(p, e + (x[0] * y[1] + x[1] * y[0]))


def mul_d(x, b):
    p, e = two_prod(x[0], b)
    return fast_two_sum(p, e + x[1] * b)


def div(x, y):
    q1 = x[0] / y[0]
    r = sub(x, mul_d(y, q1))
    q2 = r[0] / y[0]
    r = sub(r, mul_d(y, q2))
    q3 = r[0] / y[0]
    return add(fast_two_sum(q1, q2), dd(q3))


def sqrt(x):
    s = np.sqrt(np.maximum(x[0], 0.0))
    r = sub(x, two_prod(s, s))
    safe = np.where(s > 0, 2.0 * s, 1.0)
    return fast_two_sum(s, np.where(s > 0, r[0] / safe, 0.0))


def dsum(x, axis=0):
    """pairwise double-double sum along `axis`"""
    h, l = np.moveaxis(x[0], axis, 0), np.moveaxis(x[1], axis, 0)
    if h.shape[0] == 0:
        return np.zeros(h.shape[1:]), np.zeros(h.shape[1:])
    while h.shape[0] > 1:
        n = h.shape[0] // 2
        a = add((h[:n], l[:n]), (h[n:2 * n], l[n:2 * n]))
        if h.shape[0] % 2:
            h, l = np.concatenate([a[0], h[2 * n:]]), np.concatenate([a[1], l[2 * n:]])
        else:
            h, l = a
    return h[0], l[0]


def rowdot(x, y):
    """row-wise dot product of two double-double arrays (n, D) -> (n,) double-double"""
    return dsum(mul(x, y), axis=1)


def to_float(x):
    return x[0] + x[1]


def take(x, idx, axis=0):
    return np.take(x[0], idx, axis=axis), np.take(x[1], idx, axis=axis)


# ---- references ------------------------------------------------------------------------------------------------------------------
def walk_weights(z):
    """(ns, s) normals -> the exact weights (z - mean z) / sqrt(s - 1) as double-double"""
    s = z.shape[1]
    zbar = div(dsum(dd(z), axis=1), dd(np.full(z.shape[0], float(s))))
    rs = div(dd(1.0), sqrt(dd(float(s - 1))))
    return mul(sub(dd(z), (zbar[0][:, None], zbar[1][:, None])), rs)


def walk_s_proposal(x, c, z):
    """x (ns, D) current positions, c (ns, s, D) the helpers' positions, z (ns, s) normals -> (q (ns, D), w (ns, s) as float)"""
    w = walk_weights(z)
    d = two_sum(c, -x[:, None, :])                    # c - x, exact
    dq = dsum(mul((w[0][:, :, None], w[1][:, :, None]), d), axis=1)
    return to_float(add(dd(x), dq)), to_float(w)


def complement_stats(C):
    """(Nc, D) rows -> (mean, covariance with ddof 1), both double-double, the covariance from the centred rows"""
    Nc, D = C.shape
    mu = div(dsum(dd(C), axis=0), dd(np.full(D, float(Nc))))
    d = sub(dd(C), (mu[0][None, :], mu[1][None, :]))
    S = dd(np.zeros((D, D)))
    R = max(1, (1 << 20) // (D * D))
    for r0 in range(0, Nc, R):
        a = (d[0][r0:r0 + R], d[1][r0:r0 + R])
        p = mul((a[0][:, :, None], a[1][:, :, None]), (a[0][:, None, :], a[1][:, None, :]))
        S = add(S, dsum(p, axis=0))
    return mu, div(S, dd(np.full((D, D), float(Nc - 1))))


def cholesky(S, semidefinite):
    """lower Cholesky factor of the double-double matrix S.  semidefinite (the whole-complement walk): a pivot <= 1e-12 S_jj (the
    diagonal before the factorisation) zeroes column j.  Otherwise (KDE, scipy): a pivot <= 0 raises LinAlgError."""
    D = S[0].shape[0]
    A = (S[0].copy(), S[1].copy())
    tol = 1e-12 * np.diag(S[0])
    L = dd(np.zeros((D, D)))
    for j in range(D):
        piv = (A[0][j, j], A[1][j, j])
        if semidefinite:
            zero = not (sub(piv, dd(tol[j]))[0] > 0)
        else:
            if not (piv[0] > 0):
                raise np.linalg.LinAlgError("reference: covariance is not positive definite (pivot %d)" % j)
            zero = False
        if zero:
            continue
        ljj = sqrt((np.array([piv[0]]), np.array([piv[1]])))
        col = div((A[0][j:, j], A[1][j:, j]), (np.full(D - j, ljj[0][0]), np.full(D - j, ljj[1][0])))
        col[0][0], col[1][0] = ljj[0][0], ljj[1][0]
        L[0][j:, j], L[1][j:, j] = col
        c1 = (col[0][1:], col[1][1:])
        upd = mul((c1[0][:, None], c1[1][:, None]), (c1[0][None, :], c1[1][None, :]))
        t = sub((A[0][j + 1:, j + 1:], A[1][j + 1:, j + 1:]), upd)
        A[0][j + 1:, j + 1:], A[1][j + 1:, j + 1:] = t
    return L


def matvec(L, z):
    """rows of z (n, D) -> L z as double-double (n, D)"""
    n, D = z.shape
    out = dd(np.zeros((n, D)))
    R = max(1, (1 << 20) // (D * D))
    for r0 in range(0, n, R):
        zz = dd(z[r0:r0 + R][:, None, :])
        p = dsum(mul((L[0][None], L[1][None]), zz), axis=2)
        out[0][r0:r0 + R], out[1][r0:r0 + R] = p
    return out


def linear_proposal(base, L, z):
    """q = base + L z: the whole-complement walk (base = x) and KDE (base = the drawn complement row)"""
    return to_float(add(dd(base), matvec(L, z)))


def _power(x, m):
    r, b = dd(1.0), x
    while m:
        if m & 1:
            r = mul(r, b)
        b = mul(b, b)
        m >>= 1
    return r


def kde_bandwidth(rule, Nc, D, bw=0.0):
    """gaussian_kde's factor: 0 Scott n^(-1/(d+4)), 1 Silverman (n (d+2) / 4)^(-1/(d+4)), 2 the scalar bw.  The root a^(-1/m) is
    one Newton step on h^m a - 1 = 0 from float64's pow, with the residual in double-double."""
    if rule == 2:
        return dd(float(bw))
    m = D + 4
    a = div(dd(float(Nc) * (D + 2)), dd(4.0)) if rule == 1 else dd(float(Nc))
    h = dd(float(a[0] + a[1]) ** (-1.0 / m))
    for _ in range(2):
        P = mul(a, _power(h, m))
        r = sub(P, dd(1.0))
        h = sub(h, dd(r[0] * h[0] / (m * P[0])))
    return h


def forward_solve(L, V):
    """rows of V (n, D), double-double -> rows of L^-1 V"""
    n, D = V[0].shape
    Y = dd(np.zeros((n, D)))
    for i in range(D):
        t = (V[0][:, i], V[1][:, i])
        if i:
            p = mul((Y[0][:, :i], Y[1][:, :i]), (L[0][i, :i][None, :], L[1][i, :i][None, :]))
            t = sub(t, dsum(p, axis=1))
        y = div(t, (np.full(n, L[0][i, i]), np.full(n, L[1][i, i])))
        Y[0][:, i], Y[1][:, i] = y
    return Y


def _lse_neg_half_sq(yq, YC):
    """for each query row of yq (double-double): LSE_j(-|yq - YC_j|^2 / 2) from direct differences"""
    nq, D = yq[0].shape
    Nc = YC[0].shape[0]
    out = np.empty(nq)
    R = max(1, (1 << 21) // max(1, Nc * D))
    for r0 in range(0, nq, R):
        a = (yq[0][r0:r0 + R][:, None, :], yq[1][r0:r0 + R][:, None, :])
        d = sub(a, (YC[0][None], YC[1][None]))
        t = mul_d(dsum(mul(d, d), axis=2), -0.5)             # (R, Nc)
        m = t[0].max(axis=1)
        e = to_float(sub(t, dd(m[:, None])))
        out[r0:r0 + R] = m + np.log(np.sum(np.exp(e), axis=1))
    return out


def kde_log_ratio(mu, Lh, C, s_rows, k, z):
    """logpdf(s) - logpdf(q) of gaussian_kde(C) with factor Lh (the bandwidth-scaled Cholesky factor, double-double).
    s_rows (n, D): the current positions; k (n,): complement ranks of the drawn centres; z (n, D) their normals, so the
    proposal's whitened position is Y_C[k] + z exactly (the device's q is that point rounded).
    -> (factor (n,), R: the largest whitened norm involved)"""
    mu2 = (mu[0][None, :], mu[1][None, :])
    YC = forward_solve(Lh, sub(dd(C), mu2))
    ys = forward_solve(Lh, sub(dd(s_rows), mu2))
    yq = add(take(YC, k), dd(z))
    f = _lse_neg_half_sq(ys, YC) - _lse_neg_half_sq(yq, YC)
    R = max(np.sqrt(np.max(np.sum(to_float(Y) ** 2, axis=1))) for Y in (YC, ys, yq))
    return f, R


# ---- the built-in log-probabilities ---------------------------------------------------------------------------------------------
def dabs(x):
    neg_ = x[0] < 0
    return np.where(neg_, -x[0], x[0]), np.where(neg_, -x[1], x[1])


def iso_logprob(x):
    """-1/2 sum x_d^2 on rows x (n, D) -> (log-prob (n,) double-double, M = sum x_d^2 (n,) float)"""
    s = dsum(two_prod(x, x), axis=1)
    return mul_d(s, -0.5), to_float(s)


def diag_logprob(x, mu, ivar):
    """-1/2 sum ivar_d (x_d - mu_d)^2 -> (log-prob double-double, M = sum |ivar_d| (x_d - mu_d)^2 float)"""
    x = np.asarray(x, dtype=np.float64)
    r = two_sum(x, -np.asarray(mu, dtype=np.float64)[None, :])               # exact
    t = mul_d(mul(r, r), np.asarray(ivar, dtype=np.float64)[None, :])
    return mul_d(dsum(t, axis=1), -0.5), to_float(dsum(dabs(t), axis=1))


def sym(icov):
    """(icov + icov^T) / 2 as double-double (the halving is exact)"""
    icov = np.asarray(icov, dtype=np.float64)
    a = two_sum(icov, icov.T)
    return a[0] * 0.5, a[1] * 0.5


def dense_factor(icov):
    """-> the lower Cholesky factor L of A = (icov + icov^T) / 2, double-double: A = L L^T"""
    return cholesky(sym(icov), semidefinite=False)


def rowvec_lower(r, L):
    """rows r (n, D), L lower triangular (D, D), both double-double -> y_n = sum_{k >= n} r_k L_kn, (n, D) double-double"""
    n, D = r[0].shape
    y = dd(np.zeros((n, D)))
    for k in range(D):
        p = mul((r[0][:, k:k + 1], r[1][:, k:k + 1]), (L[0][k, :k + 1][None, :], L[1][k, :k + 1][None, :]))
        t = add((y[0][:, :k + 1], y[1][:, :k + 1]), p)
        y[0][:, :k + 1], y[1][:, :k + 1] = t
    return y


def dense_logprob(x, mu, icov, L=None):
    """-1/2 r^T A r, A = (icov + icov^T) / 2, r = x - mu (exact), evaluated as -1/2 |r L|^2 with the double-double Cholesky factor L
    of A (dense_factor; it may be handed in): L L^T = A to D 2^-104 |L||L^T|, far below anything float64 can see.
    -> (log-prob (n,) double-double, S = sum_n a_n^2 with a_n = sum_k |r_k| |L_kn| (n,) float)"""
    x = np.asarray(x, dtype=np.float64)
    if L is None:
        L = dense_factor(icov)
    r = two_sum(x, -np.asarray(mu, dtype=np.float64)[None, :])
    y = rowvec_lower(r, L)
    a = np.abs(to_float(r)) @ np.abs(to_float(L))
    return mul_d(dsum(mul(y, y), axis=1), -0.5), np.sum(a * a, axis=1)


def dense_logprob_direct(x, mu, icov):
    """-1/2 sum_ij r_i A_ij r_j term by term (no factorisation): the check of dense_logprob on small cases"""
    x = np.asarray(x, dtype=np.float64)
    A = sym(icov)
    r = two_sum(x, -np.asarray(mu, dtype=np.float64)[None, :])
    t = mul(mul((r[0][:, :, None], r[1][:, :, None]), (A[0][None], A[1][None])), (r[0][:, None, :], r[1][:, None, :]))
    return mul_d(dsum(dsum(t, axis=2), axis=1), -0.5)


def rosenbrock_logprob(x, scale):
    """-(sum_{d < D-1} 100 (x_{d+1} - x_d^2)^2 + (1 - x_d)^2) / scale
    -> (log-prob (n,) double-double, |a1| (n, D-1), x_d^2 (n, D-1), |b1| (n, D-1) floats; a1 = x_{d+1} - x_d^2, b1 = 1 - x_d)"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    sq = two_prod(x[:, :-1], x[:, :-1])                                   # exact
    a1 = sub(dd(x[:, 1:]), sq)
    b1 = two_sum(np.ones_like(x[:, :-1]), -x[:, :-1])                       # exact
    t = add(mul_d(mul(a1, a1), 100.0), mul(b1, b1))
    s = dsum(t, axis=1)
    lp = neg(div(s, dd(np.full(n, float(scale)))))
    return lp, np.abs(to_float(a1)), sq[0], np.abs(to_float(b1))


def box_logprob(x):
    """0 inside [0, 1]^D, -inf outside (exact)"""
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.any((x > 1.0) | (x < 0.0), axis=1), -np.inf, 0.0)
