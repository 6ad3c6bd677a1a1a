"""The built-in log-probabilities against tests/hiprec.py: forward-error bounds, derived, and the seeded input families, shared by
tests/test_hiprec_cpu.py (the references against mpmath, the negative controls) and tests/test_gpu_logprob_reference.py.

u = 2^-53 is the unit roundoff, EPS = 2u, gamma_k = k u / (1 - k u).  Every bound is a multiple of a running-error quantity that the
reference computes from the DIFFERENCES the arithmetic works on -- never of the coordinates' magnitude: an offset of 2^21 in x and mu
changes none of them.

iso / diag:  |lp - ref| <= (D + 4) u M,  M = sum_d |ivar_d| r_d^2  (= 2 |ref| for ivar > 0; iso: ivar = 1, r = x).
  fl(r_d) = r_d (1 + d1) enters squared: 2u.  fl(ivar_d r_d): u.  The products enter the sum through an fma, whose rounding belongs to
  the sum: a term passes through at most D roundings, in any order (a padded lane adds an exact zero).  gamma_(D+3) M <= (D + 4) u M.

dense:  |lp - ref| <= C_DENSE EPS (D + 8) S,  S = sum_n a_n^2, a_n = sum_k |r_k| |L_kn|, A = sym(icov) = L L^T.
  The kernels compute y = fl(r) Lh (f64 fma chains, any order; Lh the host's float64 Cholesky factor of fl(sym(icov))), then
  -1/2 sum y_n^2.
    fl(r) = r (1 + d): y_n moves by u a_n; the chain of D fmas adds gamma_D a_n: |yh_n - y_n| <= gamma_(D+1) a_n, and |y_n| <= a_n, so
      1/2 sum |yh_n^2 - y_n^2| <= gamma_(D+1) S                                             (D + 1) u S
    squares summed through fmas, D non-zero terms:  1/2 gamma_(D+1) sum y_n^2 <=              (D + 1) u S / 2
    the host's Cholesky: Lh Lh^T = Ah + E, |E| <= gamma_(D+1) |Lh||Lh^T|: 1/2 |r^T E r| <=    (D + 1) u S / 2
    fl((icov_ij + icov_ji) / 2) = A_ij (1 + d), |A| <= |L||L^T|:  1/2 u |r|^T |A| |r| <=      u S / 2
  together (2 D + 2.5) u S = (D + 1.25) EPS S: C_DENSE = 1, and (D + 8) leaves room for the second-order terms and for S being
  taken with the reference's L where the kernel's error grows with |Lh| (the two differ by D u kappa, relatively).
C_DENSE = 1

rosenbrock:  |lp - ref| <= C_ROSEN (D + 2) EPS T / scale,  T = sum_d 200 |a1| x_d^2 + 100 a1^2 + b1^2 + 100 u (x_d^2 + |a1|)^2.
  a1 = x_(d+1) - x_d^2 with x_d^2 rounded first (or not, when the compiler contracts it): |da1| <= e = u (x_d^2 + |a1|).
  100 a1^2 is fl(100 a1h) a1h inside an fma: off by 100 (2 |a1| e + e^2) + 100 u a1^2 = u (200 |a1| x_d^2 + 300 a1^2) + 100 e^2;
  b1 = fl(1 - x_d): b1^2 off by 2 u b1^2.  The 2 (D - 1) products pass through at most 2 (D - 1) roundings of the sum, the division
  by the scale adds one: (2 D - 1) u (100 a1^2 + b1^2).  Term by term that is at most (2 D + 2) u of T's first three terms, plus
  100 e^2 = 100 u^2 (x_d^2 + |a1|)^2, which is T's last term times u (it matters only where |a1| < u x_d^2, on the valley's floor):
  (2 D + 4) u T = (D + 2) EPS T with the second-order terms.  C_ROSEN = 1.  T does not scale with |lp|: on the valley
  (|a1| ~ 1e-9 x_d^2) the first term is 2e9 times 100 a1^2.

box: exact."""
import hashlib

import numpy as np

import hiprec as hp

U = 2.0 ** -53
EPS = 2.0 * U
C_DENSE = 1.0
C_ROSEN = 1.0
KINDS = ("iso", "diag", "dense", "rosenbrock", "box")
# family -> the target kinds it applies to
FAMILIES = {"benign": KINDS, "offset": ("diag", "dense"), "illcond": ("dense",), "asym": ("dense",), "valley": ("rosenbrock",),
            "scaled": ("diag", "dense")}
ROSEN_SCALE = 20.0


def _seed(kind, family, D):
    return 1000003 * KINDS.index(kind) + 7919 * sorted(FAMILIES).index(family) + D


def _pow2_scales(D, rs):
    return 2.0 ** rs.randint(-24, 25, D)


def _cov_benign(D, rs):
    A = rs.randn(D, D)
    return A @ A.T / D + 0.1 * np.eye(D)


def valley_rows(n, D, rs):
    """x_(d+1) = x_d^2 (1 + 1e-9 randn) while 1e-3 <= x_d^2 <= 30; a coordinate that would leave that range starts afresh"""
    x = np.empty((n, D))
    fresh = lambda m: rs.uniform(0.5, 5.4, m) * rs.choice([-1.0, 1.0], m)
    x[:, 0] = fresh(n)
    for d in range(1, D):
        sq = x[:, d - 1] ** 2
        nxt = sq * (1.0 + 1e-9 * rs.randn(n))
        ok = (sq >= 1e-3) & (sq <= 30.0)
        x[:, d] = np.where(ok, nxt, fresh(n))
    return x


def make(kind, family, D, n, seed=None):
    """-> dict(kind, D, x (n, D) rows drawn from (or near) the target, and the target's parameters: mu, ivar | icov, chol_cov, scale)"""
    assert kind in FAMILIES[family], (kind, family)
    rs = np.random.RandomState(_seed(kind, family, D) if seed is None else seed)
    t = dict(kind=kind, family=family, D=D)
    if kind == "iso":
        t["x"] = rs.randn(n, D)
    elif kind == "box":
        t["x"] = rs.randn(n, D) * 0.6 + 0.5
        t["x"][: n // 3] = rs.rand(n // 3, D)
        if n > 3:
            t["x"][0, 0], t["x"][1, D - 1], t["x"][2, 0] = 1.0, 0.0, np.nextafter(1.0, 2.0)           # the closed edges, and just outside
    elif kind == "rosenbrock":
        t["scale"] = ROSEN_SCALE
        if family == "valley":
            t["x"] = valley_rows(n, D, rs)
        else:
            t["x"] = rs.randn(n, D)
            if D > 1:
                t["x"][:, 1:] = t["x"][:, :-1] ** 2 + 0.3 * rs.randn(n, D - 1)
    elif kind == "diag":
        if family == "offset":
            mu, ivar = 2.0 ** 21 + rs.rand(D), 2.0 ** 26 * rs.uniform(0.5, 2.0, D)
        else:
            mu, ivar = rs.randn(D), 1.0 / (0.1 + rs.rand(D))
        x = mu + rs.randn(n, D) / np.sqrt(ivar)
        if family == "scaled":
            sc = _pow2_scales(D, rs)
            mu, ivar, x = mu * sc, ivar / (sc * sc), x * sc
        t.update(mu=mu, ivar=ivar, x=x, sd=1.0 / np.sqrt(ivar))
    else:
        if family == "illcond":
            # the eigenvalues of the covariance run from 1 down to 1e-10; scaled to a unit diagonal it is the correlation matrix
            Q = np.linalg.qr(rs.randn(D, D))[0]
            lam = np.logspace(0.0, -10.0, D) if D > 1 else np.ones(1)
            s = np.sqrt(np.sum(Q * Q * lam[None, :], axis=1))
            icov = ((Q * (1.0 / lam)[None, :]) @ Q.T) * np.outer(s, s)
            icov = 0.5 * (icov + icov.T)
            Lc = (Q * np.sqrt(lam)[None, :]) / s[:, None]                   # cov = Lc Lc^T
            mu = rs.randn(D)
            t["corr"] = Lc @ Lc.T
        else:
            cov = _cov_benign(D, rs)
            mu = rs.randn(D)
            if family == "offset":
                mu, cov = 2.0 ** 21 + rs.rand(D), cov * 2.0 ** -26
            icov = np.linalg.inv(cov)
            icov = 0.5 * (icov + icov.T)
            Lc = np.linalg.cholesky(cov)
        x = mu + rs.randn(n, D) @ Lc.T
        if family == "asym":
            dg = np.sqrt(np.diag(icov))
            icov = icov + np.triu(1e-9 * np.outer(dg, dg) * rs.randn(D, D), 1)
        if family == "scaled":
            sc = _pow2_scales(D, rs)
            mu, icov, x, Lc = mu * sc, icov / np.outer(sc, sc), x * sc, Lc * sc[:, None]
        t.update(mu=mu, icov=icov, x=x, chol_cov=Lc)
    return t


_FACTORS = {}


def _factor(t):
    key = hashlib.sha1(np.ascontiguousarray(t["icov"]).tobytes()).hexdigest()
    if key not in _FACTORS:
        _FACTORS[key] = hp.dense_factor(t["icov"])
    return _FACTORS[key]


def reference(t, x):
    """rows x (n, D) of target t -> (reference log-prob (n,) float64, its bound (n,), the reference as double-double)"""
    kind, D = t["kind"], t["D"]
    x = np.ascontiguousarray(x, dtype=np.float64)
    if kind == "box":
        lp = hp.box_logprob(x)
        return lp, np.zeros(len(x)), (lp, np.zeros(len(x)))
    if kind == "iso":
        lp, M = hp.iso_logprob(x)
        bound = (D + 4) * U * M
    elif kind == "diag":
        lp, M = hp.diag_logprob(x, t["mu"], t["ivar"])
        bound = (D + 4) * U * M
    elif kind == "dense":
        lp, S = hp.dense_logprob(x, t["mu"], t["icov"], _factor(t))
        bound = C_DENSE * EPS * (D + 8) * S
    else:
        lp, a1, sq, b1 = hp.rosenbrock_logprob(x, t["scale"])
        T = np.sum(200.0 * a1 * sq + 100.0 * a1 * a1 + b1 * b1 + 100.0 * U * (sq + a1) ** 2, axis=1)
        bound = C_ROSEN * (D + 2) * EPS * T / t["scale"]
    return hp.to_float(lp), bound, lp


def ratio(got, t, x):
    """-> error / bound per row (0 where both vanish), after checking that non-finite values agree exactly"""
    ref, bound, refdd = reference(t, x)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin]), "non-finite log-probs differ from the reference"
    assert np.all(np.isfinite(got[fin])), "a log-prob is not finite where the reference is"
    err = np.abs(hp.to_float(hp.sub(hp.dd(got[fin]), (refdd[0][fin], refdd[1][fin]))))
    out = np.zeros(len(ref))
    out[fin] = np.where(err == 0, 0.0, err / np.maximum(bound[fin], 1e-300))
    return out
