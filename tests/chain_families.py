"""Chains far from the origin: the seeded target families and the exact references that the chain-analysis kernels (summaries,
histograms, autocorrelation) are held to, shared by tests/test_chain_families_cpu.py (the references against fractions.Fraction,
the negative control) and tests/test_gpu_chain_offset_reference.py.

A posterior of times, epochs or frequencies sits at |mean| / sd of 2^20 ... 2^40.  There NumPy's own mean and covariance lose the
digits the device loses, so they cannot be the reference.  What can: for |mu| >> sd the subtraction x - mu is exact (Sterbenz), so
the recentred copy r = x - mu holds the same numbers as x, shifted, and at unit scale NumPy is accurate again:
  mean(x) = mean(r) + mu          exactly; mean(r) from math.fsum
  cov(x)  = cov(r)                exactly; np.cov(r) is within n u sd_j sd_k of it (a dot product of n terms)
  acf(x)  = acf(r)                exactly; autocorr._batched_acf(r)
recentre() asserts (x - mu) + mu == x bit for bit, which is what makes r the same data.

Families (each a DiagGaussian(mu, ivar) and its start cloud; sd_d is no power of two):
  centred        mu = 0: the control
  offset_e       mu_d = s_d 2^e sd_d, s_d = +3, -3, +1, -1 cycling over d, column 0 at 0: e = 20, 34, 40
  scaled         the centred target and start times 2^(k_d) per column, k_d = +200, -200, 0, +37 cycling: every chain, summary,
                 histogram and autocorrelation time is the centred one's, scaled, bit for bit

Bounds (u = 2^-53; derived, never measured):
  mean  |mean - m| <= u |m| + 2 n u mean|x - m|       the final rounding, and any-order summation of the residuals x - mu0 (at most
                                                      (n - 1) u of sum|x - mu0|; the factor 2 covers mu0 being off m by less than the
                                                      spread, which holds up to offset_40 at the n used here)
  cov   |cov_jk - C_jk| <= 8 n u sqrt(C_jj C_kk)      the suite's bound (tests/test_gpu_batch_summary.py), now against the exact C

Why the kernels use the corrected two-pass covariance (the negative control of the CPU test): with mu0 the rounded mean, off by
delta, the plain form sum (x_j - mu0_j)(x_k - mu0_k) / (n - 1) is off by n / (n - 1) delta_j delta_k.  delta is relative to |mean|,
the bound to sd: at offset_34 and offset_40 the plain form breaks the bound.  (G_jk - r_j r_k / n) / (n - 1), r = sum (x - mu0),
removes exactly that term."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
FAMILIES = ("centred", "offset_20", "offset_34", "offset_40", "scaled")
OFFSET_FAMILIES = ("offset_20", "offset_34", "offset_40")
SIGNS = (3.0, -3.0, 1.0, -1.0)
SCALE_EXP = (200, -200, 0, 37)


def scale_exponents(D):
    return np.array([SCALE_EXP[d % 4] for d in range(D)], dtype=np.int64)


def family(name, D, seed):
    """-> dict(name, D, mu (D), ivar (D), sd (D), scale (D): the power of two every column is multiplied by (1 but for `scaled`))"""
    assert name in FAMILIES, name
    rs = np.random.RandomState(seed)
    sd = np.sqrt(0.2 + rs.rand(D))
    mu = np.zeros(D)
    scale = np.ones(D)
    if name.startswith("offset_"):
        e = int(name[len("offset_"):])
        s = np.array([SIGNS[d % 4] for d in range(D)])
        s[0] = 0.0
        assert D < 2 or (s < 0).any()
        mu = s * 2.0 ** e * sd
    elif name == "scaled":
        scale = 2.0 ** scale_exponents(D).astype(np.float64)
    # the scaled family is the centred one (same seed -> same sd) times a power of two: 1 / (sd sc)^2 = ivar / sc^2 exactly
    ivar = (1.0 / (sd * sd)) / (scale * scale)
    return dict(name=name, D=D, mu=mu, ivar=ivar, sd=sd * scale, scale=scale)


def start_cloud(fam, shape, seed):
    """start positions shape + (D,): mu + sd randn; the scaled family's are the centred family's times the scale, bit for bit"""
    rs = np.random.RandomState(seed)
    z = rs.randn(*(tuple(shape) + (fam["D"],)))
    return fam["mu"] + ((fam["sd"] / fam["scale"]) * z) * fam["scale"]


def recentre(x, mu):
    """x (..., D) -> x - mu, asserted exact: adding mu back gives x bit for bit"""
    x = np.asarray(x, dtype=np.float64)
    r = x - mu
    assert np.array_equal(r + mu, x), "x - mu is not exact: the recentred copy is not the same data"
    return r


def exact_mean(r, mu):
    """columns of r (n, D) recentred by mu -> the mean of x = r + mu as Fractions (D of them).  math.fsum rounds the exact sum
    once: the result is within u |sum r| / n of the exact mean, at most 1 / (2 n) of the bound's second term."""
    n = len(r)
    return [Fraction(math.fsum(r[:, d])) / n + Fraction(float(mu[d])) for d in range(r.shape[1])]


def mean_ratio(mean, r, mu):
    """|mean - m| / (u |m| + 2 n u mean|x - m|) per column, m the exact mean; 0 where both vanish"""
    n, D = r.shape
    out = np.zeros(D)
    for d, m in enumerate(exact_mean(r, mu)):
        err = abs(Fraction(float(mean[d])) - m)
        spread = math.fsum(np.abs(r[:, d] - float(m - Fraction(float(mu[d]))))) / n
        bound = U * abs(float(m)) + 2 * n * U * spread
        out[d] = float(err) / bound if bound > 0 else (0.0 if err == 0 else np.inf)
    return out


def exact_cov(r):
    """np.cov of the recentred copy (n, D) -> (D, D)"""
    return np.atleast_2d(np.cov(r.T))


def cov_bound(C, n):
    sd = np.sqrt(np.diag(C))
    return 8 * n * U * np.outer(sd, sd)


def cov_ratio(cov, r):
    """|cov_jk - C_jk| / (8 n u sqrt(C_jj C_kk)) -> (D, D); 0 where both vanish"""
    C = exact_cov(r)
    bound = cov_bound(C, len(r))
    err = np.abs(cov - C)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / bound)


def fraction_mean_cov(x):
    """x (n, D) -> (mean: D Fractions, cov: D x D Fractions, ddof = 1) in exact rational arithmetic; small inputs only"""
    n, D = x.shape
    cols = [[Fraction(float(v)) for v in x[:, d]] for d in range(D)]
    mean = [sum(c) / n for c in cols]
    dev = [[v - mean[d] for v in cols[d]] for d in range(D)]
    cov = [[sum(a * b for a, b in zip(dev[j], dev[k])) / (n - 1) for k in range(D)] for j in range(D)]
    return mean, cov


# ---- stand-ins for the device's arithmetic (the CPU test's negative control): float64, one fixed order, no extended precision
def sequential_sum(x):
    """columns of x (n, D) added one sample after the other, every partial sum rounded"""
    return np.cumsum(x, axis=0)[-1]


def plain_two_pass_cov(x):
    """sum (x_j - mu0_j)(x_k - mu0_k) / (n - 1) with the rounded mean mu0"""
    n = len(x)
    mu0 = sequential_sum(x) / n
    d = x - mu0
    G = np.stack([[sequential_sum((d[:, j] * d[:, k])[:, None])[0] for k in range(x.shape[1])] for j in range(x.shape[1])])
    return G / (n - 1)


def corrected_two_pass(x):
    """-> (mean, cov): mu0 + r / n and (G_jk - r_j r_k / n) / (n - 1), r = sum (x - mu0) in the mean's order"""
    n = len(x)
    mu0 = sequential_sum(x) / n
    d = x - mu0
    r = sequential_sum(d)
    G = np.stack([[sequential_sum((d[:, j] * d[:, k])[:, None])[0] for k in range(x.shape[1])] for j in range(x.shape[1])])
    return mu0 + r / n, (G - np.outer(r, r) / n) / (n - 1)


# ---- autocorrelation
def reference_tau(r, c=5):
    """recentred chain r (nt, N, D) -> (tau (D), windows (D), margin (D)): integrated_time's estimate and its Sokal window, and
    min over the chosen lag m and the lag before of |m - c tau(m)| / m -- how far the window is from tipping"""
    from emcee_amd import autocorr
    nt, _, D = r.shape
    tau = autocorr.integrated_time(r, c=c, tol=0, quiet=True)
    win, margin = np.zeros(D, dtype=np.int64), np.zeros(D)
    for d in range(D):
        rho = autocorr._batched_acf(r[:, :, d]).mean(axis=1)
        w, t = autocorr.tau_from_mean_acf(rho, c)
        assert t == tau[d]
        taus = 2.0 * np.cumsum(rho) - 1.0
        win[d] = w
        margin[d] = min(abs(m - c * taus[m]) / m for m in (w, w - 1) if m >= 1)
    return tau, win, margin
