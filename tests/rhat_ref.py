"""Split-R-hat: the exact reference, the derived error bounds and the stand-ins for the device's arithmetic, shared by
tests/test_rhat_cpu.py and tests/test_gpu_rhat.py.  The definition is emcee_amd.summary.split_rhat's (csrc/emx_rhat.hip repeats it).

Everything here works on the half-series themselves: chains_of() cuts an array into z (G, C, h, W) -- G groups of C chains of
length h, W columns -- in the kernel's chain order (member, walker, half).  exact() is the definition in fractions.Fraction.

The arithmetic under test (kernel_arithmetic() is its NumPy transcription, summed one sample after the other), per chain c:
  mu0 = x0 + sum(x - x0) / h        x0 the chain's first sample.  eta = |mu0 - mu_c| <= u |mu_c| + (h + 2) u mean|x - x0|
  d = x - mu0,  r = sum d,  G = sum d^2,  s2 = (G - r^2 / h) / (h - 1),  q = r / h        (the chain mean is mu0 + q)
and per group, with c0 = mu0 of the group's first chain:
  e_c = (mu0_c - c0) + q_c,  within = sum s2_c / C,  between = (sum e_c^2 - (sum e_c)^2 / C) / (C - 1)

Bounds (u = 2^-53; first order in u; derived, never measured).  m is the group mean, W and B the exact within and between,
a_c = mean_t |x_ct - m| the mean absolute deviation of chain c's samples from the group mean, abar = mean_c a_c.

Regime.  Both bounds suppose eta_max = max_c eta_c <= min(sqrt(W) / 2, abar / 4): the centres are off their chains' means by
less than the spread.  eta is a rounding of mu0, so this fails only where the spread itself is of the order of h ulp(|mean|), where
a double holds no variance to speak of.  regime_ratio() computes eta_max's bound from exact quantities and the tests assert it
on their data (it holds with a factor > 100 to spare up to offset_40); the bounds themselves have no term in |mean|.

within.   With rho = eta / s: G carries (h + 2) u of (h - 1) s^2 + h eta^2 (h fused steps and two roundings of d^2's operand),
          r carries (h + 1) u sum|d| <= (h + 1) u h sqrt(s^2 + eta^2), so r^2 / h is off by 2 h eta of that, and three more
          roundings finish s2.  Averaged over the group (Jensen for the square root) with eta <= sqrt(W) / 2 this is at most
          (h + 5 + (h + 2) h / (4 (h - 1)) + 1.13 (h + 1) h / (h - 1)) u W <= 8 h u W for every h >= 2: the suite's own variance bound
          (chain_families.cov_bound, 8 n u).  Averaging C non-negative terms in any order adds (C - 1) u, the division u:
            |within - W| <= (8 h + C) u W
between.  Write b_c = a_c + abar / 4 (>= a_c + eta).  Then mean_t|d| <= 2 a_c + eta <= 2 b_c, the centre is off the group mean by
          delta with |delta| <= a_1 + eta <= b_1, and |e_c| <= b_c + b_1.  The computed e_c is off by
            Delta_c <= u (2 |e_c| + 2 (h + 2) b_c)      (the subtraction, q's sum of h terms and division, the addition).
          T = sum e^2 - (sum e)^2 / C = (C - 1) B whatever the centre, and Q = sum e^2 = (C - 1) B + C delta^2.  Rounding T from
          the computed e (C fused steps; C - 1 additions of sum e, squared; a product, a division, a subtraction) costs at most
          (3 C + 2) u Q, using C delta^2 <= Q; the Delta_c move T by at most 2 sum (|e_c| + |delta|) Delta_c
          <= u (8 Q + 4 (h + 2) (sum b_c^2 + 2 b_1 sum b_c)).  With Q <= (C - 1) B + C b_1^2 and a factor 2 for the division by
          C - 1 and the terms of second order:
            |between - B| <= 2 u ((3 C + 10) ((C - 1) B + C b_1^2) + 4 (h + 2) (sum b_c^2 + 2 b_1 sum b_c)) / (C - 1)
          It is written in u, h, C and the group's spread alone.

The negative control, one_pass(): sum x and sum x^2.  Its variance is off by u h |mean|^2: at offset_34 and offset_40 it breaks
both bounds by many orders of magnitude."""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53


def chains_of(x, log_prob=None, pool=False):
    """x (nt, N, D) or (nt, B, N, D) [+ log_prob without the last axis, appended as a column] -> z (G, C, h, W): B groups of 2 N
    chains, or with pool one group of 2 B N, chains in (member, walker, half) order"""
    x = np.asarray(x, dtype=np.float64)
    if log_prob is not None:
        x = np.concatenate([x, np.asarray(log_prob, dtype=np.float64)[..., None]], axis=-1)
    if x.ndim == 3:
        x = x[:, None]
    nt, B, N, W = x.shape
    h = nt // 2
    z = np.stack([x[:h], x[nt - h:]], axis=0).transpose(2, 3, 0, 1, 4)          # (B, N, 2, h, W)
    return np.ascontiguousarray(z.reshape((1, B * N * 2, h, W) if pool else (B, N * 2, h, W)))


def exact(z):
    """the definition in Fractions -> dict of (G, W) object arrays: within, between, and the spread the bounds are written in:
    a (G, W) lists of the C values a_c, eta (G, W) the bound on eta_max"""
    G, C, h, W = z.shape
    out = {k: np.empty((G, W), dtype=object) for k in ("within", "between", "a", "eta")}
    for g in range(G):
        for w in range(W):
            chains = [[Fraction(float(v)) for v in z[g, c, :, w]] for c in range(C)]
            mu = [sum(ch) / h for ch in chains]
            s2 = [sum((v - m) ** 2 for v in ch) / (h - 1) for ch, m in zip(chains, mu)]
            m = sum(mu) / C
            out["within"][g, w] = sum(s2) / C
            out["between"][g, w] = sum((v - m) ** 2 for v in mu) / (C - 1)
            out["a"][g, w] = [sum(abs(v - m) for v in ch) / h for ch in chains]
            out["eta"][g, w] = max(Fraction(U) * abs(mc) + (h + 2) * Fraction(U) * sum(abs(v - ch[0]) for v in ch) / h
                                   for ch, mc in zip(chains, mu))
    return out


def bounds(ex, C, h):
    """-> (within bound, between bound), float (G, W), from exact()'s dict"""
    G, W = ex["within"].shape
    bw, bb = np.empty((G, W)), np.empty((G, W))
    for g in range(G):
        for w in range(W):
            a = ex["a"][g, w]
            abar = sum(a) / C
            b = [v + abar / 4 for v in a]
            sb, sb2 = sum(b), sum(v * v for v in b)
            Q = (C - 1) * ex["between"][g, w] + C * b[0] ** 2
            bw[g, w] = float((8 * h + C) * ex["within"][g, w]) * U
            bb[g, w] = float(2 * ((3 * C + 10) * Q + 4 * (h + 2) * (sb2 + 2 * b[0] * sb)) / (C - 1)) * U
    return bw, bb


def regime_ratio(ex, C):
    """eta_max / min(sqrt(W) / 2, abar / 4) -> float (G, W): the bounds suppose <= 1.  0 for a constant group."""
    G, W = ex["within"].shape
    out = np.zeros((G, W))
    for g in range(G):
        for w in range(W):
            lim = min(float(ex["within"][g, w]) ** 0.5 / 2, float(sum(ex["a"][g, w]) / C) / 4)
            eta = float(ex["eta"][g, w])
            out[g, w] = 0.0 if eta == 0 else (eta / lim if lim > 0 else np.inf)
    return out


def ratios(within, between, ex, C, h):
    """|within - W| / bound and |between - B| / bound -> two float (G, W) arrays; 0 where the error is 0"""
    bw, bb = bounds(ex, C, h)
    G, W = bw.shape
    rw, rb = np.zeros((G, W)), np.zeros((G, W))
    for g in range(G):
        for w in range(W):
            for out, got, want, bound in ((rw, within, ex["within"], bw), (rb, between, ex["between"], bb)):
                v = float(got[g, w])
                if not np.isfinite(v):
                    out[g, w] = np.inf
                    continue
                err = float(abs(Fraction(v) - want[g, w]))
                out[g, w] = 0.0 if err == 0 else (err / bound[g, w] if bound[g, w] > 0 else np.inf)
    return rw, rb


def rhat_expression(within, between, h):
    """the NumPy expression that the definition fixes for rhat"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt((h - 1) / h + between / within)


def check(r, z, what):
    """r: an RHat whose arrays are (W,) or (G, W); z (G, C, h, W): the chains it was computed from.  Asserts the regime, both
    bounds against exact() and rhat's expression bit for bit -> worst err / bound of within and of between"""
    G, C, h, W = z.shape
    assert (r.nchains, r.length) == (C, h), what
    within, between = np.asarray(r.within).reshape(G, W), np.asarray(r.between).reshape(G, W)
    ex = exact(z)
    assert regime_ratio(ex, C).max() <= 1, (what, "the data is outside the regime the bounds suppose")
    rw, rb = ratios(within, between, ex, C, h)
    print("%s: within worst err / bound = %.3g, between = %.3g" % (what, rw.max(), rb.max()))
    assert rw.max() <= 1 and rb.max() <= 1, (what, rw.max(), rb.max())
    assert np.array_equal(np.asarray(r.rhat).reshape(G, W), rhat_expression(within, between, h), equal_nan=True), what
    return float(rw.max()), float(rb.max())


# ---- stand-ins for the device's arithmetic: float64, one sample after the other, no extended precision
def _seq(v, axis):
    return np.take(np.cumsum(v, axis=axis), -1, axis=axis)


def kernel_arithmetic(z):
    """the kernels' passes and centres -> (within, between) (G, W)"""
    G, C, h, W = z.shape
    x0 = z[:, :, :1]
    mu0 = x0[:, :, 0] + _seq(z - x0, 2) / h
    d = z - mu0[:, :, None]
    r = _seq(d, 2)
    s2 = (_seq(d * d, 2) - r * r / h) / (h - 1)
    e = (mu0 - mu0[:, :1]) + r / h
    e1 = _seq(e, 1)
    return _seq(s2, 1) / C, (_seq(e * e, 1) - e1 * e1 / C) / (C - 1)


def one_pass(z):
    """the negative control: sum x and sum x^2, for the chains and again for their means"""
    G, C, h, W = z.shape
    s1 = _seq(z, 2)
    s2 = (_seq(z * z, 2) - s1 * s1 / h) / (h - 1)
    mu = s1 / h
    m1 = _seq(mu, 1)
    return _seq(s2, 1) / C, (_seq(mu * mu, 1) - m1 * m1 / C) / (C - 1)
