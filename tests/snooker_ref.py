"""The snooker proposal (de_snooker.py:41-46; make_proposal<MOVE_SNOOKER> in csrc/emx_kernels.hpp) in double-double, its
forward-error bounds, and the seeded input families, shared by tests/test_snooker_ref_cpu.py and
tests/test_gpu_snooker_reference.py.  NumPy and tests/hiprec.py only: nothing here comes from the library.

Per row (s the walker, z, z1, z2 its three partners, D columns), in double-double unless said otherwise:

    delta = s - z            norm = sqrt(sum delta^2)            dd = (delta . (z1 - z2)) / norm
    q = s + (delta / norm) gammas dd                             nq = sqrt(sum (q - z)^2)   (q NOT rounded to float64 first)
    f = (D - 1) log(nq / norm)       the quotient in double-double, the logarithm and the product in np.longdouble

dd is dot(u, z1) - dot(u, z2) of the reference in its well-conditioned form (one sum of delta (z1 - z2), z1 - z2 exact as a
double-double).  For D = 1, f = 0 * log(...) by NumPy's rules: NaN where nq = 0.

THE BOUNDS (u = 2^-53 the unit roundoff, EPS = 2u).  They scale with what the arithmetic loses, never with |x| alone:

    A      = sum_d |delta_d| |z1_d| + sum_d |delta_d| |z2_d|
    ddb    = (D + C1) A / norm                                   what e1 / norm - e2 / norm can lose, in units of EPS
    qbound = EPS (|q_d| + C2 |u_d| gammas |dd| + |u_d| gammas ddb)
    fbound = (D - 1) EPS (C3 + |log nq| + |log norm| + (norm + gammas ddb + gammas |dd|) / nq)

C1 = 4.  Both the reference (dot(u, z1) - dot(u, z2)) and the kernel (e1 / norm - e2 / norm, e_k = sum delta z_k) form the two dot
  products apart.  fl(delta_d) = delta_d (1 + d), |d| <= u; a sum of D products passes through at most D roundings in any order
  (fma or not, a padded lane adds an exact zero): |e_k - exact| <= (D + 1) u sum |delta||z_k|.  The norm is off by at most
  (D / 2 + 2) u relatively in the worst case (below), which moves e_k / norm by that much of |e_k| <= sum |delta||z_k|, and the
  division adds u: together (1.5 D + 4) u A / norm = (0.75 D + 2) EPS A / norm <= (D + 4) EPS A / norm, the difference's own rounding,
  u |dd|, going to C2.
C2 = 4.  prod_d = fl(fl(fl(delta_d / norm) gammas) dd) carries, in units of |u_d| gammas |dd|: u (delta_d), u (the division), u
  (gammas), u (dd), u (the difference e1 / norm - e2 / norm above) and the norm's relative error.  sum delta^2 is a sum of non-negative
  terms: every partial sum is below the total, so its k-th rounding costs at most u of the total.  The kernel takes chains of
  CH V <= 16 fmas a lane and a tree of log2 G <= 6 levels, NumPy's dot 8-wide blocks and a tree: the roundings are of random sign and
  add up as the root of their number, sqrt(22) u for the sum, half of it for its root, u for sqrt itself: 3.4 u.  8.4 u in all, of
  which five are worst cases of single roundings that do not all occur at once: C2 EPS = 8 u.  The last addition s_d + prod_d is the
  EPS |q_d| term (u |q_d| would do; the second u leaves room for the reference's own rounding of q to float64 in the comparison).
  The absolute error of dd, EPS ddb, times |u_d| gammas, is the third term.
C3 = 4.  nq: the reference takes |q - z| from its rounded q, the kernel |norm + gammas dd| (|u| = 1).  Either way the absolute error of
  nq is that of norm (EPS norm at most, as above), gammas times that of dd (EPS ddb, and u |dd| of the product's rounding), and the
  last rounding: EPS (norm + gammas ddb + gammas |dd|) covers them.  log nq then moves by that over nq -- the condition number of the
  logarithm near nq -> 0 is what the bound must scale with -- and the two logarithms are each within an ulp of theirs: EPS |log nq| +
  EPS |log norm|, which also covers the subtraction's u |log nq - log norm| and the product with D - 1.  What is left is the
  relative error of norm inside log norm (1.7 EPS at most, as above) and second-order terms: C3 = 4 leaves twice that.

WHAT FIXES THE CONSTANTS.  The float64 NumPy transcription of de_snooker.py:41-46 (ref64) stays at or below 0.5 of each bound on
every family below at every ndim of NDIMS; the float64 transcription of the kernel's formulation (kernel64) stays below 1.  Worst
error / bound, measured on the CPU (tests/test_snooker_ref_cpu.py prints them):

    family          ref64 q   ref64 f   kernel64 q   kernel64 f        (48 rows a case, ndim 1 ... 1024)
    benign           0.467     0.130      0.467        0.120
    offset           0.481     0.073      0.481        0.100
    close            0.417     0.127      0.417        0.093
    tiny_delta       0.343     0.414      0.343        0.414
    lands_on_z       0.344     0.209      0.344        0.168
    one_hot          0.159     0.134      0.159        0.117
    pow2_uniform     0.394     0.224      0.394        0.228

(The proposal's share is the last rounding, u |q| = 0.5 EPS |q|: no float64 evaluation can stay far below 0.5 of qbound, and none of a
correct formulation comes near 1.)  Measured on an MI355X: the docstring of tests/test_gpu_snooker_reference.py."""
import numpy as np

import hiprec as hp

LD = np.longdouble
U = 2.0 ** -53
EPS = 2.0 * U
C1, C2, C3 = 4.0, 4.0, 4.0
GAMMAS = 1.7                     # DESnookerMove's default
GAMMAS_EXACT = 1.75              # the exact-landing rows of one_hot: 1.75 * 4 = 7 with no rounding anywhere
FAMILIES = ("benign", "offset", "close", "tiny_delta", "lands_on_z", "one_hot", "pow2_uniform")
# both ends of every (G, V, CH) range of pick_shape (csrc/emx_small_host.hpp) for odd (V = 1) and even (V = 2) ndim, up to the widest
# layout the snooker kernels are instantiated for (G 64, CH 8: 511 odd, 1024 even)
NDIMS = (1, 2, 3, 4, 5, 7, 8, 9, 10, 15, 16, 17, 18, 31, 32, 33, 34, 63, 64, 65, 66, 127, 128, 129, 130, 255, 256, 257, 258, 511, 512,
         514, 1024)
NDIMS_REFUSED = (513, 1026, 2049)


def _col(x):
    return x[0][:, None], x[1][:, None]


def reference(s, z, z1, z2, gammas):
    """rows s, z, z1, z2 (n, D) -> dict: q (n, D) double-double and qf its float64 rounding, f (n,) np.longdouble and ff its float64
    rounding, the floats delta, norm, dd, nq, u, and the bounds qbound (n, D), fbound (n,)"""
    s, z, z1, z2 = (np.ascontiguousarray(a, dtype=np.float64) for a in (s, z, z1, z2))
    n, D = s.shape
    delta = hp.two_sum(s, -z)                                          # exact
    norm = hp.sqrt(hp.dsum(hp.mul(delta, delta), axis=1))
    ddv = hp.div(hp.rowdot(delta, hp.two_sum(z1, -z2)), norm)
    u = hp.div(delta, _col(norm))
    q = hp.add(hp.dd(s), hp.mul(hp.mul_d(u, float(gammas)), _col(ddv)))
    qz = hp.sub(q, hp.dd(z))
    nq = hp.sqrt(hp.dsum(hp.mul(qz, qz), axis=1))
    ratio = hp.div(nq, norm)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = LD(D - 1.0) * np.log(ratio[0].astype(LD) + ratio[1].astype(LD))
    out = dict(q=q, qf=hp.to_float(q), f=f, ff=f.astype(np.float64), delta=hp.to_float(delta), norm=hp.to_float(norm),
               dd=hp.to_float(ddv), nq=hp.to_float(nq), u=hp.to_float(u), gammas=float(gammas), D=D)
    ad = np.abs(out["delta"])
    A = np.sum(ad * np.abs(z1), axis=1) + np.sum(ad * np.abs(z2), axis=1)
    ddb = (D + C1) * A / out["norm"]
    au = np.abs(out["u"])
    g = abs(float(gammas))
    out["ddb"] = ddb
    out["qbound"] = EPS * (np.abs(out["qf"]) + C2 * au * g * np.abs(out["dd"])[:, None] + au * g * ddb[:, None])
    with np.errstate(divide="ignore", invalid="ignore"):
        out["fbound"] = (D - 1.0) * EPS * (C3 + np.abs(np.log(out["nq"])) + np.abs(np.log(out["norm"]))
                                           + (out["norm"] + g * ddb + g * np.abs(out["dd"])) / out["nq"])
    return out


def ratios(q, f, ref):
    """error / bound of a proposal q (n, D) and its factor f (n,) -> (rq (n, D), rf (n,)); 0 where the error is 0.  A factor the
    reference gives as non-finite must be that value exactly, and where the bound is zero (D = 1) so must the error be."""
    errq = np.abs(hp.to_float(hp.sub(hp.dd(np.asarray(q, dtype=np.float64)), ref["q"])))
    rq = np.where(errq == 0, 0.0, errq / np.maximum(ref["qbound"], 1e-300))
    f = np.asarray(f, dtype=np.float64)
    fin = np.isfinite(ref["ff"])
    assert np.array_equal(f[~fin], ref["ff"][~fin], equal_nan=True), "a factor differs where the reference is not finite"
    assert np.all(np.isfinite(f[fin])), "a factor is not finite where the reference is"
    rf = np.zeros(len(f))
    errf = np.abs(f[fin].astype(LD) - ref["f"][fin]).astype(np.float64)
    rf[fin] = np.where(errf == 0, 0.0, errf / np.maximum(ref["fbound"][fin], 1e-300))
    return rq, rf


# ---- float64 transcriptions -------------------------------------------------------------------------------------------------------
def ref64(s, z, z1, z2, gammas):
    """de_snooker.py:41-46 in float64 NumPy, row by row -> (q, f)"""
    n, D = s.shape
    q = np.empty_like(s)
    m = np.empty(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(n):
            delta = s[i] - z[i]
            norm = np.linalg.norm(delta)
            u = delta / norm
            q[i] = s[i] + u * gammas * (np.dot(u, z1[i]) - np.dot(u, z2[i]))
            m[i] = np.log(np.linalg.norm(q[i] - z[i])) - np.log(norm)
        return q, (D - 1.0) * m


MUTANTS = ("sums_over_D_minus_1", "padding_column_in_n2", "e1_only", "gammas_twice", "u_not_normalised", "norm_float32",
           "D_for_D_minus_1", "log_without_fabs", "z1_z2_swapped", "delta_negated_in_second_pass")


def kernel64(s, z, z1, z2, gammas, mutant=None):
    """the kernel's formulation in float64 NumPy: the three sums n2, e1, e2 in one pass, dd = e1 / norm - e2 / norm, the proposal in a
    second pass, |q - z| = |norm + gammas dd| -> (q, f).  `mutant`: one of MUTANTS, the same text with that one mistake."""
    assert mutant is None or mutant in MUTANTS, mutant
    n, D = s.shape
    if mutant == "z1_z2_swapped":
        z1, z2 = z2, z1
    dl = s - z
    cols = slice(0, D - 1) if mutant == "sums_over_D_minus_1" else slice(0, D)
    n2 = np.sum(dl[:, cols] * dl[:, cols], axis=1)
    e1 = np.sum(dl[:, cols] * z1[:, cols], axis=1)
    e2 = np.sum(dl[:, cols] * z2[:, cols], axis=1)
    if mutant == "padding_column_in_n2":
        n2 = n2 + dl[:, -1] * dl[:, -1]
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = np.sqrt(n2)
        if mutant == "norm_float32":
            norm = norm.astype(np.float32).astype(np.float64)
        dd = e1 / norm if mutant == "e1_only" else e1 / norm - e2 / norm
        dl2 = -dl if mutant == "delta_negated_in_second_pass" else dl
        u = dl2 if mutant == "u_not_normalised" else dl2 / norm[:, None]
        ug = u * gammas
        if mutant == "gammas_twice":
            ug = ug * gammas
        q = s + ug * dd[:, None]
        t = norm + gammas * dd
        nq = t if mutant == "log_without_fabs" else np.abs(t)
        Df = D if mutant == "D_for_D_minus_1" else D - 1.0
        f = Df * (np.log(nq) - np.log(norm))
    return q, f


# ---- input families ---------------------------------------------------------------------------------------------------------------
def _seed(name, D, seed):
    return (1000003 * FAMILIES.index(name) + 7919 * D + seed) % (2 ** 32)


def family(name, n, D, seed=0, exact_landing=False):
    """n seeded rows of family `name` at ndim D -> dict(s, z, z1, z2 (n, D), gammas)

    benign        unit cloud
    offset        mean 2^21, unit spread
    close         z2 = z1 + 1e-7 noise
    tiny_delta    s = z + 1e-9 noise
    lands_on_z    z1 = z2 + u t + (noise orthogonal to u) with t such that norm + gammas dd = 1e-6 norm
    one_hot       delta non-zero in one column (exact zeros in u); exact_landing: small integers and gammas = 1.75 such that the
                  proposal IS z (nq = 0, f = -inf; NaN at ndim 1), every operation of either formulation being exact
    pow2_uniform  benign times 2^40 (even rows) and times 2^-40 (odd rows)"""
    rs = np.random.RandomState(_seed(name, D, seed))
    s, z, z1, z2 = (rs.randn(n, D) for _ in range(4))
    g = GAMMAS
    if name == "offset":
        s, z, z1, z2 = (2.0 ** 21 + a for a in (s, z, z1, z2))
    elif name == "close":
        z2 = z1 + 1e-7 * rs.randn(n, D)
    elif name == "tiny_delta":
        s = z + 1e-9 * rs.randn(n, D)
    elif name == "lands_on_z":
        delta = s - z
        norm = np.sqrt(np.sum(delta * delta, axis=1))
        u = delta / norm[:, None]
        w = rs.randn(n, D)
        w = w - np.sum(w * u, axis=1)[:, None] * u
        t = -(1.0 - 1e-6) * norm / g
        z1 = z2 + u * t[:, None] + w
    elif name == "one_hot":
        k = rs.randint(D, size=n)
        r = np.arange(n)
        if exact_landing:
            g = GAMMAS_EXACT
            s, z, z1, z2 = (np.round(4.0 * a) for a in (s, z, z1, z2))
            m = rs.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], n)
            s = z.copy()
            s[r, k] = z[r, k] + 7.0 * m                            # delta_k = 7 m, norm = 7 |m|
            z1[r, k] = z2[r, k] - 4.0 * m                          # dd = sign(m) (-4 m): norm + 1.75 dd = 0
        else:
            a = s[r, k]
            s = z.copy()
            s[r, k] = a
    elif name == "pow2_uniform":
        sc = np.where(np.arange(n) % 2 == 0, 2.0 ** 40, 2.0 ** -40)[:, None]
        s, z, z1, z2 = (a * sc for a in (s, z, z1, z2))
    elif name != "benign":
        raise KeyError(name)
    return dict(s=s, z=z, z1=z1, z2=z2, gammas=g)
