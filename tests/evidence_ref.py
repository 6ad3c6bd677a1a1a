"""The exact reference of PTSampler.get_evidence / pt.stepping_stone_log_evidence, for tests/test_pt_evidence_cpu.py and
tests/test_gpu_pt_evidence.py: the definition at the top of csrc/emx_pt_evidence.hip on float64 inputs, in stdlib `decimal` at 60
digits.  d = fl(b[j] - b[j+1]) and a = fl(d L) are the doubles the definition names, converted exactly; every exp, sum, log,
merge, standard deviation and trapezoid after that is Decimal's.  -inf and NaN follow the definition's rules (the context traps
nothing, so inf - inf is NaN and log 0 is -inf as in IEEE arithmetic).

Error bounds (u = 2^-52; `check` holds a result to them and returns the worst err / bound):
  a log-ratio     (n_merged + 2 max|d L| + 16) u, n_merged the samples merged into it (n for a block's, K n for the selection's):
                  the worst-case summation error of positive terms, (n - 1) u; the two roundings in the exponent's argument,
                  relative to |d L|; a handful of ulps for exp, log and the merges; a factor 2 of slack.  A block's S is held to
                  the same bound relative to S (d log S = dS / S), its M exactly (a maximum has no rounding).
  a mean of L     n_merged u max|L| over the finite L.  A block's sum of L: n times that.
  tail            b[T-1] times the mean's bound, plus u |tail| for the product.
  logz_ss         the sum of its parts' bounds, plus T u (sum |parts|) for the additions; block_logz_ss likewise.
  logz_ti         the largest mean bound of the ladder (the trapezoid weights add up to b[0] = 1) plus (T + 4) u max|mean| for
                  its roundings; dlogz_ti, the difference of two such integrals, twice that plus 2 u max|mean|.
  err_*           K values each within E move their standard error by at most E / sqrt(K - 1) <= E; plus 8 u max|value| for the
                  subtractions from the mean.
Non-finite outputs must match in kind."""
import decimal
from decimal import Decimal

import numpy as np

U = Decimal(2) ** -52
NEG, NAN = Decimal("-Infinity"), Decimal("NaN")
FIELDS = ("logz_ss", "err_ss", "logz_ti", "dlogz_ti", "err_ti", "log_ratios", "mean_logl", "tail", "block_logz_ss", "block_logz_ti")


def context():
    return decimal.Context(prec=60, traps=[])


def _dsum(xs, c):
    tot = Decimal(0)
    for x in xs:
        tot = c.add(tot, x)
    return tot


def _finite_max_abs(x):
    x = np.abs(x[np.isfinite(x)])
    return Decimal(float(x.max())) if x.size else Decimal(0)


def _ti(b, y, c):
    """pt._ti on one ladder: Decimals b (T), y (T) -> (logz, |logz - logz2|)"""
    b, y = list(b), list(y)
    if b[-1] != 0:
        b, y = b + [Decimal(0)], y + [y[-1]]
    b2, y2 = b[:-1:2] + [Decimal(0)], y[:-1:2] + [y[-1]]

    def trapezoid(yy, xx):
        return _dsum([c.multiply(c.multiply(Decimal("0.5"), c.subtract(xx[i + 1], xx[i])), c.add(yy[i + 1], yy[i])) for i in range(len(xx) - 1)], c)
    lz, lz2 = c.minus(trapezoid(y, b)), c.minus(trapezoid(y2, b2))
    return lz, c.abs(c.subtract(lz, lz2))


def _stderr(v, c):
    K = len(v)
    if K < 2:
        return NAN
    mean = c.divide(_dsum(v, c), Decimal(K))
    ss = _dsum([c.power(c.subtract(x, mean), 2) for x in v], c)
    return c.divide(c.sqrt(c.divide(ss, Decimal(K - 1))), c.sqrt(Decimal(K)))


def exact(betas, logls, nblocks):
    """betas (G, T), logls (G, T, nt, N) float64 -> dict: the per-block triples "sum_L" (G, T, K), "amax" (G, T - 1, K; float64,
    exact), "sexp" (G, T - 1, K), "block_log_ratio", every Evidence field of FIELDS, and a bound for each under "bound" -- object
    arrays of Decimal (finite, -Infinity or NaN)"""
    c = context()
    b = np.asarray(betas, dtype=np.float64)
    x = np.asarray(logls, dtype=np.float64)
    G, T, nt, N = x.shape
    K = int(nblocks)
    bl = nt // K
    n = bl * N
    assert bl >= 1 and b.shape == (G, T)
    x = x[:, :, nt - K * bl:].reshape(G, T, K, n)
    obj = lambda *s: np.empty(s, dtype=object)  # noqa: E731
    A, M, S, lr = obj(G, T, K), np.empty((G, T - 1, K)), obj(G, T - 1, K), obj(G, T - 1, K)
    bd = {k: None for k in ("sum_L", "sexp", "block_log_ratio") + FIELDS}
    bd["sum_L"], bd["block_log_ratio"], bd["log_ratios"], bd["mean_logl"] = obj(G, T, K), obj(G, T - 1, K), obj(G, T - 1), obj(G, T)
    for k in ("logz_ss", "err_ss", "logz_ti", "dlogz_ti", "err_ti", "tail"):
        bd[k] = obj(G)
    bd["block_logz_ss"], bd["block_logz_ti"] = obj(G, K), obj(G, K)
    out = {k: obj(G) for k in ("logz_ss", "err_ss", "logz_ti", "dlogz_ti", "err_ti", "tail")}
    out.update(log_ratios=obj(G, T - 1), mean_logl=obj(G, T), block_logz_ss=obj(G, K), block_logz_ti=obj(G, K))
    dn, dKn = Decimal(n), Decimal(K * n)
    for g in range(G):
        for t in range(T):
            for k in range(K):
                v = x[g, t, k]
                A[g, t, k] = NAN if np.isnan(v).any() else NEG if (v == -np.inf).any() else _dsum([Decimal(float(q)) for q in v], c)
                bd["sum_L"][g, t, k] = dn * dn * U * _finite_max_abs(v)
            out["mean_logl"][g, t] = c.divide(_dsum(list(A[g, t]), c), dKn)
            bd["mean_logl"][g, t] = dKn * U * _finite_max_abs(x[g, t])
        bmean = [[c.divide(A[g, t, k], dn) for t in range(T)] for k in range(K)]
        bmean_bd = [[dn * U * _finite_max_abs(x[g, t, k]) for t in range(T)] for k in range(K)]
        for j in range(T - 1):
            d = b[g, j] - b[g, j + 1]                   # fl(b[j] - b[j+1])
            amax_all = Decimal(0)
            for k in range(K):
                a = d * x[g, j + 1, k]                  # fl(d L)
                assert not (a == np.inf).any(), "+inf is outside the definition"
                fin = a[np.isfinite(a)]
                m = float(fin.max()) if fin.size else -np.inf
                M[g, j, k] = m
                if np.isnan(a).any():
                    S[g, j, k] = NAN
                else:
                    dm = Decimal(m)
                    S[g, j, k] = _dsum([c.exp(c.subtract(Decimal(float(q)), dm)) for q in fin], c)
                lr[g, j, k] = c.add(Decimal(m), c.ln(c.divide(S[g, j, k], dn)))
                amax = _finite_max_abs(a)
                amax_all = max(amax_all, amax)
                bd["block_log_ratio"][g, j, k] = (dn + 2 * amax + 16) * U
            ms = float(M[g, j].max())
            w = [S[g, j, k] if M[g, j, k] == -np.inf else c.multiply(S[g, j, k], c.exp(c.subtract(Decimal(float(M[g, j, k])), Decimal(ms))))
                 for k in range(K)]
            out["log_ratios"][g, j] = c.add(Decimal(ms), c.ln(c.divide(_dsum(w, c), dKn)))
            bd["log_ratios"][g, j] = (dKn + 2 * amax_all + 16) * U
        last = Decimal(float(b[g, T - 1]))
        db = [Decimal(float(q)) for q in b[g]]

        def with_tail(ratios, ratio_bounds, mean_last, mean_last_bound):
            tail = c.multiply(last, mean_last) if last > 0 else Decimal(0)
            tail_bd = (last * mean_last_bound + U * abs(tail)) if last > 0 and tail.is_finite() else Decimal(0)
            parts = list(ratios) + [tail]
            tot = _dsum(parts, c)
            mag = _dsum([abs(p) for p in parts if p.is_finite()], c)
            return tail, tail_bd, tot, _dsum(list(ratio_bounds), c) + tail_bd + T * U * mag

        def ti_bounds(means, mean_bounds):
            mag = max([abs(q) for q in means if q.is_finite()] + [Decimal(0)])
            e = max(mean_bounds) + (T + 4) * U * mag
            return e, 2 * e + 2 * U * mag
        out["tail"][g], bd["tail"][g], out["logz_ss"][g], bd["logz_ss"][g] = with_tail(
            out["log_ratios"][g], bd["log_ratios"][g], out["mean_logl"][g, T - 1], bd["mean_logl"][g, T - 1])
        out["logz_ti"][g], out["dlogz_ti"][g] = _ti(db, list(out["mean_logl"][g]), c)
        bd["logz_ti"][g], bd["dlogz_ti"][g] = ti_bounds(list(out["mean_logl"][g]), list(bd["mean_logl"][g]))
        for k in range(K):
            _, _, out["block_logz_ss"][g, k], bd["block_logz_ss"][g, k] = with_tail(
                lr[g, :, k], bd["block_log_ratio"][g, :, k], bmean[k][T - 1], bmean_bd[k][T - 1])
            out["block_logz_ti"][g, k] = _ti(db, bmean[k], c)[0]
            bd["block_logz_ti"][g, k] = ti_bounds(bmean[k], bmean_bd[k])[0]
        for err, blocks in (("err_ss", "block_logz_ss"), ("err_ti", "block_logz_ti")):
            out[err][g] = _stderr(list(out[blocks][g]), c)
            fin = [abs(q) for q in out[blocks][g] if q.is_finite()]
            bd[err][g] = max(bd[blocks][g]) + 8 * U * max(fin + [Decimal(0)])
    bd["sexp"] = bd["block_log_ratio"]
    out.update(sum_L=A, amax=M, sexp=S, block_log_ratio=lr, bound=bd, n=n, nblocks=K, block_length=bl)
    return out


def kind(v):
    """'nan', '-inf', '+inf' or 'finite' of a float or a Decimal"""
    if isinstance(v, Decimal):
        return "nan" if v.is_nan() else ("-inf" if v < 0 else "+inf") if v.is_infinite() else "finite"
    v = float(v)
    return "nan" if v != v else "-inf" if v == -np.inf else "+inf" if v == np.inf else "finite"


def compare(got, want, bound, what, relative=False):
    """every element of the float array `got` against the Decimals `want` -> the worst err / bound (0 where nothing is finite)"""
    got, worst = np.asarray(got, dtype=np.float64), 0.0
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for idx in np.ndindex(*got.shape):
        g, w = got[idx], want[idx]
        assert kind(g) == kind(w), "%s%s: got %r, the reference has %r" % (what, list(idx), g, w)
        if kind(w) == "finite":
            err, lim = abs(Decimal(float(g)) - w), bound[idx] * (abs(w) if relative else 1)
            assert err <= lim, "%s%s: got %r, the reference has %s: off by %.3g, the bound is %.3g" % (what, list(idx), g, w, err, lim)
            if lim > 0:
                worst = max(worst, float(err / lim))
    return worst


def check(ev, ref, what=""):
    """an Evidence against exact()'s dict -> {field: worst err / bound}"""
    assert (ev.nblocks, ev.block_length) == (ref["nblocks"], ref["block_length"]), what
    return {f: compare(getattr(ev, f), ref[f], ref["bound"][f], "%s %s" % (what, f)) for f in FIELDS}


def check_blocks(A, M, S, ref, what=""):
    """the device's per-block triples against exact()'s -> {name: worst err / bound}"""
    assert np.array_equal(np.asarray(M), ref["amax"]), "%s amax" % what
    return {"sum_L": compare(A, ref["sum_L"], ref["bound"]["sum_L"], what + " sum_L"),
            "sexp": compare(S, ref["sexp"], ref["bound"]["sexp"], what + " sexp", relative=True)}
