"""tests/snooker_ref.py before it judges a kernel: the double-double reference against mpmath, the float64 transcription of
de_snooker.py:41-46 within HALF of both bounds on every family and ndim (which is what fixes the constants C1 ... C3), the float64
transcription of the kernel's formulation within the bounds, every listed mistake of that formulation outside them, and the exact
power-of-two covariance of the reference itself."""
import functools

import mpmath
import numpy as np
import pytest

import snooker_ref as sr

ROWS = 48


@functools.lru_cache(maxsize=None)
def _case(name, D):
    fam = sr.family(name, ROWS, D)
    return fam, sr.reference(fam["s"], fam["z"], fam["z1"], fam["z2"], fam["gammas"])


def _worst(fn, name, D, **kw):
    fam, ref = _case(name, D)
    q, f = fn(fam["s"], fam["z"], fam["z1"], fam["z2"], fam["gammas"], **kw)
    rq, rf = sr.ratios(q, f, ref)
    return float(rq.max()), float(rf.max())


def test_reference_against_mpmath():
    mpmath.mp.prec = 400
    for name in sr.FAMILIES:
        for D in (1, 2, 5, 33):
            fam, ref = _case(name, D)
            g = mpmath.mpf(fam["gammas"])
            for i in (0, 1, ROWS - 1):
                s, z, z1, z2 = ([mpmath.mpf(float(v)) for v in fam[k][i]] for k in ("s", "z", "z1", "z2"))
                delta = [a - b for a, b in zip(s, z)]
                norm = mpmath.sqrt(sum(d * d for d in delta))
                dd = sum(d * (a - b) for d, a, b in zip(delta, z1, z2)) / norm
                q = [a + d / norm * g * dd for a, d in zip(s, delta)]
                nq = mpmath.sqrt(sum((a - b) ** 2 for a, b in zip(q, z)))
                scale = max(abs(d) / norm * g * abs(dd) for d in delta)
                for d in range(D):
                    got = mpmath.mpf(float(ref["q"][0][i, d])) + mpmath.mpf(float(ref["q"][1][i, d]))
                    assert abs(got - q[d]) <= 2.0 ** -95 * (abs(q[d]) + scale), (name, D, i, d)
                f = (D - 1) * mpmath.log(nq / norm)
                # the double-double quotient is good to 2^-95 in units of (norm + gammas |dd|) / nq; the 80-bit logarithm to 2^-63
                tol = (D - 1) * (2.0 ** -62 * (1 + abs(mpmath.log(nq / norm))) + 2.0 ** -90 * (norm + g * abs(dd)) / nq)
                hi = float(ref["f"][i])
                got = mpmath.mpf(hi) + mpmath.mpf(float(ref["f"][i] - sr.LD(hi)))          # the 80-bit value, exactly
                assert abs(got - f) <= tol + mpmath.mpf(2) ** -1070, (name, D, i)


def test_exact_landing_rows_of_one_hot():
    for D in (1, 2, 7, 64):
        fam = sr.family("one_hot", ROWS, D, exact_landing=True)
        ref = sr.reference(fam["s"], fam["z"], fam["z1"], fam["z2"], fam["gammas"])
        assert np.array_equal(ref["qf"], fam["z"]) and np.all(ref["q"][1] == 0) and np.all(ref["nq"] == 0)
        assert np.all(np.isnan(ref["ff"])) if D == 1 else np.all(ref["ff"] == -np.inf)
        for fn in (sr.ref64, sr.kernel64):
            q, f = fn(fam["s"], fam["z"], fam["z1"], fam["z2"], fam["gammas"])
            assert np.array_equal(q, fam["z"]) and np.array_equal(f, ref["ff"], equal_nan=True)
    fam = sr.family("one_hot", ROWS, 9)
    ref = sr.reference(fam["s"], fam["z"], fam["z1"], fam["z2"], fam["gammas"])
    assert np.all(np.sum(ref["u"] == 0, axis=1) == 8) and np.all(np.sum(np.abs(ref["u"]) == 1, axis=1) == 1)


def test_families_are_what_they_say():
    D = 5
    r = {name: _case(name, D) for name in sr.FAMILIES}
    fam, ref = r["lands_on_z"]
    t = (ref["norm"] + fam["gammas"] * ref["dd"]) / ref["norm"]
    assert np.all(np.abs(t - 1e-6) < 1e-12) and np.all(np.abs(ref["nq"] / ref["norm"] - 1e-6) < 1e-9)
    fam, ref = r["close"]
    assert np.all(np.abs(fam["z2"] - fam["z1"]) < 1e-6) and np.all(fam["z2"] != fam["z1"])
    fam, ref = r["tiny_delta"]
    assert np.all(ref["norm"] < 1e-8) and np.all(ref["norm"] > 0)
    fam, ref = r["offset"]
    assert np.all(np.abs(fam["s"] - 2.0 ** 21) < 8)


def test_float64_transcriptions_stay_inside_the_bounds(capsys):
    """ref64 <= 0.5 of each bound: that leaves a kernel a factor of two over the reference's own float64 evaluation and no more;
    kernel64 <= 1"""
    lines = []
    for name in sr.FAMILIES:
        w = np.zeros(4)
        at = [0] * 4
        for D in sr.NDIMS:
            v = _worst(sr.ref64, name, D) + _worst(sr.kernel64, name, D)
            for k in range(4):
                if v[k] > w[k]:
                    w[k], at[k] = v[k], D
        lines.append("%-13s ref64 q %.3f (ndim %d) f %.3f (ndim %d) | kernel64 q %.3f (ndim %d) f %.3f (ndim %d)" % (
            name, w[0], at[0], w[1], at[1], w[2], at[2], w[3], at[3]))
        assert w[0] <= 0.5 and w[1] <= 0.5, lines[-1]
        assert w[2] <= 1.0 and w[3] <= 1.0, lines[-1]
    with capsys.disabled():
        print("\nsnooker reference, worst error / bound over ndim %d ... %d:" % (sr.NDIMS[0], sr.NDIMS[-1]))
        print("\n".join(lines))


MUTANT_NDIMS = (1, 2, 3, 5, 8, 33, 130)


@pytest.mark.parametrize("mutant", sr.MUTANTS)
def test_bounds_catch_the_mistake(mutant, capsys):
    """each mistake of the kernel's formulation leaves a bound (or turns a finite factor into a NaN) on at least one family.  None
    of the ten is uncatchable; log_without_fabs shows only where norm + gammas dd is negative for some row, which it never is on
    `close` (dd ~ 1e-7) and `lands_on_z` (+1e-6 norm by construction), and is on every other family."""
    caught = []
    for name in sr.FAMILIES:
        for D in MUTANT_NDIMS:
            try:
                rq, rf = _worst(sr.kernel64, name, D, mutant=mutant)
                hit = not (rq <= 1.0 and rf <= 1.0)
            except AssertionError:                 # non-finite where the reference is finite, or the other way round
                hit = True
            if hit:
                caught.append((name, D))
    with capsys.disabled():
        print("\n%-30s caught on %d of %d (family, ndim) cases; families: %s" % (
            mutant, len(caught), len(sr.FAMILIES) * len(MUTANT_NDIMS), sorted({c[0] for c in caught})))
    assert caught, mutant
    # a mistake of the general text shows on the benign cloud as well, not only at an edge
    assert any(c[0] == "benign" for c in caught), (mutant, caught)


@pytest.mark.parametrize("k", [40, -40, 9])
def test_reference_is_covariant_under_a_uniform_power_of_two(k):
    for D in (1, 2, 5, 33, 130):
        for name in ("benign", "close", "lands_on_z", "one_hot"):
            fam, ref = _case(name, D)
            sc = 2.0 ** k
            ref2 = sr.reference(fam["s"] * sc, fam["z"] * sc, fam["z1"] * sc, fam["z2"] * sc, fam["gammas"])
            assert np.array_equal(ref["q"][0] * sc, ref2["q"][0]) and np.array_equal(ref["q"][1] * sc, ref2["q"][1]), (name, D)
            assert np.array_equal(ref["f"], ref2["f"], equal_nan=True), (name, D)
            assert np.array_equal(ref["qbound"] * sc, ref2["qbound"]), (name, D)


def test_pow2_uniform_family_is_benign_scaled():
    for D in (3, 16):
        a = sr.family("pow2_uniform", ROWS, D)
        sc = np.where(np.arange(ROWS) % 2 == 0, 2.0 ** 40, 2.0 ** -40)[:, None]
        rs = sr.reference(a["s"], a["z"], a["z1"], a["z2"], a["gammas"])
        r1 = sr.reference(a["s"] / sc, a["z"] / sc, a["z1"] / sc, a["z2"] / sc, a["gammas"])
        assert np.array_equal(r1["q"][0] * sc, rs["q"][0]) and np.array_equal(r1["f"], rs["f"])
