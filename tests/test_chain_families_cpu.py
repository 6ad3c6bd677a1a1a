"""tests/chain_families.py held up without a device: its references against fractions.Fraction on small inputs, and the recorded
reason for the corrected two-pass covariance of the summary kernels -- the plain form breaks the suite's bound 8 n u sd sd once
|mean| / sd reaches 2^34, the corrected form does not."""
from fractions import Fraction

import numpy as np
import pytest

import chain_families as cf
from emcee_amd import autocorr

U = cf.U


def synthetic(name, n, D, seed=3):
    """n draws of the family's target, as a chain would hold them -> (x, family)"""
    fam = cf.family(name, D, seed)
    return cf.start_cloud(fam, (n,), seed + 1), fam


@pytest.mark.parametrize("name", cf.FAMILIES)
def test_families_are_what_they_say(name):
    D = 7
    fam = cf.family(name, D, 11)
    base = cf.family("centred", D, 11)
    assert np.array_equal(fam["sd"], base["sd"] * fam["scale"]) and np.array_equal(fam["ivar"] * fam["scale"] ** 2, base["ivar"])
    if name.startswith("offset_"):
        e = int(name.split("_")[1])
        assert fam["mu"][0] == 0 and (fam["mu"][1:] < 0).any() and (fam["mu"][1:] > 0).any()
        assert np.array_equal(fam["mu"][1:], np.array([cf.SIGNS[d % 4] for d in range(1, D)]) * 2.0 ** e * fam["sd"][1:])
    else:
        assert (fam["mu"] == 0).all()
    if name == "scaled":
        assert np.array_equal(np.log2(fam["scale"]), [200, -200, 0, 37, 200, -200, 0])
        assert np.array_equal(cf.start_cloud(fam, (5, 3), 2), cf.start_cloud(base, (5, 3), 2) * fam["scale"])
    else:
        assert (fam["scale"] == 1).all()


@pytest.mark.parametrize("name", cf.FAMILIES)
def test_recentring_is_exact(name):
    x, fam = synthetic(name, 500, 5)
    r = cf.recentre(x, fam["mu"])
    for d in range(5):                                      # exact as rationals, not only in floating point
        assert all(Fraction(float(a)) - Fraction(float(fam["mu"][d])) == Fraction(float(b)) for a, b in zip(x[:40, d], r[:40, d]))


def test_recentring_refuses_an_inexact_subtraction():
    x = np.array([[1.0 + 2.0 ** -52]])                      # half an ulp below it is a tie, which rounds to 1, and 1 + mu to 1 again
    with pytest.raises(AssertionError):
        cf.recentre(x, np.array([2.0 ** -53]))


@pytest.mark.parametrize("name", cf.FAMILIES)
def test_references_equal_fraction_arithmetic_within_the_stated_bounds(name):
    n, D = 200, 4
    x, fam = synthetic(name, n, D)
    r = cf.recentre(x, fam["mu"])
    mean, cov = cf.fraction_mean_cov(x)
    # the mean: within u |sum r| / n of the exact one
    for d, m in enumerate(cf.exact_mean(r, fam["mu"])):
        assert abs(m - mean[d]) <= Fraction(U) * abs(sum(Fraction(float(v)) for v in r[:, d])) / n, (name, d)
    # an exactly rounded mean passes the mean bound, NumPy's mean of the uncentred column need not
    exact_rounded = np.array([float(m) for m in mean])
    assert (cf.mean_ratio(exact_rounded, r, fam["mu"]) <= 1).all()
    # the covariance of the recentred copy: a dot product of n terms, within n u sd sd = 1 / 8 of the bound; twice that for the
    # centring
    C = cf.exact_cov(r)
    Cx = np.array([[float(cov[j][k]) for k in range(D)] for j in range(D)])
    ratio = np.abs(C - Cx) / cf.cov_bound(Cx, n)
    print("%s: np.cov of the recentred copy: worst err / bound = %.3g" % (name, ratio.max()))
    assert (ratio <= 0.25).all(), (name, ratio.max())
    assert (cf.cov_ratio(Cx, r) <= 0.25).all()


@pytest.mark.parametrize("name", cf.FAMILIES)
def test_plain_two_pass_breaks_the_bound_far_out_and_the_corrected_form_holds(name):
    """n = 66 x 37 samples of 7 columns, the smallest single-sampler case of the GPU test"""
    n, D = 66 * 37, 7
    x, fam = synthetic(name, n, D)
    r = cf.recentre(x, fam["mu"])
    plain = cf.cov_ratio(cf.plain_two_pass_cov(x), r).max()
    mean, cov = cf.corrected_two_pass(x)
    corrected = cf.cov_ratio(cov, r).max()
    numpy_cov = cf.cov_ratio(np.atleast_2d(np.cov(x.T)), r).max()
    mr = cf.mean_ratio(mean, r, fam["mu"]).max()
    print("%s: err / bound: plain %.3g, np.cov %.3g, corrected %.3g; corrected mean %.3g" % (name, plain, numpy_cov, corrected, mr))
    assert corrected <= 1 and mr <= 1, (name, corrected, mr)
    assert np.array_equal(cov, cov.T)
    if name in ("offset_34", "offset_40"):
        assert plain > 1, (name, plain)
    if name in ("centred", "scaled"):
        assert plain <= 1 and numpy_cov <= 1, (name, plain, numpy_cov)


@pytest.mark.parametrize("name", cf.FAMILIES)
def test_host_acf_centred_twice_equals_the_recentred_series(name):
    """autocorr._batched_acf on x against itself on the exactly recentred copy: the AR(1) walkers of a chain-like series"""
    nt, N, D = 257, 8, 3
    fam = cf.family(name, D, 5)
    rs = np.random.RandomState(6)
    z = np.zeros((nt, N, D))
    z[0] = rs.randn(N, D)
    for t in range(1, nt):
        z[t] = 0.9 * z[t - 1] + np.sqrt(1 - 0.81) * rs.randn(N, D)
    x = fam["mu"] + ((fam["sd"] / fam["scale"]) * z) * fam["scale"]
    r = cf.recentre(x, fam["mu"])
    tau, win, margin = cf.reference_tau(r)
    assert (margin > 1e-6).all(), margin
    got = autocorr.integrated_time(x, tol=0, quiet=True)
    np.testing.assert_allclose(got, tau, rtol=1e-8)
    for d in range(D):
        w, _ = autocorr.tau_from_mean_acf(autocorr._batched_acf(x[:, :, d]).mean(axis=1), 5)
        assert w == win[d], (name, d)
