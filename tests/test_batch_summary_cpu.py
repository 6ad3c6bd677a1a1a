"""EnsembleBatch.get_summary without a GPU: the C ABI of emx_summary_batch / emx_host_order_stats, the argument checks that
must fire before any device is touched, the host interpolation (summary.quantile_ranks + summary.lerp against np.quantile)
and the radix selection the kernels share with their host twin (against np.sort, exactly)."""
import os
import re

import numpy as np
import pytest

from emcee_amd import BatchSummary, EnsembleBatch, PTSampler, _lib, summary, targets
from emcee_amd.targets import BatchCallable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


@pytest.fixture
def no_device(monkeypatch):
    """any attempt to create the device handle or to call the library fails the test"""
    def refuse(self):
        raise AssertionError("a device was touched before the arguments were checked")
    monkeypatch.setattr(EnsembleBatch, "_handle", refuse)
    monkeypatch.setattr(EnsembleBatch, "_lib", refuse)


def header_text():
    return open(os.path.join(ROOT, "include", "emx.h")).read()


def declared_types(name):
    txt = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, txt)
    assert m, "include/emx.h does not declare %s" % name
    return [p.strip().rsplit(None, 1)[0].replace(" *", "*") for p in m.group(1).split(",")]


def test_header_declares_and_library_exports_the_entry_points():
    assert declared_types("emx_summary_batch") == [
        "emx_batch*", "int32_t", "int32_t", "int64_t", "int64_t", "int64_t", "double*", "double*", "int32_t", "const int64_t*", "double*",
        "double*", "double*", "int64_t*"]
    assert declared_types("emx_host_order_stats") == ["const double*", "int64_t", "int64_t", "int32_t", "const int64_t*", "double*"]
    lib = _lib.load()
    for name, nargs in (("emx_summary_batch", 14), ("emx_host_order_stats", 6)):
        assert hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.C.c_int and len(args) == nargs
    assert '"batch_summary_members"' in header_text()
    assert BatchSummary is summary.BatchSummary
    assert BatchSummary._fields == ("nsamples", "mean", "cov", "quantiles", "map_coords", "map_log_prob")


def test_build_compiles_the_new_translation_unit():
    from emcee_amd import _build
    assert any(s.endswith("emx_batch_summary.hip") for s in _build.SRCS)
    assert len(_build.SRCS) == 17


def bad_argument_cases(get):
    with pytest.raises(ValueError, match="run the sampler"):
        get()
    for thin in (0, -1, 1.5):
        with pytest.raises(ValueError, match="thin"):
            get(thin=thin)
    for discard in (-1, 0.5):
        with pytest.raises(ValueError, match="discard"):
            get(discard=discard)
    for q in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match="quantile"):
            get(quantiles=(0.5, q))
        with pytest.raises(ValueError, match="quantile"):
            get(quantiles=q)
    with pytest.raises(ValueError, match="at most 16"):
        get(quantiles=np.linspace(0, 1, 17))


def test_bad_arguments_before_any_device(no_device):
    bt = EnsembleBatch(3, 16, 2, targets.IsoGaussian(), seeds=[1, 2, 3])
    bad_argument_cases(bt.get_summary)
    bad_argument_cases(bt[1].get_summary)
    with pytest.raises(ValueError, match="members"):
        bt._summary_device(lo=2, hi=2)
    with pytest.raises(ValueError, match="members"):
        bt._summary_device(lo=0, hi=4)
    with pytest.raises(ValueError, match="at most 32 ranks"):
        bt._summary_device(ranks=list(range(33)))


def test_bad_arguments_before_any_device_ptsampler(no_device):
    pt = PTSampler(3, 16, 2, BatchCallable(lambda q: -0.5 * (q ** 2).sum(-1)), nbatch=2, seeds=[1, 2])
    bad_argument_cases(pt.get_summary)


# ---------------------------------------------------------------------------------------------------------------- quantiles
def quantile_inputs():
    rs = np.random.RandomState(0)
    yield "n1", np.array([3.25])
    yield "n2", np.array([-1.0, 2.0])
    yield "normal_1001", rs.randn(1001)
    yield "ties_5000", np.round(rs.randn(5000), 1)
    yield "all_equal", np.full(77, -2.5)
    yield "offset_2e5", 1e3 + rs.randn(200000)
    yield "ties_2e5", np.round(10 * rs.randn(200000), 1)
    yield "wide_range", rs.randn(4096) * 10.0 ** rs.randint(-8, 8, size=4096)


@pytest.mark.parametrize("name,x", list(quantile_inputs()), ids=[n for n, _ in quantile_inputs()])
def test_ranks_and_lerp_reproduce_np_quantile(name, x):
    rs = np.random.RandomState(len(x))
    q = np.concatenate([[0.0, 0.16, 0.5, 0.84, 1.0], rs.rand(40)])
    xs = np.sort(x)
    lo, hi, g = summary.quantile_ranks(len(x), q)
    assert lo.dtype == np.int64 and (0 <= lo).all() and (lo <= hi).all() and (hi <= len(x) - 1).all() and (hi - lo <= 1).all()
    assert (0 <= g).all() and (g < 1).all()
    got = summary.lerp(xs[lo], xs[hi], g)
    ref = np.quantile(x, q)
    err = np.abs(got - ref).max()
    print("%s: max |ours - np.quantile| = %.3g (bound %.3g)" % (name, err, 4 * U * np.abs(x).max()))
    assert err <= 4 * U * np.abs(x).max()
    if np.__version__.startswith("2.2"):
        assert np.array_equal(got, ref)
    # scalar q, and plan_ranks' shared ranks
    lo1, hi1, g1 = summary.quantile_ranks(len(x), 0.5)
    assert summary.lerp(xs[lo1], xs[hi1], g1) == got[2]
    ranks, ilo, ihi, gg = summary.plan_ranks(len(x), q)
    assert np.array_equal(ranks, np.unique(ranks)) and np.array_equal(ranks[ilo], lo) and np.array_equal(ranks[ihi], hi)
    out = summary.interpolate(xs[ranks][None, :, None], ilo, ihi, gg)
    assert np.array_equal(out[0, :, 0], got)


def test_no_quantiles_is_an_empty_array():
    ranks, ilo, ihi, g = summary.plan_ranks(10, summary.check_quantiles(()))
    assert len(ranks) == 0
    assert summary.interpolate(np.empty((3, 0, 4)), ilo, ihi, g).shape == (3, 0, 4)


# ---------------------------------------------------------------------------------------------------------------- selection
def host_order_stats(x, ranks, stride=1):
    x = np.ascontiguousarray(x, dtype=np.float64)
    ranks = np.ascontiguousarray(ranks, dtype=np.int64)
    n = len(range(0, len(x), stride))
    out = np.full(len(ranks), np.nan)
    assert _lib.load().emx_host_order_stats(x, n, stride, len(ranks), ranks, out) == 0
    return out


def same_bits_or_zeros(a, b):
    """array_equal (so that -0.0 == +0.0, as np.sort cannot tell them apart) and the same sign wherever the value is not 0"""
    return np.array_equal(a, b) and np.array_equal(np.signbit(a[a != 0]), np.signbit(b[b != 0]))


def selection_inputs():
    rs = np.random.RandomState(1)
    tiny = np.finfo(np.float64).tiny
    yield "mixed_signs", rs.randn(5000) * 3
    yield "ties", np.round(rs.randn(20000), 1)
    yield "zeros", np.array([0.0, -0.0, 1.0, -1.0, 0.0, -0.0, -0.0, 5e-324, -5e-324])
    yield "subnormals", np.concatenate([rs.randn(300) * tiny, rs.randint(-50, 50, size=300) * 5e-324, [tiny, -tiny]])
    yield "huge", np.concatenate([[1.79e308, -1.79e308, 1.79e308], rs.randn(100) * 1e307])
    yield "inf", np.array([np.inf, -np.inf, 0.5, -0.5, np.inf, 1e300, -np.inf])
    yield "n1", np.array([-7.5])
    yield "all_equal", np.full(1000, 0.1)
    yield "positive_close", 1e3 + 1e-9 * rs.randn(4000)


@pytest.mark.parametrize("name,x", list(selection_inputs()), ids=[n for n, _ in selection_inputs()])
def test_host_order_stats_equal_sorted_values(name, x):
    n = len(x)
    xs = np.sort(x)
    rs = np.random.RandomState(n)
    sets = [np.array([0]), np.array([n - 1]), np.arange(min(n, 32)), np.arange(max(n - 32, 0), n),
            rs.randint(0, n, size=32), np.sort(rs.randint(0, n, size=7))]
    if n >= 3:
        sets += [np.array([n // 2, n // 2 + 1, n // 2, 0, n - 1, n - 2, n - 1])]        # adjacent pairs, repeated ranks, unsorted
    for ranks in sets:
        got = host_order_stats(x, ranks)
        assert same_bits_or_zeros(got, xs[ranks]), (name, ranks)
    assert len(host_order_stats(x, np.array([], dtype=np.int64))) == 0


def test_host_order_stats_with_a_stride():
    rs = np.random.RandomState(2)
    x = np.round(rs.randn(3000), 2)
    for stride in (2, 5, 7):
        sel = np.sort(x[::stride])
        ranks = np.array([0, len(sel) - 1, len(sel) // 3, len(sel) // 3 + 1])
        assert np.array_equal(host_order_stats(x, ranks, stride), sel[ranks])


def test_host_order_stats_refuses_bad_arguments():
    lib = _lib.load()
    x, out = np.arange(4.0), np.zeros(33)
    r = lambda *v: np.array(v, dtype=np.int64)  # noqa: E731
    assert lib.emx_host_order_stats(x, 0, 1, 1, r(0), out) == -1
    assert lib.emx_host_order_stats(x, 4, 0, 1, r(0), out) == -1
    assert lib.emx_host_order_stats(x, 4, 1, 1, r(4), out) == -1
    assert lib.emx_host_order_stats(x, 4, 1, 1, r(-1), out) == -1
    assert lib.emx_host_order_stats(x, 4, 1, 33, np.zeros(33, dtype=np.int64), out) == -1
    assert lib.emx_host_order_stats(x, 4, 1, 2, r(3, 0), out) == 0 and out[0] == 3.0 and out[1] == 0.0
