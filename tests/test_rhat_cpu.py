"""Split-R-hat without a GPU: summary.split_rhat against the definition in exact rational arithmetic, the error bounds of
tests/rhat_ref.py (its docstring derives them) held by a NumPy transcription of the kernels' arithmetic and broken by the one-pass
form, power-of-two covariance, the argument checks that must fire before any device is touched, the shapes every class returns,
and the host-chain path of Backend.get_rhat."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import chain_families as cf
import rhat_ref as rr
from emcee_amd import EnsembleBatch, EnsembleSampler, PTSampler, _lib, device, summary, targets
from emcee_amd.backends import Backend
from emcee_amd.state import State
from emcee_amd.targets import BatchCallable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NTS, WALKERS, DIMS = (4, 5, 37), (2, 7), (1, 3)
B = 3                                       # ensembles of the 4-d arrays


def walk(name, nt, N, D, seed=0, members=None):
    """-> (x (nt, [members,] N, D), lp without the last axis, family): start_cloud plus a seeded random walk whose steps are
    0.25 ... 0.75 sd long; the scaled family's array is the centred family's times the scale, bit for bit"""
    fam = cf.family(name, D, seed)
    shape = (N,) if members is None else (members, N)
    rs = np.random.RandomState(seed + 7)
    start = cf.start_cloud(fam, shape, seed + 1)
    steps = rs.choice([-1.0, 1.0], size=(nt,) + shape + (D,)) * (0.25 + 0.5 * rs.rand(*((nt,) + shape + (D,))))
    pos = np.cumsum(steps, axis=0)
    x = start + ((fam["sd"] / fam["scale"]) * pos) * fam["scale"]
    return x, -0.5 * (pos * pos).sum(axis=-1), fam


def test_header_declares_and_library_exports_the_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "emx.h")).read(), flags=re.S)
    for name, nargs in (("emx_rhat_batch", 12), ("emx_rhat", 9)):
        m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, txt)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert hasattr(_lib.load(), name) and len(_lib.SIGNATURES[name][1]) == nargs
    assert '"batch_rhat_members"' in open(os.path.join(ROOT, "include", "emx.h")).read()
    from emcee_amd import _build
    assert any(s.endswith("emx_rhat.hip") for s in _build.MORE_SRCS) and all(s in _build.DEPS for s in _build.MORE_SRCS)
    assert summary.RHat._fields == ("rhat", "within", "between", "nchains", "length")


# ---------------------------------------------------------------------------------------------------------------- the definition
def check_against_fractions(r, z, what):
    out = rr.check(r, z, what)
    h = r.length
    assert np.array_equal(r.rhat, np.sqrt((h - 1) / h + r.between / r.within)), what
    return out


@pytest.mark.parametrize("name", cf.FAMILIES)
@pytest.mark.parametrize("nt", NTS)
def test_split_rhat_against_exact_rational_arithmetic(nt, name):
    for N in WALKERS:
        for D in DIMS:
            x, lp, _ = walk(name, nt, N, D, seed=nt + N + D)
            xb, lpb, _ = walk(name, nt, N, D, seed=nt + N + D, members=B)
            for with_lp in (False, True):
                what = "%s nt=%d %dx%d lp=%s" % (name, nt, N, D, with_lp)
                r = summary.split_rhat(x, log_prob=lp if with_lp else None)
                assert r.rhat.shape == (D + with_lp,)
                check_against_fractions(r, rr.chains_of(x, lp if with_lp else None), what)
                for pool in (False, True):
                    r = summary.split_rhat(xb, log_prob=lpb if with_lp else None, pool=pool)
                    assert r.rhat.shape == ((D + with_lp,) if pool else (B, D + with_lp))
                    check_against_fractions(r, rr.chains_of(xb, lpb if with_lp else None, pool=pool), what + " pool=%s" % pool)
            if nt % 2:
                # the middle sample belongs to neither half
                y = x.copy()
                y[nt // 2] += 1000.0 * (1.0 + np.abs(y[nt // 2]))
                a, b = summary.split_rhat(x), summary.split_rhat(y)
                assert all(np.array_equal(u, v) for u, v in zip(a, b)), (name, nt)
                y = x.copy()
                y[nt // 2 - 1] *= 3.0                       # ... and its neighbour does belong to one
                assert not np.array_equal(summary.split_rhat(y).within, a.within)


# ---------------------------------------------------------------------------------------------------------------- the bounds
@pytest.mark.parametrize("name", cf.FAMILIES)
def test_the_kernels_arithmetic_holds_the_bounds_and_one_pass_sums_break_them(name):
    worst = {"kernel": [0.0, 0.0], "one_pass": [0.0, 0.0]}
    for nt, N, D in ((4, 2, 1), (5, 7, 3), (37, 7, 3), (37, 2, 1)):
        xb, lpb, _ = walk(name, nt, N, D, seed=nt + N, members=B)
        for pool in (False, True):
            z = rr.chains_of(xb, lpb, pool=pool)
            G, Cn, h, W = z.shape
            ex = rr.exact(z)
            assert rr.regime_ratio(ex, Cn).max() <= 1
            for key, fn in (("kernel", rr.kernel_arithmetic), ("one_pass", rr.one_pass)):
                rw, rb = rr.ratios(*fn(z), ex, Cn, h)
                if key == "one_pass":
                    rw, rb = rw[:, :D], rb[:, :D]           # the log-prob column is near the origin in every family
                worst[key] = [max(worst[key][0], rw.max()), max(worst[key][1], rb.max())]
    print("%s: worst err / bound -- kernel arithmetic: within %.3g, between %.3g; one pass: within %.3g, between %.3g"
          % ((name,) + tuple(worst["kernel"]) + tuple(worst["one_pass"])))
    assert max(worst["kernel"]) <= 1, worst
    if name in ("offset_34", "offset_40"):
        assert min(worst["one_pass"]) > 1, worst


# ---------------------------------------------------------------------------------------------------------------- scale covariance
@pytest.mark.parametrize("nt,N,D", [(5, 2, 1), (37, 7, 3), (36, 7, 5)])
def test_power_of_two_covariance(nt, N, D):
    (xa, _, _), (xb, _, fam) = walk("centred", nt, N, D, members=B), walk("scaled", nt, N, D, members=B)
    sc = fam["scale"]
    assert np.array_equal(np.log2(sc), cf.scale_exponents(D)) and np.array_equal(xa * sc, xb)      # the premise
    for arrays, kw in (((xa[:, 0], xb[:, 0]), {}), ((xa, xb), {"pool": False}), ((xa, xb), {"pool": True})):
        a, b = summary.split_rhat(arrays[0], **kw), summary.split_rhat(arrays[1], **kw)
        assert np.array_equal(a.rhat, b.rhat) and np.isfinite(a.rhat).all()
        assert np.array_equal(a.within * sc * sc, b.within) and np.array_equal(a.between * sc * sc, b.between)


# ---------------------------------------------------------------------------------------------------------------- arguments, shapes
STEPS, N, D = 13, 8, 3


def filled_backend(x, lp):
    b = Backend()
    b.reset(x.shape[1], x.shape[2])
    b.grow(len(x), None)
    for t in range(len(x)):
        b.save_step(State(x[t], log_prob=lp[t]), np.ones(x.shape[1], dtype=bool))
    return b


class FakeLib(object):
    """emx_rhat_batch on a host copy of a member-major chain (members, steps, N, D): the Python layers above the library run as
    they do on a device"""

    def __init__(self, chain, lp):
        self.chain, self.lp, self.calls = chain, lp, []

    def emx_rhat_batch(self, h, lo, hi, pool, start, stop, stride, log_prob, within, between, nc, length):
        self.calls.append((lo, hi, pool, start, stop, stride, log_prob))
        x = self.chain[lo:hi, start:stop:stride]
        lp = self.lp[lo:hi, start:stop:stride] if log_prob else None
        G, W = (pool if pool else hi - lo), x.shape[-1] + (1 if log_prob else 0)
        for g in range(G):
            sel = slice(g, None, pool) if pool else slice(g, g + 1)
            r = summary.split_rhat(x[sel].transpose(1, 0, 2, 3), None if lp is None else lp[sel].transpose(1, 0, 2), pool=True)
            for dst, src in ((within, r.within), (between, r.between)):
                (C.c_double * W).from_address(dst.value + g * W * 8)[:] = src.tolist()
        nc._obj.value, length._obj.value = r.nchains, r.length
        return 0


@pytest.fixture
def stored_batch(monkeypatch):
    """-> make(sampler, members): the sampler behaves as if `members` ensembles of STEPS x N x D were stored, with FakeLib below"""
    def make(obj, members, steps=STEPS):
        rs = np.random.RandomState(members)
        lib = FakeLib(rs.randn(members, steps, N, D), rs.randn(members, steps, N))
        bt = obj if isinstance(obj, EnsembleBatch) else obj._b
        monkeypatch.setattr(bt, "_h", C.c_void_p(1))
        monkeypatch.setattr(EnsembleBatch, "iteration", property(lambda self: steps))
        monkeypatch.setattr(EnsembleBatch, "_lib", lambda self: lib)
        monkeypatch.setattr(EnsembleBatch, "close", lambda self: None)
        return lib
    return make


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")
    monkeypatch.setattr(device.DeviceEnsemble, "__init__", refuse)      # (constructors check shapes with the library's host entry points)
    monkeypatch.setattr(device.DeviceEnsemble, "rhat", refuse)
    monkeypatch.setattr(EnsembleBatch, "_handle", refuse)
    monkeypatch.setattr(EnsembleBatch, "_lib", refuse)


def bad_argument_cases(get, stored, members_ok):
    for thin in (0, -1, 1.5):
        with pytest.raises(ValueError, match="thin"):
            get(thin=thin)
    for discard in (-1, 0.5):
        with pytest.raises(ValueError, match="discard"):
            get(discard=discard)
    for chains in ("chains", None, 1) + (() if members_ok else ("members",)):
        with pytest.raises(ValueError, match="chains"):
            get(chains=chains)
    if stored:
        for kw in ({"discard": stored - 3}, {"discard": stored}, {"thin": stored // 3}, {"discard": 2, "thin": 4}):
            nt = len(range(min(kw.get("discard", 0) + kw.get("thin", 1) - 1, stored), stored, kw.get("thin", 1)))
            assert nt < 4
            with pytest.raises(ValueError, match="at least 4|select none"):
                get(**kw)


def test_bad_arguments_before_any_device(no_device):
    s = EnsembleSampler(16, 2, targets.IsoGaussian())
    with pytest.raises(AttributeError, match="run the sampler"):
        s.get_rhat()
    bad_argument_cases(s.get_rhat, 0, False)
    rs = np.random.RandomState(0)
    b = filled_backend(rs.randn(STEPS, N, D), rs.randn(STEPS, N))
    bad_argument_cases(b.get_rhat, STEPS, False)
    bt = EnsembleBatch(3, 16, 2, targets.IsoGaussian(), seeds=[1, 2, 3])
    for get, members_ok in ((bt.get_rhat, True), (bt[1].get_rhat, False)):
        with pytest.raises(ValueError, match="run the sampler"):
            get()
        bad_argument_cases(get, 0, members_ok)
    pt = PTSampler(3, 16, 2, BatchCallable(lambda q: -0.5 * (q ** 2).sum(-1)), nbatch=2, seeds=[1, 2])
    with pytest.raises(ValueError, match="run the sampler"):
        pt.get_rhat()
    bad_argument_cases(pt.get_rhat, 0, True)
    for x in (np.zeros((3, 4, 2)), np.zeros((3, 2, 4, 2))):
        with pytest.raises(ValueError, match="at least 4"):
            summary.split_rhat(x)
    with pytest.raises(ValueError, match="pool"):
        summary.split_rhat(np.zeros((8, 4, 2)), pool=True)
    with pytest.raises(ValueError, match="shape"):
        summary.split_rhat(np.zeros((8, 4)))
    with pytest.raises(ValueError, match="log_prob"):
        summary.split_rhat(np.zeros((8, 4, 2)), log_prob=np.zeros((8, 3)))


def test_short_selections_raise_on_a_stored_batch_before_the_library_is_called(stored_batch):
    bt = EnsembleBatch(3, N, D, targets.IsoGaussian(), seeds=[1, 2, 3])
    lib = stored_batch(bt, 3)
    for get, members_ok in ((bt.get_rhat, True), (bt[2].get_rhat, False)):
        bad_argument_cases(get, STEPS, members_ok)
    assert lib.calls == []


def test_output_shapes_of_every_class(stored_batch):
    rs = np.random.RandomState(1)
    b = filled_backend(rs.randn(STEPS, N, D), rs.randn(STEPS, N))
    for lp in (False, True):
        r = b.get_rhat(discard=1, log_prob=lp)
        assert isinstance(r, summary.RHat) and (r.nchains, r.length) == (2 * N, 6)
        assert all(a.shape == (D + lp,) for a in r[:3])
    bt = EnsembleBatch(4, N, D, targets.IsoGaussian(), seeds=[1, 2, 3, 4])
    lib = stored_batch(bt, 4)
    for lp in (False, True):
        r = bt.get_rhat(discard=1, log_prob=lp)
        assert all(a.shape == (4, D + lp) for a in r[:3]) and (r.nchains, r.length) == (2 * N, 6)
        one = bt[2].get_rhat(discard=1, log_prob=lp)
        assert all(a.shape == (D + lp,) and np.array_equal(a, f[2]) for a, f in zip(one[:3], r[:3])) and one[3:] == r[3:]
        pooled = bt.get_rhat(discard=1, chains="members", log_prob=lp)
        assert all(a.shape == (D + lp,) for a in pooled[:3]) and (pooled.nchains, pooled.length) == (4 * 2 * N, 6)
        ref = summary.split_rhat(lib.chain[:, 1:].transpose(1, 0, 2, 3), lib.lp[:, 1:].transpose(1, 0, 2) if lp else None, pool=True)
        assert all(np.array_equal(u, v) for u, v in zip(pooled, ref))
    assert lib.calls[0] == (0, 4, 0, 1, STEPS, 1, 0) and lib.calls[1][:3] == (2, 3, 0) and lib.calls[2][:3] == (0, 4, 1)
    # PTSampler: member m = object x ntemps + rung; "members" pools every rung over the objects
    T, objects = 3, 2
    pt = PTSampler(T, N, D, BatchCallable(lambda q: -0.5 * (q ** 2).sum(-1)), nbatch=objects, seeds=[1, 2])
    lib = stored_batch(pt, T * objects)
    for lp in (False, True):
        r = pt.get_rhat(thin=2, log_prob=lp)
        assert all(a.shape == (objects, T, D + lp) for a in r[:3]) and (r.nchains, r.length) == (2 * N, 3)
        pooled = pt.get_rhat(thin=2, chains="members", log_prob=lp)
        assert all(a.shape == (T, D + lp) for a in pooled[:3]) and (pooled.nchains, pooled.length) == (objects * 2 * N, 3)
        for t in range(T):
            x = lib.chain[t::T, 1::2].transpose(1, 0, 2, 3)
            ref = summary.split_rhat(x, lib.lp[t::T, 1::2].transpose(1, 0, 2) if lp else None, pool=True)
            assert all(np.array_equal(u[t], v) for u, v in zip(pooled[:3], ref[:3]))
            own = summary.split_rhat(x, pool=False)
            np.testing.assert_allclose(r.within[:, t, :D], own.within, rtol=1e-13)       # NumPy's order may differ with the shape
    assert lib.calls[0][:3] == (0, T * objects, 0) and lib.calls[1][:3] == (0, T * objects, T)


def test_constant_columns_and_minus_infinity_give_nan_not_an_exception():
    rs = np.random.RandomState(2)
    x, lp = rs.randn(STEPS, N, D), rs.randn(STEPS, N)
    x[:, :, 1] = 0.1                                    # a constant that no sum of copies reproduces exactly
    lp[4, 3] = -np.inf
    with np.errstate(all="raise"):
        r = summary.split_rhat(x, log_prob=lp)
    assert np.isnan(r.rhat[1]) and r.within[1] == 0 and r.between[1] == 0
    assert np.isnan(r.rhat[D]) and np.isfinite(r.rhat[[0, 2]]).all()
    b = filled_backend(x, lp)
    with np.errstate(all="raise"):
        got = b.get_rhat(log_prob=True)
    assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(got[:3], r[:3]))
    x[5, 2, 0] = np.nan
    assert np.isnan(summary.split_rhat(x).rhat[:2]).all() and np.isfinite(summary.split_rhat(x).rhat[2])
    pooled = summary.split_rhat(np.stack([x, x + 1.0], axis=1), pool=True)
    assert np.isnan(pooled.rhat[0]) and pooled.within[1] == 0 and pooled.between[1] > 0 and pooled.rhat[1] == np.inf


# ---------------------------------------------------------------------------------------------------------------- the host path
@pytest.mark.parametrize("discard,thin", [(0, 1), (5, 3), (2, 2)])
def test_host_backend_returns_split_rhats_tuple(discard, thin):
    x, lp, _ = walk("offset_20", 37, 6, 3)
    b = filled_backend(x, lp)
    assert b._dev is None
    for with_lp in (False, True):
        got = b.get_rhat(discard=discard, thin=thin, log_prob=with_lp)
        ref = summary.split_rhat(b.get_chain(discard=discard, thin=thin),
                                 log_prob=b.get_log_prob(discard=discard, thin=thin) if with_lp else None)
        assert isinstance(got, summary.RHat) and got[3:] == ref[3:] == (12, len(range(discard + thin - 1, 37, thin)) // 2)
        assert all(np.array_equal(u, v) for u, v in zip(got[:3], ref[:3]))
