"""PTSampler.get_evidence without a GPU: pt.stepping_stone_log_evidence (the host twin of emx_pt_evidence + the merge) against the
exact reference of tests/evidence_ref.py within the bounds its docstring derives, the estimator's calibration on independent exact
samples of a model whose evidence is known -- where thermodynamic integration is off by 0.28 -- and the plumbing: argument checks
before any device is touched, the call get_evidence makes, the build lists and the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import evidence_ref as er
from emcee_amd import EnsembleBatch, PTSampler, _build, _lib, pt, summary
from emcee_amd.pt import default_betas, stepping_stone_log_evidence
from emcee_amd.targets import BatchCallable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, T, NT, N = 2, 4, 37, 5


def gauss(q):
    return -0.5 * (q ** 2).sum(-1)


def ladder(T, ends_at_zero):
    return default_betas(T, 2, np.inf if ends_at_zero else None)


def draw(case, rs, shape=(G, T, NT, N)):
    L = -3.0 * rs.rand(*shape) ** 2 - rs.rand(*shape)
    if case == "offset":
        L = -1e6 + 2.0 * rs.rand(*shape) - 1.0
    elif case == "scattered -inf":
        L[:, -1][rs.rand(*L[:, -1].shape) < 0.3] = -np.inf
        L[0, 1, 5, 2] = -np.inf
    elif case == "a block of -inf":
        L[0, -1, NT - 9:] = -np.inf                     # K = 4: blocks of 9 rows, the last one whole
        L[1, 2, 1 + 9:1 + 18] = -np.inf                 # ... and the second of another rung
        L[1, -1] = -np.inf                              # every block of a rung
    elif case == "a NaN":
        L[0, 2, 20, 1] = np.nan
        L[1, -1, NT - 9:] = -np.inf
        L[1, -1, NT - 3, 0] = np.nan                    # among nothing but -inf
    return L


# ---------------------------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("case", ["plain", "offset", "scattered -inf", "a block of -inf", "a NaN"])
@pytest.mark.parametrize("ends_at_zero", [True, False])
def test_host_twin_against_the_exact_reference(case, ends_at_zero):
    rs = np.random.RandomState(len(case) + ends_at_zero)
    L, b = draw(case, rs), np.tile(ladder(T, ends_at_zero), (G, 1))
    b[1, 1:-1] *= 0.9                                    # every object its own ladder
    for K in (4, 1, 37):
        with np.errstate(all="raise", invalid="ignore", under="ignore"):
            ev = stepping_stone_log_evidence(b, L, nblocks=K)
        ref = er.exact(b, L, K)
        worst = er.check(ev, ref, "%s K=%d" % (case, K))
        print("%s, ladder ends at %s, K = %d: worst err / bound %s" % (case, "0" if ends_at_zero else "> 0", K,
                                                                        {k: "%.2g" % v for k, v in worst.items()}))
        assert np.array_equal(ev.betas, b) and ev.logz_ss.shape == (G,) and ev.log_ratios.shape == (G, T - 1)
        assert ev.block_logz_ss.shape == ev.block_logz_ti.shape == (G, K) and ev.mean_logl.shape == (G, T)
        if K == 1:
            assert np.isnan(ev.err_ss).all() and np.isnan(ev.err_ti).all()
        if case == "a block of -inf" and K == 4:
            assert ev.block_logz_ss[0, -1] == -np.inf and (ev.block_logz_ss[1] == -np.inf).all() and ev.logz_ss[1] == -np.inf
            assert ev.mean_logl[0, -1] == -np.inf and not np.isfinite(ev.logz_ti[0])
            assert np.isfinite(ev.logz_ss[0]) == ends_at_zero           # above 0 the tail extrapolates the hottest rung's mean, -inf
        if case == "a NaN" and K == 4:
            assert np.isnan(ev.logz_ss).all() and np.isfinite(ev.block_logz_ss[0, :2]).all() and np.isnan(ev.block_logz_ss[1, -1])


def test_one_rung_two_rungs_and_the_shapes_of_betas():
    rs = np.random.RandomState(3)
    L = draw("plain", rs, (3, 1, 12, 4))
    ev = stepping_stone_log_evidence(np.ones(1), L, nblocks=3)
    er.check(ev, er.exact(np.ones((3, 1)), L, 3), "T=1")
    assert ev.log_ratios.shape == (3, 0) and np.array_equal(ev.logz_ss, ev.tail) and np.array_equal(ev.tail, ev.mean_logl[:, 0])
    for b in (np.array([1.0, 0.0]), np.array([1.0, 0.25])):
        L = draw("plain", rs, (3, 2, 12, 4))
        ev = stepping_stone_log_evidence(b, L, nblocks=3)
        er.check(ev, er.exact(np.tile(b, (3, 1)), L, 3), "T=2")
        assert (ev.tail == 0).all() == (b[-1] == 0)
        one = stepping_stone_log_evidence(b, L[1], nblocks=3)                  # no leading axis: G = 1
        assert all(np.array_equal(np.asarray(u)[1:2], v, equal_nan=True) for u, v in zip(ev[:11], one[:11])) and one[11:] == ev[11:] == (3, 4)
    # the remainder is dropped at the early end
    L2 = L.copy()
    L2[:, :, :2] -= 100.0
    assert L.shape[2] % 5 == 2
    assert all(np.array_equal(u, v) for u, v in zip(stepping_stone_log_evidence(b, L, 5)[:11], stepping_stone_log_evidence(b, L2, 5)[:11]))
    for bad in (0, -1, 1.5, True, 13):
        with pytest.raises(ValueError, match="nblocks"):
            stepping_stone_log_evidence(b, L, nblocks=bad)
    with pytest.raises(ValueError, match="betas"):
        stepping_stone_log_evidence(np.ones(3), L)
    with pytest.raises(ValueError, match="shape"):
        stepping_stone_log_evidence(b, L[0, 0])


# ---------------------------------------------------------------------------------------------------------------- calibration
def test_calibration_on_exact_samples_where_thermodynamic_integration_fails():
    """Independent exact samples of the tempered model (no Markov chain): the 2-d unit Gaussian likelihood in the +-10 box,
    log Z = -2 log 20, on default_betas(6, 2, np.inf) with 8 192 samples a rung and 8 blocks.  Measured: bias 0.0026 against a
    standard error of 0.0021; spread across seeds 0.0164 against an rms block error of 0.0172; TI at -6.27."""
    exact, betas, n = -2.0 * np.log(20.0), default_betas(6, 2, np.inf), 8192
    logls = np.empty((64, 6, n // 8, 8))
    for i, seed in enumerate(range(100, 164)):
        rs = np.random.RandomState(seed)
        for t, beta in enumerate(betas):
            if beta == 0:
                x = rs.uniform(-10.0, 10.0, size=(n, 2))
            else:
                x = np.empty((0, 2))
                while len(x) < n:
                    y = rs.randn(n, 2) / np.sqrt(beta)
                    x = np.concatenate([x, y[(np.abs(y) <= 10.0).all(axis=1)]])[:n]
            logls[i, t] = (-0.5 * (x ** 2).sum(-1) - np.log(2.0 * np.pi)).reshape(n // 8, 8)
    ev = stepping_stone_log_evidence(betas, logls, nblocks=8)
    bias, spread = (ev.logz_ss - exact).mean(), ev.logz_ss.std(ddof=1)
    rms = np.sqrt((ev.err_ss ** 2).mean())
    print("bias %.4f +- %.4f, spread %.4f, rms block error %.4f, TI %.3f ... %.3f" % (bias, spread / 8.0, spread, rms, ev.logz_ti.min(),
                                                                                       ev.logz_ti.max()))
    assert abs(bias) <= 4.0 * spread / np.sqrt(64)
    assert 0.5 * spread <= rms <= 2.0 * spread
    assert (np.abs(ev.logz_ti - exact) > 0.2).all()


# ---------------------------------------------------------------------------------------------------------------- plumbing
def test_header_build_lists_and_exports():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "emx.h")).read(), flags=re.S)
    m = re.search(r"int\s+emx_pt_evidence\s*\(([^)]*)\)", txt)
    assert m and len(m.group(1).split(",")) == 13
    assert hasattr(_lib.load(), "emx_pt_evidence") and len(_lib.SIGNATURES["emx_pt_evidence"][1]) == 13
    assert any(s.endswith("emx_pt_evidence.hip") for s in _build.MORE_SRCS) and all(s in _build.DEPS for s in _build.MORE_SRCS)
    assert not any(s.endswith("emx_pt_evidence.hip") for s in _build.SRCS)
    assert summary.Evidence._fields == ("logz_ss", "err_ss", "logz_ti", "dlogz_ti", "err_ti", "log_ratios", "mean_logl", "tail", "block_logz_ss",
                                        "block_logz_ti", "betas", "nblocks", "block_length")
    assert "stepping_stone_log_evidence" in pt.__all__ and "Evidence" in summary.__all__
    for doc in (PTSampler.log_evidence_estimate.__doc__, PTSampler.mean_log_likelihood.__doc__):
        assert "get_evidence" in doc
    assert "M* = max_k M" in PTSampler.get_evidence.__doc__ and "M* = max_k M" in stepping_stone_log_evidence.__doc__


def test_the_library_refuses_a_null_handle_without_a_device():
    out = np.zeros(8)
    p = out.ctypes.data_as(C.c_void_p)
    assert _lib.load().emx_pt_evidence(None, 0, 1, 0, 4, 1, 2, p, p, p, p, p, None) == -1


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")
    monkeypatch.setattr(EnsembleBatch, "_handle", refuse)
    monkeypatch.setattr(EnsembleBatch, "_lib", refuse)


BOX = (np.full(2, -10.0), np.full(2, 10.0))


def test_bad_arguments_before_any_device(no_device):
    s = PTSampler(3, 16, 2, BatchCallable(gauss), log_prior=BOX, nbatch=2, seeds=[1, 2])
    for kw, match in (({"nblocks": 0}, "nblocks"), ({"nblocks": -2}, "nblocks"), ({"nblocks": 2.5}, "nblocks"), ({"nblocks": True}, "nblocks"),
                      ({"thin": 0}, "thin"), ({"thin": 1.5}, "thin"), ({"discard": -1}, "discard"), ({"discard": 0.5}, "discard")):
        with pytest.raises(ValueError, match=match):
            s.get_evidence(**kw)
    with pytest.raises(AttributeError, match="run the sampler"):
        s.get_evidence()
    flat = PTSampler(3, 16, 2, BatchCallable(gauss), nbatch=2, seeds=[1, 2])
    with pytest.raises(ValueError, match="normalised prior"):
        flat.get_evidence()
    with pytest.raises(ValueError, match="nblocks"):        # its arguments come first
        flat.get_evidence(nblocks=0)


class FakeLib(object):
    """emx_pt_evidence on host copies of the L plane (members, steps, N) and the beta plane (members, steps): the Python above the
    library runs as it does on a device"""

    def __init__(self, L, beta, T):
        self.L, self.beta, self.T, self.calls = L, beta, T, []

    def emx_pt_evidence(self, h, lo, hi, start, stop, stride, K, sum_L, amax, sexp, betas, changed, rows):
        self.calls.append((lo, hi, start, stop, stride, K))
        T = self.T
        L = self.L.reshape((-1, T) + self.L.shape[1:])[lo:hi, :, start:stop:stride]
        bt = self.beta.reshape((-1, T) + self.beta.shape[1:])[lo:hi, :, start:stop:stride]
        nt = L.shape[2]
        bl = nt // K
        x = L[:, :, nt - K * bl:].reshape(hi - lo, T, K, -1)
        used = bt[:, :, nt - K * bl:]
        b = used[:, :, 0]
        a = (b[:, :-1] - b[:, 1:])[:, :, None, None] * x[:, 1:]
        M = a.max(axis=-1)
        fill = lambda dst, src: C.memmove(dst, np.ascontiguousarray(src).ctypes.data, src.nbytes) if src.size else None  # noqa: E731
        fill(sum_L, x.sum(axis=-1))
        fill(amax, M)
        fill(sexp, np.exp(a - M[..., None]).sum(axis=-1))
        fill(betas, b)
        fill(changed, (used != used[:, :, :1]).any(axis=(1, 2)).astype(np.int32))
        rows._obj.value = bl
        return 0


def test_get_evidence_calls_the_library_on_the_selection_and_merges_like_the_twin(monkeypatch):
    objects, T, steps, N = 3, 4, 41, 6
    rs = np.random.RandomState(5)
    L = -3.0 * rs.rand(objects * T, steps, N)
    beta = np.repeat(np.tile(default_betas(T, 2, np.inf), objects)[:, None], steps, axis=1)
    beta[T + 1, :10] = 0.625                          # object 1's ladder moved over the first 10 stored steps
    s = PTSampler(T, N, 2, BatchCallable(gauss), log_prior=BOX, Tmax=np.inf, nbatch=objects, seeds=[1, 2, 3])
    lib = FakeLib(L, beta, T)
    monkeypatch.setattr(s, "_h", C.c_void_p(1))
    monkeypatch.setattr(EnsembleBatch, "iteration", property(lambda self: steps))
    monkeypatch.setattr(EnsembleBatch, "_lib", lambda self: lib)
    monkeypatch.setattr(EnsembleBatch, "close", lambda self: None)
    with pytest.raises(ValueError, match=r"object 1: the ladder changed.*Freeze adaptation \(adaptive = False\), run on, and discard the adaptive phase"):
        s.get_evidence()
    assert lib.calls == [(0, objects, 0, steps, 1, 8)]
    for kw in ({"discard": 10}, {"discard": 11, "thin": 3, "nblocks": 4}, {"discard": 3, "thin": 2, "nblocks": 1}):
        discard, thin, K = kw["discard"], kw.get("thin", 1), kw.get("nblocks", 8)
        if discard + thin - 1 < 10:
            with pytest.raises(ValueError, match="object 1"):           # K = 1 uses every selected row
                s.get_evidence(**kw)
            continue
        ev = s.get_evidence(**kw)
        start = discard + thin - 1
        assert lib.calls[-1] == (0, objects, start, steps, thin, K)
        ref = stepping_stone_log_evidence(beta.reshape(objects, T, steps)[:, :, -1],
                                          L.reshape(objects, T, steps, N)[:, :, start::thin], nblocks=K)
        assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(ev[:11], ref[:11])) and ev[11:] == ref[11:]
    n = len(lib.calls)
    for kw in ({"nblocks": steps + 1}, {"discard": steps - 3, "nblocks": 4}, {"discard": steps}):
        with pytest.raises(ValueError, match="nblocks"):
            s.get_evidence(**kw)
    assert len(lib.calls) == n
