"""EnsembleBatch.get_autocorr_time(on_device=True) without a GPU: the C ABI of emx_autocorr_batch, the tuning key, and the
argument checks that must fire before any device is touched."""
import os
import re

import numpy as np
import pytest

from emcee_amd import EnsembleBatch, _lib, targets
from emcee_amd.batch import _check_tol
from emcee_amd.autocorr import AutocorrError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    """any attempt to create the device handle or to call the library fails the test"""
    def refuse(self):
        raise AssertionError("a device was touched before the arguments were checked")
    monkeypatch.setattr(EnsembleBatch, "_handle", refuse)
    monkeypatch.setattr(EnsembleBatch, "_lib", refuse)


def header_text():
    return open(os.path.join(ROOT, "include", "emx.h")).read()


def test_header_declares_and_library_exports_the_entry_point():
    txt = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    m = re.search(r"int\s+emx_autocorr_batch\s*\(([^)]*)\)", txt)
    assert m, "include/emx.h does not declare emx_autocorr_batch"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [p.rsplit(None, 1)[0].replace(" *", "*") for p in params] == [
        "emx_batch*", "int32_t", "int32_t", "int64_t", "int64_t", "double", "double*", "int32_t*", "int64_t*"], params
    lib = _lib.load()
    assert hasattr(lib, "emx_autocorr_batch")
    res, args = _lib.SIGNATURES["emx_autocorr_batch"]
    assert res is _lib.C.c_int and len(args) == 9
    assert '"batch_acf_series"' in header_text()


def test_build_compiles_the_new_translation_unit():
    from emcee_amd import _build
    assert any(s.endswith("emx_batch_acf.hip") for s in _build.SRCS)


def test_bad_arguments_before_any_device(no_device):
    bt = EnsembleBatch(3, 16, 2, targets.IsoGaussian(), seeds=[1, 2, 3])
    with pytest.raises(ValueError, match="run the sampler"):
        bt.get_autocorr_time(on_device=True)
    with pytest.raises(ValueError, match="run the sampler"):
        bt[1].get_autocorr_time(on_device=True)
    for thin in (0, -1, 1.5):
        with pytest.raises(ValueError, match="thin"):
            bt.get_autocorr_time(thin=thin, on_device=True)
        with pytest.raises(ValueError, match="thin"):
            bt[2].get_autocorr_time(thin=thin, on_device=True)
    for discard in (-1, 0.5):
        with pytest.raises(ValueError, match="discard"):
            bt.get_autocorr_time(discard=discard, on_device=True)
    with pytest.raises(ValueError, match="members"):
        bt._autocorr_device(lo=2, hi=2)
    with pytest.raises(ValueError, match="members"):
        bt._autocorr_device(lo=0, hi=4)


def test_tol_rule_names_the_flagged_members(caplog):
    tau = np.array([[1.0, 2.0], [30.0, 1.0], [np.nan, 1.0], [1.0, 26.0]])
    _check_tol(tau, 2000, 50, False, [0, 1, 2, 3], tau)          # 50 tau < 2000 everywhere, NaN is never flagged
    with pytest.raises(AutocorrError, match=r"2 parameter\(s\) of members 1, 3\.") as e:
        _check_tol(tau, 1000, 40, False, [0, 1, 2, 3], tau)
    assert e.value.tau is tau and "N/40 = 25" in str(e.value)
    with caplog.at_level("WARNING", logger="emcee_amd.autocorr"):
        _check_tol(tau, 1000, 40, True, [0, 1, 2, 3], tau)
    assert "members 1, 3" in caplog.text
    many = np.full((12, 1), 10.0)
    with pytest.raises(AutocorrError, match="members 0, 1, 2, 3, 4, 5, 6, 7 and 4 more"):
        _check_tol(many, 100, 50, False, list(range(12)), many)
    with pytest.raises(AutocorrError, match=r"of member 5\.") as e:
        _check_tol(many[:1], 100, 50, False, [5], many[0])
    assert e.value.tau.shape == (1,)
