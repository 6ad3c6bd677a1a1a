"""Fused user targets that sum over data (targets.DeviceFused(..., ndata=) / compile_fused_ensemble(..., data=True)), what needs no
GPU: hipcc cross-compiles the user's translation unit, the cache and the unchanged key of a data-free build, the compiler's
diagnostics, the launchers' host-only probe, the summation order on the host, the C ABI's declarations and the refusals made before
any device is touched."""
import ctypes as C
import hashlib
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import emcee_amd
from emcee_amd import EnsembleBatch, PTSampler, _lib
from emcee_amd.targets import (FUSED_FLAGS, DeviceFused, DeviceFusedLibrary, compile_fused_ensemble, fused_data_sum, get_include)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "emcee_amd", "csrc")
HEADER = os.path.join(CSRC, "emx_fused_ensemble_data.hpp")

# model (a) of tests/c/user_ensemble_fused_data.hip as a compile_fused_ensemble source
SOURCE = r"""
struct line_data { const double* d; long long n; double box; };
struct LineModel {
    __device__ double base(const double* x, int ndim, const void* user) const {
        const line_data* u = (const line_data*)user;
        for (int d = 0; d < ndim; ++d)
            if (!(x[d] >= -u->box && x[d] <= u->box)) return -__builtin_inf();
        return 0.0;
    }
    __device__ double term(const double* x, int ndim, long long k, const void* user) const {
        const line_data* u = (const line_data*)user;
        const double r = (u->d[u->n + k] - x[0] * u->d[k] - x[1]) / u->d[2 * u->n + k];
        return -0.5 * (r * r);
    }
};
extern "C" __attribute__((visibility("default"))) int line_data_bytes() { return (int)sizeof(line_data); }
"""
# the same model the way a user wrote it before: one lane loops over the data
PLAIN = r"""
struct line_data { const double* d; long long n; double box; };
struct LineLoop {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const {
        const line_data* u = (const line_data*)user;
        double acc = 0.0;
        for (long long k = 0; k < u->n; ++k) {
            const double r = (u->d[u->n + k] - x[0] * u->d[k] - x[1]) / u->d[2 * u->n + k];
            acc = acc + r * r;
        }
        return -0.5 * acc;
    }
};
"""


class Launch(C.Structure):          # emx_fused_ensemble_launch
    _fields_ = [("abi", C.c_uint32), ("args_bytes", C.c_uint32), ("ndim", C.c_int32), ("move", C.c_int32), ("grid", C.c_int32),
                ("threads", C.c_int32), ("lds_bytes", C.c_uint64), ("hip_stream", C.c_void_p), ("args", C.c_void_p),
                ("user", C.c_void_p)]


class DataLaunch(C.Structure):      # emx_fused_ensemble_data_launch
    _fields_ = Launch._fields_ + [("ndata", C.c_int64), ("rows", C.c_int32), ("reserved", C.c_int32)]


@pytest.fixture(scope="module")
def cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("fused_ens_data_cache"))


@pytest.fixture(scope="module")
def built(cache):
    return compile_fused_ensemble(SOURCE, "LineModel", 5, name="line5", cache_dir=cache, data=True)


@pytest.fixture(scope="module")
def plain(cache):
    return compile_fused_ensemble(PLAIN, "LineLoop", 5, name="loop5", cache_dir=cache)


def _exports(path):
    nm = shutil.which("nm")
    return subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout if nm else None


def test_compile_builds_caches_and_exports_the_data_launcher_alone(built, cache):
    assert isinstance(built, DeviceFusedLibrary) and built.ndim == 5 and built.name == "line5" and built.data and built.nblobs == 0
    assert os.path.exists(built.path) and built.path.startswith(cache)
    assert built.small_name is None and built.small_launcher is None
    out = _exports(built.path)
    if out is not None:
        assert re.search(r"\bT line5\b", out), out
        assert "_small" not in out
    assert hasattr(built.lib, "line5") and not hasattr(built.lib, "line5_small")
    assert built.lib.line_data_bytes() == 24          # the user's own extern "C" function of the source
    unit = open(os.path.join(os.path.dirname(built.path), "line5.hip")).read()
    assert unit.startswith("#include <emx_fused_ensemble_data.hpp>\n") and unit.rstrip().endswith("EMX_FUSED_ENSEMBLE_DATA_TARGET(line5, LineModel, 5)")
    mtime = os.stat(built.path).st_mtime_ns
    again = compile_fused_ensemble(SOURCE, "LineModel", 5, name="line5", cache_dir=cache, data=True)
    assert again.path == built.path and os.stat(again.path).st_mtime_ns == mtime      # nothing was compiled
    t = built.target(user=1 << 20, ndata=1000)
    assert isinstance(t, DeviceFused) and t.ndim == 5 and t.ndata == 1000 and t.nblobs == 0 and t.small_fn is None
    assert t.user_address() == 1 << 20 and t.kind == _lib.TARGET_FUSED_ENSEMBLE and t.fn_ptr is built.launcher


def test_a_model_without_term_raises_with_the_compilers_diagnostic(cache):
    src = "struct NoTerm { __device__ double base(const double*, int, const void*) const { return 0.0; } };"
    with pytest.raises(RuntimeError) as e:
        compile_fused_ensemble(src, "NoTerm", 5, cache_dir=cache, data=True)
    assert "error:" in str(e.value) and "hipcc failed" in str(e.value) and "term" in str(e.value)
    with pytest.raises(ValueError) as e:
        compile_fused_ensemble(SOURCE, "LineModel", 5, cache_dir=cache, data=True, nblobs=2)
    assert "blobs" in str(e.value)


def test_a_data_free_build_keeps_its_cache_key_and_translation_unit(plain, cache):
    """the key computed the way the library computed it before `data` existed: the directory is the one the build landed in"""
    from emcee_amd import _build
    name, small_name = "loop5", "loop5_small"
    key = ("ensemble", PLAIN, "LineLoop", 5, name)
    h = hashlib.sha256(repr(key + (FUSED_FLAGS + [],)).encode())
    for d in _build.DEPS:
        if d.endswith((".hpp", ".h")):
            with open(d, "rb") as f:
                h.update(f.read())
    work = os.path.join(cache, h.hexdigest()[:24])
    assert plain.path == os.path.join(work, "lib%s.so" % name) and not plain.data
    unit = open(os.path.join(work, "%s.hip" % name)).read()
    assert unit == "#include <emx_fused_ensemble.hpp>\n\n%s\n\nEMX_FUSED_ENSEMBLE_TARGET(%s, LineLoop, 5)\nEMX_FUSED_ENSEMBLE_SMALL_TARGET(%s, LineLoop, 5)\n" % (
        PLAIN, name, small_name)
    assert plain.small_name == small_name and plain.small_launcher is not None
    assert HEADER in _build.DEPS                      # the new header is part of every key, as every header is


def _abi(header, name):
    return int(re.search(r"#define %s (0x[0-9a-fA-F]+|\d+)u" % name, open(os.path.join(CSRC, header)).read()).group(1), 0)


def test_the_probes_refuse_each_others_descriptor(built, plain):
    """grid == 0 launches nothing, so the probe runs without a GPU: 0 for exactly one args_bytes (sizeof(HalfStepArgs) is internal),
    1 for another ABI value -- the data-free launcher's among them --, 2 for another ndim"""
    abi_d, abi_f = _abi("emx_fused_ensemble_data.hpp", "EMX_FUSED_ENSEMBLE_DATA_ABI"), _abi("emx_fused_ensemble.hpp", "EMX_FUSED_ENSEMBLE_ABI")
    others = [_abi("emx_fused_ensemble.hpp", n) for n in ("EMX_FUSED_ENSEMBLE_BLOBS_ABI", "EMX_FUSED_ENSEMBLE_SMALL_ABI")]
    assert len({abi_d, abi_f} | set(others)) == 4
    fd, ff = built.launcher, plain.launcher
    fd.restype, fd.argtypes = C.c_int, [C.POINTER(DataLaunch)]
    ff.restype, ff.argtypes = C.c_int, [C.POINTER(DataLaunch)]          # (the larger struct: its leading fields are the data-free one's)
    rcs = [fd(C.byref(DataLaunch(abi=abi_d, args_bytes=n, ndim=5, move=0, grid=0))) for n in range(8, 4096, 8)]
    assert sorted(set(rcs)) == [0, 1] and rcs.count(0) == 1
    nbytes = 8 * (rcs.index(0) + 1)
    assert fd(C.byref(DataLaunch(abi=abi_d + 1, args_bytes=nbytes, ndim=5, move=0, grid=0))) == 1
    assert fd(C.byref(DataLaunch(abi=abi_d, args_bytes=nbytes, ndim=6, move=0, grid=0))) == 2
    for move in (0, 1, 2, 3, 4):                      # stretch, DE, snooker, Gaussian, evaluate rows
        assert fd(C.byref(DataLaunch(abi=abi_d, args_bytes=nbytes, ndim=5, move=move, grid=0))) == 0
    assert fd(C.byref(DataLaunch(abi=abi_d, args_bytes=nbytes, ndim=5, move=5, grid=0))) == 3
    # each launcher answers 1 to the other's descriptor; the data-free one takes its own with the same args_bytes
    for other in [abi_f] + others:
        assert fd(C.byref(DataLaunch(abi=other, args_bytes=nbytes, ndim=5, move=0, grid=0))) == 1
    assert ff(C.byref(DataLaunch(abi=abi_d, args_bytes=nbytes, ndim=5, move=0, grid=0))) == 1
    assert ff(C.byref(DataLaunch(abi=abi_f, args_bytes=nbytes, ndim=5, move=0, grid=0))) == 0
    # a launch (grid != 0) with rows a workgroup or a count of data out of range is refused before anything is launched
    for kw in (dict(rows=3), dict(rows=65), dict(rows=16, ndata=-1), dict(rows=16, ndata=2 ** 31)):
        assert fd(C.byref(DataLaunch(abi=abi_d, args_bytes=nbytes, ndim=5, move=0, grid=8, threads=256, lds_bytes=1 << 16, **kw))) == 3


def _two_loops(t):
    """the order as the header states it"""
    p = [0.0] * 64
    for lane in range(64):
        for k in range(lane, len(t), 64):
            p[lane] = p[lane] + float(t[k])
    while len(p) > 1:
        p = [p[2 * i] + p[2 * i + 1] for i in range(len(p) // 2)]
    return p[0]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_fused_data_sum_is_the_stated_order(n):
    rs = np.random.RandomState(100 + n)
    t = rs.randn(n) * 10.0 ** rs.uniform(-6, 6, n)
    got = fused_data_sum(t)
    assert isinstance(got, float) and got == _two_loops(t)
    assert fused_data_sum(list(t)) == got
    # terms of one sign: a term goes through at most ceil(n / 64) additions in its lane and six in the tree, each with a relative
    # error of at most 2^-53 (half an ulp) of a partial sum that is no larger than the total; fsum itself rounds once
    benign = -0.5 * rs.randn(n) ** 2
    exact = math.fsum(benign)
    assert abs(fused_data_sum(benign) - exact) <= ((n + 63) // 64 + 6 + 1) * np.spacing(abs(exact))


def test_fused_data_sum_is_not_numpys_order():
    """large cancelling terms a lane stride apart: they cancel exactly inside lane 0's partial, and nowhere in a sum that runs along the array"""
    t = np.full(128, 1.0)
    t[0], t[64] = 1e17, -1e17                         # lane 0: (0 + 1e17) - 1e17 = 0 exactly; every other lane: 1 + 1 = 2
    assert fused_data_sum(t) == 126.0 == _two_loops(t)
    assert float(np.sum(t)) != 126.0 and float(np.add.reduce(t)) != 126.0      # 1e17 swallows the ones next to it
    with pytest.raises(ValueError):
        fused_data_sum(np.zeros((2, 3)))
    assert fused_data_sum([]) == 0.0 and math.copysign(1.0, fused_data_sum([])) == 1.0


def test_argument_checks_and_refusals_touch_no_device(built, plain):
    with pytest.raises(ValueError) as e:
        DeviceFused(0x1000, 5, ndata=10, nblobs=2)
    assert "ndata" in str(e.value) and "blobs" in str(e.value)
    with pytest.raises(ValueError) as e:
        DeviceFused(0x1000, 5, ndata=10, small_fn=0x2000)
    assert "ndata" in str(e.value) and "small_fn" in str(e.value)
    for bad in (-1, 2 ** 31, 10.0, "10", True):
        with pytest.raises(ValueError) as e:
            DeviceFused(0x1000, 5, ndata=bad)
        assert "ndata" in str(e.value)
    assert DeviceFused(0x1000, 5, ndata=0).ndata == 0 and DeviceFused(0x1000, 5, ndata=np.int64(7)).ndata == 7
    assert DeviceFused(0x1000, 5).ndata is None
    with pytest.raises(ValueError) as e:
        built.target(user=None)
    assert "ndata" in str(e.value) and "data=True" in str(e.value)
    with pytest.raises(ValueError) as e:
        plain.target(user=None, ndata=10)
    assert "ndata" in str(e.value) and "data=True" in str(e.value)
    t = DeviceFused(0x1000, 5, ndata=10)
    with pytest.raises(TypeError) as e:
        EnsembleBatch(4, 32, 5, t)
    assert "DeviceFused" in str(e.value) and "EnsembleSampler" in str(e.value)
    with pytest.raises(TypeError) as e:
        PTSampler(4, 16, 5, t, nbatch=2)
    assert "DeviceFused" in str(e.value)
    with pytest.raises(ValueError) as e:
        emcee_amd.EnsembleSampler(32, 5, t, distributed=True)
    assert "DeviceFused" in str(e.value) and "distributed" in str(e.value)
    from emcee_amd.device import DeviceEnsemble
    nothing = object.__new__(DeviceEnsemble)          # no context, no library: the check comes first
    for bad in (-1, 1, 3, 257, 1 << 20):
        with pytest.raises(ValueError) as e:
            nothing.set_tuning("fused_data_rows", bad)
        assert "fused_data_rows" in str(e.value)
    s = emcee_amd.EnsembleSampler(32, 5, t)           # accepted, and still no device touched
    assert s._ens is None and s._device_target is t


def test_header_declares_the_data_abi():
    raw = open(os.path.join(ROOT, "include", "emx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    body = re.search(r"typedef\s+struct\s+emx_fused_ensemble_data_launch\s*\{([^}]*)\}\s*emx_fused_ensemble_data_launch\s*;", txt)
    assert body
    names = re.findall(r"\b(\w+)\s*[;,]", body.group(1))
    assert names == ["abi", "args_bytes", "ndim", "move", "grid", "threads", "lds_bytes", "hip_stream", "args", "user", "ndata", "rows", "reserved"]
    assert [n for n, _ in DataLaunch._fields_] == names and [n for n, _ in _lib.FusedEnsembleDataLaunch._fields_] == names
    assert C.sizeof(_lib.FusedEnsembleDataLaunch) == C.sizeof(DataLaunch) == 72
    assert re.search(r"typedef\s+int\s*\(\s*\*\s*emx_fused_ensemble_data_fn\s*\)\s*\(\s*const\s+emx_fused_ensemble_data_launch\s*\*\s*\)\s*;", txt)
    assert re.search(r"int\s+emx_set_target_fused_data\s*\(\s*emx_ctx\s*\*\s*\w*\s*,\s*emx_fused_ensemble_data_fn\s+\w+\s*,\s*const\s+void\s*\*\s*\w+\s*,"
                     r"\s*int64_t\s+\w+\s*\)\s*;", txt)
    lib = _lib.load()
    assert hasattr(lib, "emx_set_target_fused_data") and "emx_set_target_fused_data" in _lib.SIGNATURES
    assert _lib.SIGNATURES["emx_set_target_fused_data"][1][-1] is C.c_int64


def test_the_test_models_compile(tmp_path):
    """tests/c/user_ensemble_fused_data.hip (the GPU tests' models, every wrapping of each) cross-compiles and exports its entry points"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    so = str(tmp_path / "libuser_ens_data.so")
    subprocess.run([hipcc] + FUSED_FLAGS + ["-DUSER_NDIM=3"] + ["-I" + d for d in get_include()] +
                   [os.path.join(ROOT, "tests", "c", "user_ensemble_fused_data.hip"), "-o", so], check=True, timeout=900, capture_output=True)
    _lib.load()
    user = C.CDLL(so)
    for name in ("user_data_a", "user_data_b", "user_data_c", "user_data_d", "user_serial_a", "user_rows_a", "user_rows_b", "user_rows_c",
                 "user_rows_d", "user_setup", "user_device_pointer", "user_teardown"):
        assert hasattr(user, name)
