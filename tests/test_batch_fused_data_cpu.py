"""Fused user targets of EnsembleBatch that sum over per-member data (targets.BatchFused(..., ndata=) / compile_fused(..., data=True);
emx_fused_target_data.hpp), what needs no GPU: hipcc cross-compiles the user's translation unit, the launcher answers the grid = 0
probe, the compiler's diagnostics, the C ABI's declarations and the argument checks made before any device is touched."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from emcee_amd import EnsembleBatch, PTSampler, _lib
from emcee_amd.targets import BatchFused, BatchFusedLibrary, compile_fused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "emcee_amd", "csrc")

# a straight-line fit: the record of a member, the model with base and term, and the same inline functions as a one-lane functor
SOURCE = r"""
struct line_rec { const double* x; const double* y; const double* ivar; };
__device__ inline double line_base(const double* th, int ndim) {
    double acc = 0.0;
    for (int d = 0; d < ndim; ++d) acc = acc + th[d] * th[d];
    return -0.005 * acc;
}
__device__ inline double line_term(const double* th, const line_rec* r, long long k) {
    const double d = r->y[k] - (th[0] + th[1] * r->x[k]);
    return -0.5 * (r->ivar[k] * d * d);
}
struct LineModel {
    __device__ double base(const double* x, int ndim, int member, const void* user) const { return line_base(x, ndim); }
    __device__ double term(const double* x, int ndim, int member, long long k, const void* user) const {
        return line_term(x, (const line_rec*)user + member, k);
    }
};
struct LineFunctor {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const { return line_base(x, ndim); }
};
extern "C" __attribute__((visibility("default"))) int line_rec_bytes() { return (int)sizeof(line_rec); }
"""


class Launch(C.Structure):        # emx_fused_batch_data_launch of include/emx.h
    _fields_ = [("abi", C.c_uint32), ("args_bytes", C.c_uint32), ("ndim", C.c_int32), ("movesel", C.c_int32), ("grid", C.c_int32),
                ("threads", C.c_int32), ("lds_bytes", C.c_uint64), ("hip_stream", C.c_void_p), ("args", C.c_void_p),
                ("user", C.c_void_p), ("nblobs", C.c_int32), ("reserved", C.c_int32), ("ndata", C.c_void_p)]


def _abi(header, name):
    txt = open(os.path.join(CSRC, header)).read()
    return int(re.search(r"#define %s (0x[0-9a-fA-F]+|\d+)u" % name, txt).group(1), 0)


@pytest.fixture(scope="module")
def cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("fused_data_cache"))


@pytest.fixture(scope="module")
def built(cache):
    return compile_fused(SOURCE, "LineModel", 5, name="line5", cache_dir=cache, data=True)


@pytest.fixture(scope="module")
def plain(cache):
    return compile_fused(SOURCE, "LineFunctor", 5, name="plain5", cache_dir=cache)


def _args_bytes(fn, abi):
    """sizeof(SmallRunArgs) is internal: exactly one size is the library's"""
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(Launch)]
    rcs = [fn(C.byref(Launch(abi=abi, args_bytes=n, ndim=5, movesel=0, grid=0))) for n in range(8, 4096, 8)]
    assert sorted(set(rcs)) == [0, 1] and rcs.count(0) == 1
    return 8 * (rcs.index(0) + 1)


def test_compile_fused_data_builds_and_exports_the_launcher(built, plain, cache):
    assert isinstance(built, BatchFusedLibrary) and built.ndim == 5 and built.name == "line5" and built.data and built.nblobs == 0
    assert os.path.exists(built.path) and built.path.startswith(cache)
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", built.path], capture_output=True, text=True, check=True).stdout
        assert re.search(r"\bT line5\b", out), out
    assert built.lib.line_rec_bytes() == 24           # the user's own extern "C" function of the source
    assert built.path != plain.path and not plain.data
    t = built.target(user=1 << 20, ndata=[3, 0, 70])
    assert isinstance(t, BatchFused) and t.ndim == 5 and t.user_address() == 1 << 20 and t.ndata == (3, 0, 70) and t.nblobs == 0
    assert t.fn_ptr is built.launcher
    assert built.target(ndata=17).ndata == 17
    assert built.target(ndata=np.array([1, 2], dtype=np.int32)).ndata == (1, 2)
    with pytest.raises(ValueError) as e:              # a data library needs the counts, any other refuses them
        built.target(user=1 << 20)
    assert "data=True" in str(e.value)
    with pytest.raises(ValueError) as e:
        plain.target(ndata=4)
    assert "data=True" in str(e.value)
    assert plain.target().ndata is None
    # data=False keeps the translation unit and the cached library it always had
    assert compile_fused(SOURCE, "LineFunctor", 5, name="plain5", cache_dir=cache, data=False).path == plain.path


def test_the_launcher_answers_the_probe(built, plain):
    """grid == 0 launches nothing, so the probe runs without a GPU: 0 for this library's values at exactly one args_bytes, 1 for
    another ABI value -- the plain launcher's among them, and the plain launcher answers 1 to this one --, 2 for another ndim"""
    abi, abi_plain = _abi("emx_fused_target_data.hpp", "EMX_FUSED_BATCH_DATA_ABI"), _abi("emx_fused_target.hpp", "EMX_FUSED_ABI")
    fn = built.launcher
    nbytes = _args_bytes(fn, abi)
    good = dict(abi=abi, args_bytes=nbytes, ndim=5, movesel=0, grid=0)
    assert fn(C.byref(Launch(**good))) == 0
    assert fn(C.byref(Launch(**dict(good, abi=abi + 1)))) == 1
    assert fn(C.byref(Launch(**dict(good, abi=abi_plain)))) == 1
    assert fn(C.byref(Launch(**dict(good, ndim=6)))) == 2
    assert fn(C.byref(Launch(**dict(good, movesel=7)))) == 0
    assert fn(C.byref(Launch(**dict(good, movesel=3)))) == 3
    assert fn(C.byref(Launch(**dict(good, nblobs=2)))) == 4       # a data target carries no blobs
    assert fn(None) == 1
    pf = plain.launcher
    assert _args_bytes(pf, abi_plain) == nbytes                   # one SmallRunArgs
    assert pf(C.byref(Launch(**dict(good, abi=abi_plain)))) == 0
    assert pf(C.byref(Launch(**good))) == 1


def test_the_abi_constants_are_pairwise_distinct():
    vals = {}
    for hpp in ("emx_fused_target.hpp", "emx_fused_target_data.hpp", "emx_fused_ensemble.hpp", "emx_fused_ensemble_data.hpp", "emx_pt_fused.hpp"):
        for m in re.finditer(r"#define (EMX_FUSED\w*_ABI) (0x[0-9a-fA-F]+|\d+)u", open(os.path.join(CSRC, hpp)).read()):
            vals[m.group(1)] = int(m.group(2), 0)
    assert "EMX_FUSED_BATCH_DATA_ABI" in vals
    sharing = ("EMX_FUSED_ABI", "EMX_FUSED_BATCH_DATA_ABI", "EMX_FUSED_ENSEMBLE_SMALL_ABI")      # the three that travel in emx_fused_launch's prefix
    assert len({vals[k] for k in sharing}) == 3
    ens = ("EMX_FUSED_ENSEMBLE_ABI", "EMX_FUSED_ENSEMBLE_BLOBS_ABI", "EMX_FUSED_ENSEMBLE_SMALL_ABI", "EMX_FUSED_ENSEMBLE_DATA_ABI",
           "EMX_FUSED_BATCH_DATA_ABI")
    assert len({vals[k] for k in ens}) == len(ens)


def test_a_model_without_term_fails_with_the_compilers_diagnostic(cache):
    src = "struct NoTerm { __device__ double base(const double* x, int ndim, int member, const void* user) const { return 0.0; } };"
    with pytest.raises(RuntimeError) as e:
        compile_fused(src, "NoTerm", 5, cache_dir=cache, data=True)
    assert "error:" in str(e.value) and "hipcc failed" in str(e.value) and "term" in str(e.value)
    with pytest.raises(RuntimeError) as e:            # the plain functor is not a data model
        compile_fused(SOURCE, "LineFunctor", 5, cache_dir=cache, data=True)
    assert "error:" in str(e.value) and "base" in str(e.value)


def test_argument_checks_touch_no_device(cache):
    for bad in (True, 2.0, -1, 2 ** 31, "7", [3, True], [3, 2.5], [3, -1], [3, 2 ** 31], np.array([1.0, 2.0])):
        with pytest.raises(ValueError) as e:
            BatchFused(0x1000, 5, ndata=bad)
        assert "ndata" in str(e.value), bad
    assert BatchFused(0x1000, 5, ndata=0).ndata == 0
    assert BatchFused(0x1000, 5, ndata=2 ** 31 - 1).ndata == 2 ** 31 - 1
    assert BatchFused(0x1000, 5, ndata=np.int64(9)).ndata == 9
    assert BatchFused(0x1000, 5, ndata=(4, 0, 2 ** 31 - 1)).ndata == (4, 0, 2 ** 31 - 1)
    assert BatchFused(0x1000, 5).ndata is None
    with pytest.raises(ValueError) as e:              # no blobs with data
        BatchFused(0x1000, 5, nblobs=2, ndata=7)
    assert "nblobs" in str(e.value) and "ndata" in str(e.value)
    with pytest.raises(ValueError) as e:
        compile_fused(SOURCE, "LineModel", 5, nblobs=2, cache_dir=cache, data=True)
    assert "nblobs" in str(e.value) and "data" in str(e.value)
    # the length of ndata against the batch's size, when the batch takes the target
    t = BatchFused(0x1000, 5, ndata=[1, 2, 3])
    with pytest.raises(ValueError) as e:
        EnsembleBatch(4, 32, 5, t)
    assert "nbatch = 4" in str(e.value) and "got 3" in str(e.value)
    for ok in (t, BatchFused(0x1000, 5, ndata=6)):
        b = EnsembleBatch(3, 32, 5, ok)               # accepted, and still no device touched
        assert b._h is None and b._targets == [ok]
    with pytest.raises(ValueError) as e:              # ndim of the launcher != the batch's
        EnsembleBatch(3, 32, 6, t)
    assert "ndim 5" in str(e.value) and "ndim 6" in str(e.value)
    with pytest.raises(TypeError) as e:               # PTSampler refuses it as it refuses any BatchFused
        PTSampler(4, 16, 5, t, nbatch=3)
    assert "BatchFused" in str(e.value)


def test_header_declares_the_descriptor_and_the_setter():
    raw = open(os.path.join(ROOT, "include", "emx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    body = re.search(r"typedef\s+struct\s+emx_fused_batch_data_launch\s*\{([^}]*)\}\s*emx_fused_batch_data_launch\s*;", txt)
    assert body
    plain = re.search(r"struct\s+emx_fused_launch\s*\{([^}]*)\}", txt).group(1)
    names = lambda s: re.findall(r"(\w+)\s*[;,]", s)  # noqa: E731
    assert names(plain)[:10] == ["abi", "args_bytes", "ndim", "movesel", "grid", "threads", "lds_bytes", "hip_stream", "args", "user"]
    assert names(body.group(1)) == names(plain) + ["ndata"]       # emx_fused_launch's fields, then the counts
    assert re.search(r"const\s+int64_t\s*\*\s*ndata\s*;", body.group(1))
    assert [f[0] for f in Launch._fields_] == names(body.group(1)) == [f[0] for f in _lib.FusedBatchDataLaunch._fields_]
    assert C.sizeof(Launch) == C.sizeof(_lib.FusedBatchDataLaunch) == C.sizeof(_lib.FusedLaunch) + 8
    assert re.search(r"typedef\s+int\s*\(\s*\*\s*emx_fused_batch_data_fn\s*\)\s*\(\s*const\s+emx_fused_batch_data_launch\s*\*\s*\)\s*;", txt)
    assert re.search(r"int\s+emx_set_batch_target_fused_data\s*\(\s*emx_batch\s*\*\s*\w*\s*,\s*emx_fused_batch_data_fn\s+\w+\s*,\s*int32_t\s+\w+\s*,"
                     r"\s*const\s+void\s*\*\s*\w+\s*,\s*const\s+int64_t\s*\*\s*\w+\s*\)\s*;", txt)
    lib = _lib.load()
    assert hasattr(lib, "emx_set_batch_target_fused_data") and "emx_set_batch_target_fused_data" in _lib.SIGNATURES
    assert os.path.exists(os.path.join(CSRC, "emx_fused_target_data.hpp"))
    data_hdr = open(os.path.join(CSRC, "emx_fused_ensemble_data.hpp")).read()
    assert "EnsembleBatch" not in re.search(r"// Out of scope:[^\n]*", data_hdr).group(0).split(".")[0]
