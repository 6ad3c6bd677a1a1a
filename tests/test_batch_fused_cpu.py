"""Fused user targets of EnsembleBatch (targets.BatchFused / compile_fused), what needs no GPU: hipcc cross-compiles the user's
translation unit, the cache, the compiler's diagnostics, the C ABI's declarations and the argument checks made before any
device is touched."""
import ctypes as C
import os
import re
import shutil
import subprocess
import time

import pytest

import emcee_amd
from emcee_amd import EnsembleBatch, PTSampler, _lib, moves
from emcee_amd.targets import BatchFused, BatchFusedLibrary, compile_fused, get_include

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# model (a) of tests/c/user_fused_logprob.hip as a compile_fused source: the functor and a helper of the user's own
SOURCE = r"""
struct diag_data { const double* mu; const double* ivar; };
struct DiagModel {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const {
        const diag_data* u = (const diag_data*)user;
        double acc = 0.0;
        for (int d = 0; d < ndim; ++d) {
            const double r = x[d] - u->mu[(long long)member * ndim + d];
            acc = acc + u->ivar[(long long)member * ndim + d] * r * r;
        }
        return -0.5 * acc;
    }
};
extern "C" __attribute__((visibility("default"))) int diag_data_bytes() { return (int)sizeof(diag_data); }
"""


@pytest.fixture(scope="module")
def cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("fused_cache"))


@pytest.fixture(scope="module")
def built(cache):
    t0 = time.time()
    lib = compile_fused(SOURCE, "DiagModel", 5, name="diag5", cache_dir=cache)
    print("compile_fused: one model, ndim 5: %.1f s" % (time.time() - t0))
    return lib


def test_compile_fused_builds_and_exports_the_launcher(built, cache):
    assert isinstance(built, BatchFusedLibrary) and built.ndim == 5 and built.name == "diag5"
    assert os.path.exists(built.path) and built.path.startswith(cache)
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", built.path], capture_output=True, text=True, check=True).stdout
        assert re.search(r"\bT diag5\b", out), out
    assert isinstance(built.lib, C.CDLL)
    assert built.lib.diag_data_bytes() == 16          # the user's own extern "C" function of the source
    t = built.target(user=1 << 20)
    assert isinstance(t, BatchFused) and t.ndim == 5 and t.user_address() == 1 << 20
    assert t.fn_ptr is built.launcher


def test_the_launcher_checks_the_header_version_on_the_probe(built):
    """grid == 0 launches nothing, so the probe runs without a GPU: 0 for this library's values, 1 for another version's, 2 for
    another ndim"""
    class Launch(C.Structure):
        _fields_ = [("abi", C.c_uint32), ("args_bytes", C.c_uint32), ("ndim", C.c_int32), ("movesel", C.c_int32), ("grid", C.c_int32),
                    ("threads", C.c_int32), ("lds_bytes", C.c_uint64), ("hip_stream", C.c_void_p), ("args", C.c_void_p),
                    ("user", C.c_void_p)]
    txt = open(os.path.join(ROOT, "emcee_amd", "csrc", "emx_fused_target.hpp")).read()
    abi = int(re.search(r"#define EMX_FUSED_ABI (\d+)u", txt).group(1))
    fn = built.launcher
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(Launch)]
    rcs = []
    for nbytes in range(8, 4096, 8):                  # sizeof(SmallRunArgs) is internal: exactly one size is the library's
        rcs.append(fn(C.byref(Launch(abi=abi, args_bytes=nbytes, ndim=5, movesel=0, grid=0))))
    assert sorted(set(rcs)) == [0, 1] and rcs.count(0) == 1
    nbytes = 8 * (rcs.index(0) + 1)
    assert fn(C.byref(Launch(abi=abi + 1, args_bytes=nbytes, ndim=5, movesel=0, grid=0))) == 1
    assert fn(C.byref(Launch(abi=abi, args_bytes=nbytes, ndim=6, movesel=0, grid=0))) == 2
    assert fn(C.byref(Launch(abi=abi, args_bytes=nbytes, ndim=5, movesel=7, grid=0))) == 0
    assert fn(C.byref(Launch(abi=abi, args_bytes=nbytes, ndim=5, movesel=3, grid=0))) == 3


def test_compile_fused_caches(built, cache):
    mtime = os.stat(built.path).st_mtime_ns
    t0 = time.time()
    again = compile_fused(SOURCE, "DiagModel", 5, name="diag5", cache_dir=cache)
    assert again.path == built.path and os.stat(again.path).st_mtime_ns == mtime
    assert time.time() - t0 < 2.0                     # nothing was compiled
    other = compile_fused(SOURCE, "DiagModel", 3, name="diag5", cache_dir=cache)
    assert other.path != built.path and os.path.exists(other.path) and other.ndim == 3
    flagged = compile_fused(SOURCE, "DiagModel", 5, name="diag5", flags=["-DSOMETHING=1"], cache_dir=cache)
    assert flagged.path != built.path


def test_compile_fused_default_cache_dir(monkeypatch, tmp_path, built):
    monkeypatch.setenv("EMCEE_AMD_CACHE", str(tmp_path / "envcache"))
    lib = compile_fused(SOURCE, "DiagModel", 5, name="diag5")
    assert lib.path.startswith(str(tmp_path / "envcache"))


def test_a_syntax_error_raises_with_the_compilers_diagnostic(cache):
    with pytest.raises(RuntimeError) as e:
        compile_fused(SOURCE + "\nthis is not C++;\n", "DiagModel", 5, cache_dir=cache)
    assert "error:" in str(e.value) and "hipcc failed" in str(e.value)
    with pytest.raises(RuntimeError) as e:          # a functor without the call operator: the error names the contract's call
        compile_fused("struct Empty {};", "Empty", 5, cache_dir=cache)
    assert "error:" in str(e.value)
    with pytest.raises(ValueError):
        compile_fused(SOURCE, "DiagModel", 0, cache_dir=cache)
    with pytest.raises(ValueError):
        compile_fused(SOURCE, "Diag Model; int x", 5, cache_dir=cache)


def test_header_declares_the_fused_abi():
    raw = open(os.path.join(ROOT, "include", "emx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"typedef\s+struct\s+emx_fused_launch\s*\{[^}]*\}\s*emx_fused_launch\s*;", txt)
    for field in ("abi", "args_bytes", "ndim", "movesel", "grid", "threads", "lds_bytes", "hip_stream", "args", "user"):
        assert re.search(r"\b%s\b" % field, re.search(r"struct\s+emx_fused_launch\s*\{([^}]*)\}", txt).group(1))
    assert re.search(r"typedef\s+int\s*\(\s*\*\s*emx_fused_batch_fn\s*\)\s*\(\s*const\s+emx_fused_launch\s*\*\s*\)\s*;", txt)
    assert re.search(r"int\s+emx_set_batch_target_fused\s*\(\s*emx_batch\s*\*\s*\w*\s*,\s*emx_fused_batch_fn", txt)
    assert re.search(r"EMX_TARGET_FUSED_USER\s*=\s*8\b", txt)
    lib = _lib.load()
    assert hasattr(lib, "emx_set_batch_target_fused") and "emx_set_batch_target_fused" in _lib.SIGNATURES
    assert _lib.TARGET_FUSED_USER == 8


def test_get_include():
    inc = get_include()
    assert emcee_amd.get_include() == inc and len(inc) == 2
    assert all(os.path.isdir(d) for d in inc)
    assert os.path.exists(os.path.join(inc[0], "emx.h"))
    assert os.path.exists(os.path.join(inc[1], "emx_fused_target.hpp"))


def test_argument_checks_touch_no_device():
    with pytest.raises(TypeError):
        BatchFused(0, 5)
    with pytest.raises(TypeError):
        BatchFused(None, 5)
    with pytest.raises(TypeError):
        BatchFused(True, 5)
    with pytest.raises(TypeError):
        BatchFused(0x1000, 5.5)
    with pytest.raises(TypeError):
        BatchFused(0x1000, 5, user="somewhere")
    t = BatchFused(0x1000, 5)
    assert t.user_address() is None
    assert BatchFused(0x1000, 5, user=C.c_void_p(64)).user_address() == 64
    with pytest.raises(ValueError) as e:              # ndim of the launcher != the batch's
        EnsembleBatch(4, 32, 6, t)
    assert "ndim 5" in str(e.value) and "ndim 6" in str(e.value)
    with pytest.raises(ValueError) as e:              # a member beyond one workgroup's LDS, refused by emx_batch_check
        EnsembleBatch(2, 2048, 16, BatchFused(0x1000, 16))
    assert "LDS" in str(e.value)
    msg = C.create_string_buffer(256)
    d = moves.StretchMove()._desc(16)
    arr = (_lib.MoveDesc * 1)(d)
    lib = _lib.load()
    assert lib.emx_batch_check(2048, 16, _lib.TARGET_FUSED_USER, 1, arr, msg, 256) == -1 and b"LDS" in msg.value
    assert lib.emx_batch_check(32, 5, _lib.TARGET_FUSED_USER, 1, arr, msg, 256) == 0
    # the staging area counts: 700 x 16 fits a built-in target's workgroup and not a fused user target's under a one-split move
    g = (_lib.MoveDesc * 1)(moves.GaussianMove(0.1)._desc(16))
    assert lib.emx_batch_check(700, 16, _lib.TARGET_DIAG, 1, g, msg, 256) == 0
    assert lib.emx_batch_check(700, 16, _lib.TARGET_FUSED_USER, 1, g, msg, 256) == -1 and b"LDS" in msg.value
    with pytest.raises(TypeError) as e:
        EnsembleBatch(2, 32, 5, [t, t])
    assert "ONE" in str(e.value) and "for all members" in str(e.value)
    b = EnsembleBatch(4, 32, 5, t)                    # accepted, and still no device touched
    assert b._h is None and b._targets == [t]
    with pytest.raises(TypeError):                    # not a target of a single ensemble
        emcee_amd.EnsembleSampler(32, 5, t)


def test_ptsampler_refuses_a_fused_target():
    t = BatchFused(0x1000, 3)
    with pytest.raises(TypeError) as e:
        PTSampler(4, 16, 3, t, nbatch=2)
    assert "BatchCallable" in str(e.value) and "BatchKernel" in str(e.value) and "BatchFused" in str(e.value)


def test_the_test_models_compile(tmp_path):
    """tests/c/user_fused_logprob.hip (the GPU tests' models, both wrappings of each) cross-compiles and exports its entry points"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    so = str(tmp_path / "libuser_fused.so")
    subprocess.run([hipcc] + ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DUSER_NDIM=3",
                              "-DUSER_WITH_NAN"] + ["-I" + d for d in get_include()] +
                   [os.path.join(ROOT, "tests", "c", "user_fused_logprob.hip"), "-o", so], check=True, timeout=900, capture_output=True)
    _lib.load()
    user = C.CDLL(so)
    for name in ("user_fused_a", "user_fused_b", "user_fused_n", "user_block_a", "user_block_b", "user_block_n", "user_setup",
                 "user_device_pointer", "user_teardown"):
        assert hasattr(user, name)
