"""Fused tempered targets of PTSampler (targets.PTFused / compile_fused_pt), what needs no GPU: the argument checks made before any
device is touched, emx_pt_fused_check, hipcc cross-compiling the test models, the launcher's probe, and the compile cache."""
import ctypes as C
import os
import re
import shutil
import subprocess
import time

import numpy as np
import pytest

import emcee_amd
from emcee_amd import EnsembleBatch, PTSampler, _lib, moves
from emcee_amd.targets import BatchCallable, BatchKernel, PTFused, PTFusedLibrary, compile_fused_pt, get_include

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOURCE = r"""
struct Like {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const {
        const double* mu = (const double*)user + (long long)member * ndim;
        double acc = 0.0;
        for (int d = 0; d < ndim; ++d) acc = acc + (x[d] - mu[d]) * (x[d] - mu[d]);
        return -0.5 * acc;
    }
};
struct Prior {
    __device__ double operator()(const double* x, int ndim, int, const void*) const {
        double acc = 0.0;
        for (int d = 0; d < ndim; ++d) acc = acc + x[d] * x[d];
        return -0.005 * acc;
    }
};
"""


class Launch(C.Structure):          # emx_pt_fused_launch of include/emx.h
    _fields_ = [("abi", C.c_uint32), ("args_bytes", C.c_uint32), ("ndim", C.c_int32), ("movesel", C.c_int32), ("grid", C.c_int32),
                ("threads", C.c_int32), ("lds_bytes", C.c_uint64), ("hip_stream", C.c_void_p), ("args", C.c_void_p),
                ("user", C.c_void_p), ("has_prior", C.c_int32)]


def test_argument_checks_touch_no_device():
    for bad in (0, None, True):
        with pytest.raises(TypeError):
            PTFused(bad, 3)
    with pytest.raises(TypeError):
        PTFused(0x1000, 3.5)
    with pytest.raises(TypeError):
        PTFused(0x1000, 3, user="somewhere")
    t = PTFused(0x1000, 3)
    assert t.user_address() is None and t.has_prior is None
    assert PTFused(0x1000, 3, user=C.c_void_p(64)).user_address() == 64
    pt = PTSampler(4, 16, 3, t, nbatch=2, seeds=[1, 2])          # constructs, and no device was touched
    assert pt._h is None and pt._b._h is None
    pt = PTSampler(4, 16, 3, t, log_prior=(-np.ones(3), np.ones(3)), nbatch=2)
    assert pt._h is None
    with pytest.raises(ValueError) as e:                          # ndim of the launcher != the sampler's
        PTSampler(4, 16, 4, t)
    assert "ndim 3" in str(e.value) and "ndim 4" in str(e.value)
    with pytest.raises(ValueError) as e:                          # a prior functor in the launcher and a log_prior on top
        PTSampler(4, 16, 3, PTFused(0x1000, 3, has_prior=True), log_prior=(-np.ones(3), np.ones(3)))
    assert "prior functor" in str(e.value)
    for prior in (BatchCallable(lambda q: q.sum(-1)), BatchKernel(0x2000)):
        with pytest.raises(TypeError) as e:                       # mixing would need the callback path
            PTSampler(4, 16, 3, t, log_prior=prior)
        assert "callback path" in str(e.value)
    with pytest.raises(TypeError) as e:
        EnsembleBatch(4, 16, 3, t)
    assert "PTSampler" in str(e.value)
    with pytest.raises(TypeError):
        emcee_amd.EnsembleSampler(16, 3, t)


def test_an_object_beyond_one_workgroup_is_refused_at_construction():
    with pytest.raises(ValueError) as e:
        PTSampler(16, 256, 32, PTFused(0x1000, 32))
    assert "LDS" in str(e.value) and "BatchKernel" in str(e.value)


def test_emx_pt_fused_check():
    lib = _lib.load()
    assert "emx_pt_fused_check" in _lib.SIGNATURES and "emx_pt_set_target_fused" in _lib.SIGNATURES
    msg = C.create_string_buffer(512)
    arr = (_lib.MoveDesc * 1)(moves.StretchMove()._desc(5))
    assert lib.emx_pt_fused_check(16, 32, 5, 1, arr, msg, 512) == 0
    arr = (_lib.MoveDesc * 1)(moves.StretchMove()._desc(32))
    assert lib.emx_pt_fused_check(16, 256, 32, 1, arr, msg, 512) == -1          # its coordinates alone are 1 MB
    assert b"LDS" in msg.value and re.search(rb"\d+ bytes", msg.value)
    assert lib.emx_pt_fused_check(0, 32, 5, 1, arr, msg, 512) == -1
    assert lib.emx_pt_fused_check(4, 32, 5, 0, None, msg, 512) == -1


def test_header_declares_the_tempered_fused_abi():
    raw = open(os.path.join(ROOT, "include", "emx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    body = re.search(r"typedef\s+struct\s+emx_pt_fused_launch\s*\{([^}]*)\}\s*emx_pt_fused_launch\s*;", txt).group(1)
    for field, _ in Launch._fields_:
        assert re.search(r"\b%s\b" % field, body)
    assert re.search(r"typedef\s+int\s*\(\s*\*\s*emx_pt_fused_fn\s*\)\s*\(\s*emx_pt_fused_launch\s*\*\s*\)\s*;", txt)
    assert re.search(r"EMX_TARGET_FUSED_PT\s*=\s*9\b", txt) and _lib.TARGET_FUSED_PT == 9
    assert os.path.exists(os.path.join(get_include()[1], "emx_pt_fused.hpp"))


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """tests/c/user_pt_fused.hip (the GPU tests' models, both wrappings of each) cross-compiled for gfx950 at ndim 3"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    so = str(tmp_path_factory.mktemp("pt_fused") / "libuser_pt_fused.so")
    subprocess.run([hipcc] + ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DUSER_NDIM=3",
                              "-DUSER_WITH_NAN"] + ["-I" + d for d in get_include()] +
                   [os.path.join(ROOT, "tests", "c", "user_pt_fused.hip"), "-o", so], check=True, timeout=900, capture_output=True)
    _lib.load()
    return C.CDLL(so)


def test_the_test_models_compile_and_export_their_entry_points(models):
    for name in ("pt_fused_a", "pt_fused_ap", "pt_fused_m", "pt_fused_n", "user_block_a", "user_block_m", "user_block_n", "user_block_p",
                 "user_setup", "user_device_pointer", "user_teardown"):
        assert hasattr(models, name)


def test_the_launcher_checks_abi_size_ndim_and_selector_on_the_probe(models):
    """grid == 0 launches nothing, so the probe runs without a GPU"""
    txt = open(os.path.join(ROOT, "emcee_amd", "csrc", "emx_pt_fused.hpp")).read()
    abi = int(re.search(r"#define EMX_FUSED_PT_ABI (\d+)u", txt).group(1))
    fn = models.pt_fused_a
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(Launch)]
    rcs = [fn(C.byref(Launch(abi=abi, args_bytes=n, ndim=3, movesel=0, grid=0))) for n in range(8, 4096, 8)]
    assert sorted(set(rcs)) == [0, 1] and rcs.count(0) == 1      # sizeof(PtRunArgs) is internal: exactly one size is the library's
    nbytes = 8 * (rcs.index(0) + 1)
    assert fn(C.byref(Launch(abi=abi + 1, args_bytes=nbytes, ndim=3, movesel=0, grid=0))) == 1
    assert fn(C.byref(Launch(abi=abi, args_bytes=nbytes, ndim=4, movesel=0, grid=0))) == 2
    assert fn(C.byref(Launch(abi=abi, args_bytes=nbytes, ndim=3, movesel=7, grid=0))) == 0
    assert fn(C.byref(Launch(abi=abi, args_bytes=nbytes, ndim=3, movesel=3, grid=0))) == 3
    for name, has in (("pt_fused_a", 0), ("pt_fused_ap", 1)):      # the probe reports the prior functor
        f = getattr(models, name)
        f.restype, f.argtypes = C.c_int, [C.POINTER(Launch)]
        L = Launch(abi=abi, args_bytes=nbytes, ndim=3, movesel=0, grid=0, has_prior=-1)
        assert f(C.byref(L)) == 0 and L.has_prior == has
    n = models.pt_fused_n                                           # the single-StretchMove kernel alone
    n.restype, n.argtypes = C.c_int, [C.POINTER(Launch)]
    assert n(C.byref(Launch(abi=abi, args_bytes=nbytes, ndim=3, movesel=0, grid=0))) == 0
    assert n(C.byref(Launch(abi=abi, args_bytes=nbytes, ndim=3, movesel=7, grid=0))) == 3


def test_compile_fused_pt_builds_and_caches(tmp_path):
    cache = str(tmp_path)
    t0 = time.time()
    lib = compile_fused_pt(SOURCE, "Like", 3, prior="Prior", name="like3", cache_dir=cache)
    print("compile_fused_pt: one model, ndim 3: %.1f s" % (time.time() - t0))
    assert isinstance(lib, PTFusedLibrary) and lib.ndim == 3 and lib.name == "like3" and lib.has_prior
    assert os.path.exists(lib.path) and lib.path.startswith(cache)
    t = lib.target(user=1 << 20)
    assert isinstance(t, PTFused) and t.has_prior and t.user_address() == 1 << 20 and t.fn_ptr is lib.launcher
    mtime = os.stat(lib.path).st_mtime_ns
    t0 = time.time()
    again = compile_fused_pt(SOURCE, "Like", 3, prior="Prior", name="like3", cache_dir=cache)
    assert again.path == lib.path and os.stat(again.path).st_mtime_ns == mtime and time.time() - t0 < 2.0      # nothing was compiled
    flat = compile_fused_pt(SOURCE, "Like", 3, name="like3", cache_dir=cache)
    assert flat.path != lib.path and not flat.has_prior
    with pytest.raises(ValueError):                                 # a launcher with a prior functor and a box on top
        PTSampler(4, 16, 3, t, log_prior=(-np.ones(3), np.ones(3)))
    with pytest.raises(RuntimeError) as e:
        compile_fused_pt(SOURCE + "\nthis is not C++;\n", "Like", 3, cache_dir=cache)
    assert "error:" in str(e.value) and "hipcc failed" in str(e.value)
    with pytest.raises(ValueError):
        compile_fused_pt(SOURCE, "Like; int x", 3, cache_dir=cache)
