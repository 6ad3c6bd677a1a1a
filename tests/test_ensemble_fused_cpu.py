"""Fused user targets of the single sampler (targets.DeviceFused / compile_fused_ensemble), what needs no GPU: hipcc cross-compiles
the user's translation unit, the cache, the compiler's diagnostics, the launcher's probe, the constexpr row layout against
pick_shape, the C ABI's declarations and the refusals made before any device is touched."""
import ctypes as C
import os
import re
import shutil
import subprocess
import time

import pytest

import emcee_amd
from emcee_amd import EnsembleBatch, PTSampler, _lib
from emcee_amd.targets import DeviceFused, DeviceFusedLibrary, compile_fused_ensemble, get_include

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "emcee_amd", "csrc", "emx_fused_ensemble.hpp")

# model (a) of tests/c/user_ensemble_fused.hip as a compile_fused_ensemble source: the functor and a helper of the user's own
SOURCE = r"""
struct diag_data { const double* mu; const double* ivar; };
struct DiagModel {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const {
        const diag_data* u = (const diag_data*)user;
        double acc = 0.0;
        for (int d = 0; d < ndim; ++d) {
            const double r = x[d] - u->mu[d];
            acc = acc + u->ivar[d] * r * r;
        }
        return -0.5 * acc;
    }
};
extern "C" __attribute__((visibility("default"))) int diag_data_bytes() { return (int)sizeof(diag_data); }
"""


class Launch(C.Structure):
    _fields_ = [("abi", C.c_uint32), ("args_bytes", C.c_uint32), ("ndim", C.c_int32), ("move", C.c_int32), ("grid", C.c_int32),
                ("threads", C.c_int32), ("lds_bytes", C.c_uint64), ("hip_stream", C.c_void_p), ("args", C.c_void_p),
                ("user", C.c_void_p)]


@pytest.fixture(scope="module")
def cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("fused_ens_cache"))


@pytest.fixture(scope="module")
def built(cache):
    t0 = time.time()
    lib = compile_fused_ensemble(SOURCE, "DiagModel", 5, name="diag5", cache_dir=cache)
    print("compile_fused_ensemble: one model, ndim 5: %.1f s" % (time.time() - t0))
    return lib


def test_compile_builds_and_exports_the_launcher(built, cache):
    assert isinstance(built, DeviceFusedLibrary) and built.ndim == 5 and built.name == "diag5"
    assert os.path.exists(built.path) and built.path.startswith(cache)
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", built.path], capture_output=True, text=True, check=True).stdout
        assert re.search(r"\bT diag5\b", out), out
    assert built.lib.diag_data_bytes() == 16          # the user's own extern "C" function of the source
    t = built.target(user=1 << 20)
    assert isinstance(t, DeviceFused) and t.ndim == 5 and t.user_address() == 1 << 20 and t.kind == _lib.TARGET_FUSED_ENSEMBLE
    assert t.fn_ptr is built.launcher


def _abi():
    return int(re.search(r"#define EMX_FUSED_ENSEMBLE_ABI (0x[0-9a-fA-F]+|\d+)u", open(HEADER).read()).group(1), 0)


def test_the_probe_checks_the_header_version_and_ndim(built):
    """grid == 0 launches nothing, so the probe runs without a GPU: 0 for exactly one args_bytes (sizeof(HalfStepArgs) is internal),
    1 for a bumped ABI, 2 for another ndim"""
    abi = _abi()
    fn = built.launcher
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(Launch)]
    rcs = [fn(C.byref(Launch(abi=abi, args_bytes=n, ndim=5, move=0, grid=0))) for n in range(8, 4096, 8)]
    assert sorted(set(rcs)) == [0, 1] and rcs.count(0) == 1
    nbytes = 8 * (rcs.index(0) + 1)
    assert fn(C.byref(Launch(abi=abi + 1, args_bytes=nbytes, ndim=5, move=0, grid=0))) == 1
    assert fn(C.byref(Launch(abi=abi, args_bytes=nbytes, ndim=6, move=0, grid=0))) == 2
    for move in (0, 1, 2, 3, 4):                      # stretch, DE, snooker, Gaussian, evaluate rows
        assert fn(C.byref(Launch(abi=abi, args_bytes=nbytes, ndim=5, move=move, grid=0))) == 0
    assert fn(C.byref(Launch(abi=abi, args_bytes=nbytes, ndim=5, move=5, grid=0))) == 3
    # the batch targets' constants are other values: their descriptors, which start with the same two fields, are refused
    for other in ("emx_fused_target.hpp", "emx_pt_fused.hpp"):
        txt = open(os.path.join(ROOT, "emcee_amd", "csrc", other)).read()
        for m in re.finditer(r"#define EMX_FUSED\w*_ABI (0x[0-9a-fA-F]+|\d+)u", txt):
            assert int(m.group(1), 0) != abi
            assert fn(C.byref(Launch(abi=int(m.group(1), 0), args_bytes=nbytes, ndim=5, move=0, grid=0))) == 1


def test_compile_caches(built, cache):
    mtime = os.stat(built.path).st_mtime_ns
    again = compile_fused_ensemble(SOURCE, "DiagModel", 5, name="diag5", cache_dir=cache)
    assert again.path == built.path and os.stat(again.path).st_mtime_ns == mtime      # nothing was compiled
    other = compile_fused_ensemble(SOURCE, "DiagModel", 3, name="diag5", cache_dir=cache)
    assert other.path != built.path and os.path.exists(other.path) and other.ndim == 3
    changed = compile_fused_ensemble(SOURCE + "\n// another source\n", "DiagModel", 5, name="diag5", cache_dir=cache)
    assert changed.path != built.path and os.path.exists(changed.path)


def test_the_cache_key_includes_the_new_header():
    from emcee_amd import _build
    assert HEADER in _build.DEPS


def test_a_syntax_error_raises_with_the_compilers_diagnostic(cache):
    with pytest.raises(RuntimeError) as e:
        compile_fused_ensemble(SOURCE + "\nthis is not C++;\n", "DiagModel", 5, cache_dir=cache)
    assert "error:" in str(e.value) and "hipcc failed" in str(e.value)
    with pytest.raises(ValueError):
        compile_fused_ensemble(SOURCE, "DiagModel", 0, cache_dir=cache)
    with pytest.raises(ValueError):
        compile_fused_ensemble(SOURCE, "DiagModel", 257, cache_dir=cache)
    with pytest.raises(ValueError):
        compile_fused_ensemble(SOURCE, "Diag Model; int x", 5, cache_dir=cache)


def test_constexpr_layout_equals_pick_shape(tmp_path):
    """fused_ens_g / _v / _ch against pick_shape(D, D) for every ndim in range, in a host program; the launch rules hold everywhere"""
    src = tmp_path / "layout.cpp"
    src.write_text(r"""
#include <emx_fused_ensemble.hpp>
#include <cstdio>
int main() {
    int bad = 0;
    for (int D = 1; D <= emx::FUSED_ENS_MAX_NDIM; ++D) {
        const emx::Shape s = emx::pick_shape(D, D);
        const int tile = emx::fused_ens_tile_rule(D), gpb = (emx::FUSED_ENS_THREADS / 64) * (64 / s.G);
        if (s.G != emx::fused_ens_g(D) || s.V != emx::fused_ens_v(D) || s.CH != emx::fused_ens_ch(D)) { ++bad; std::printf("layout %d\n", D); }
        if (s.G * s.V * s.CH < D) { ++bad; std::printf("cover %d\n", D); }
        if (tile < gpb || tile % gpb != 0 || tile > emx::FUSED_ENS_THREADS) { ++bad; std::printf("tile %d\n", D); }
        if (emx::fused_ens_lds_bytes(D) > 40 * 1024 || emx::fused_ens_lds_bytes(D) < (size_t)tile * ((D | 1) * 8 + 12)) { ++bad; std::printf("lds %d\n", D); }
    }
    std::printf("checked %d\n", emx::FUSED_ENS_MAX_NDIM);
    return bad;
}
""")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "layout")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-x", "hip"] + ["-I" + d for d in get_include()] + [str(src), "-o", exe],
                   check=True, timeout=900, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "checked 256" in r.stdout, r.stdout


def test_header_declares_the_fused_ensemble_abi():
    raw = open(os.path.join(ROOT, "include", "emx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    body = re.search(r"typedef\s+struct\s+emx_fused_ensemble_launch\s*\{([^}]*)\}\s*emx_fused_ensemble_launch\s*;", txt)
    assert body
    names = re.findall(r"\b(\w+)\s*[;,]", body.group(1))
    assert names == ["abi", "args_bytes", "ndim", "move", "grid", "threads", "lds_bytes", "hip_stream", "args", "user"]
    assert [n for n, _ in Launch._fields_] == names and [n for n, _ in _lib.FusedEnsembleLaunch._fields_] == names
    assert C.sizeof(_lib.FusedEnsembleLaunch) == C.sizeof(Launch) == 56
    assert re.search(r"typedef\s+int\s*\(\s*\*\s*emx_fused_ensemble_fn\s*\)\s*\(\s*const\s+emx_fused_ensemble_launch\s*\*\s*\)\s*;", txt)
    assert re.search(r"int\s+emx_set_target_fused\s*\(\s*emx_ctx\s*\*\s*\w*\s*,\s*emx_fused_ensemble_fn\s+\w+\s*,\s*const\s+void\s*\*\s*\w+\s*\)\s*;", txt)
    assert re.search(r"EMX_TARGET_FUSED_ENSEMBLE\s*=\s*10\b", txt)
    lib = _lib.load()
    assert hasattr(lib, "emx_set_target_fused") and "emx_set_target_fused" in _lib.SIGNATURES
    assert _lib.TARGET_FUSED_ENSEMBLE == 10


def test_argument_checks_and_refusals_touch_no_device():
    for bad in (0, None, True):
        with pytest.raises(TypeError):
            DeviceFused(bad, 5)
    with pytest.raises(TypeError):
        DeviceFused(0x1000, 5.5)
    with pytest.raises(TypeError):
        DeviceFused(0x1000, 257)
    with pytest.raises(TypeError):
        DeviceFused(0x1000, 5, user="somewhere")
    t = DeviceFused(0x1000, 5)
    assert t.user_address() is None and DeviceFused(0x1000, 5, user=C.c_void_p(64)).user_address() == 64
    with pytest.raises(TypeError) as e:               # not callable outside a sampler
        t([0.0] * 5)
    assert "DeviceFused" in str(e.value)
    with pytest.raises(TypeError) as e:
        EnsembleBatch(4, 32, 5, t)
    assert "DeviceFused" in str(e.value) and "EnsembleSampler" in str(e.value)
    with pytest.raises(TypeError) as e:
        EnsembleBatch(2, 32, 5, [t, t])
    assert "DeviceFused" in str(e.value)
    with pytest.raises(TypeError) as e:
        PTSampler(4, 16, 5, t, nbatch=2)
    assert "DeviceFused" in str(e.value)
    with pytest.raises(ValueError) as e:              # ndim of the launcher != the sampler's
        emcee_amd.EnsembleSampler(32, 6, t)
    assert "ndim 5" in str(e.value) and "ndim 6" in str(e.value)
    with pytest.raises(ValueError) as e:              # one GPU only: refused before the process group is even looked at
        emcee_amd.EnsembleSampler(32, 5, t, distributed=True)
    assert "DeviceFused" in str(e.value) and "distributed" in str(e.value)
    s = emcee_amd.EnsembleSampler(32, 5, t)           # accepted, and still no device touched
    assert s._ens is None and s._device_target is t


def test_the_test_models_compile(tmp_path):
    """tests/c/user_ensemble_fused.hip (the GPU tests' models, both wrappings of each) cross-compiles and exports its entry points"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    so = str(tmp_path / "libuser_ens.so")
    subprocess.run([hipcc] + ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DUSER_NDIM=3"] +
                   ["-I" + d for d in get_include()] + [os.path.join(ROOT, "tests", "c", "user_ensemble_fused.hip"), "-o", so],
                   check=True, timeout=900, capture_output=True)
    _lib.load()
    user = C.CDLL(so)
    for name in ("user_fused_a", "user_fused_b", "user_fused_n", "user_rows_a", "user_rows_b", "user_rows_n", "user_setup",
                 "user_device_pointer", "user_teardown"):
        assert hasattr(user, name)
