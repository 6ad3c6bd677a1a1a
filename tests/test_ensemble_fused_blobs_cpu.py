"""Blobs of a DeviceFused target (EMX_FUSED_ENSEMBLE_TARGET_BLOBS / compile_fused_ensemble(nblobs=K)), what needs no GPU: hipcc
cross-compiles the five-argument functor, the launcher's probe tells versions, ndim and blob counts apart, the two descriptor types
refuse each other, the cache keeps the blob-free entries, the C ABI declares the new names, the launch rules hold for every
(ndim, nblobs), and the argument checks touch no device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import emcee_amd
from emcee_amd import EnsembleBatch, PTSampler, _lib
from emcee_amd.targets import DeviceFused, DeviceFusedLibrary, compile_fused_ensemble, get_include

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "emcee_amd", "csrc")
HEADER = os.path.join(CSRC, "emx_fused_ensemble.hpp")

# one source, both forms of the functor over one lp routine -- what compile_fused takes for a batch
SOURCE = r"""
struct diag_data { const double* mu; const double* ivar; };
struct DiagModel {
    __device__ static double lp(const double* x, int ndim, const void* user) {
        const diag_data* u = (const diag_data*)user;
        double acc = 0.0;
        for (int d = 0; d < ndim; ++d) {
            const double r = x[d] - u->mu[d];
            acc = acc + u->ivar[d] * r * r;
        }
        return -0.5 * acc;
    }
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const { return lp(x, ndim, user); }
    __device__ double operator()(const double* x, int ndim, int member, const void* user, double* blobs) const {
        const double v = lp(x, ndim, user);
        blobs[0] = x[0];
        blobs[1] = x[ndim - 1] + x[0];
        blobs[2] = v;
        return v;
    }
};
"""

NAMES = ["abi", "args_bytes", "ndim", "move", "grid", "threads", "lds_bytes", "hip_stream", "args", "user", "nblobs", "reserved",
         "blobs_cur", "blobs_row"]
NEW = ("emx_set_target_fused_blobs", "emx_get_blobs", "emx_set_blobs", "emx_eval_log_prob_blobs", "emx_snapshot_read_blobs")


class Launch(C.Structure):
    _fields_ = [("abi", C.c_uint32), ("args_bytes", C.c_uint32), ("ndim", C.c_int32), ("move", C.c_int32), ("grid", C.c_int32),
                ("threads", C.c_int32), ("lds_bytes", C.c_uint64), ("hip_stream", C.c_void_p), ("args", C.c_void_p),
                ("user", C.c_void_p), ("nblobs", C.c_int32), ("reserved", C.c_int32), ("blobs_cur", C.c_void_p),
                ("blobs_row", C.c_void_p)]


def _const(name, path=HEADER):
    return int(re.search(r"#define %s (0x[0-9a-fA-F]+|\d+)u" % name, open(path).read()).group(1), 0)


@pytest.fixture(scope="module")
def cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("fused_ens_blobs_cache"))


@pytest.fixture(scope="module")
def built(cache):
    return compile_fused_ensemble(SOURCE, "DiagModel", 5, name="diag5b", cache_dir=cache, nblobs=3)


@pytest.fixture(scope="module")
def plain(cache):
    return compile_fused_ensemble(SOURCE, "DiagModel", 5, name="diag5", cache_dir=cache)


def test_compile_with_blobs_builds_and_exports_the_launcher(built, cache):
    assert isinstance(built, DeviceFusedLibrary) and (built.ndim, built.nblobs, built.name) == (5, 3, "diag5b")
    assert os.path.exists(built.path) and built.path.startswith(cache)
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", built.path], capture_output=True, text=True, check=True).stdout
        assert re.search(r"\bT diag5b\b", out), out
    t = built.target(user=1 << 20)
    assert isinstance(t, DeviceFused) and (t.ndim, t.nblobs) == (5, 3) and t.user_address() == 1 << 20
    assert t.fn_ptr is built.launcher and t.kind == _lib.TARGET_FUSED_ENSEMBLE


def _probe(fn, **kw):
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(Launch)]
    return fn(C.byref(Launch(**kw)))


def test_the_probe_tells_versions_ndim_and_blob_counts_apart(built, plain):
    abi, old_abi = _const("EMX_FUSED_ENSEMBLE_BLOBS_ABI"), _const("EMX_FUSED_ENSEMBLE_ABI")
    assert abi != old_abi
    fn = built.launcher
    rcs = [_probe(fn, abi=abi, args_bytes=n, ndim=5, move=0, grid=0, nblobs=3) for n in range(8, 4096, 8)]
    assert sorted(set(rcs)) == [0, 1] and rcs.count(0) == 1          # exactly one args_bytes (sizeof(HalfStepArgs) is internal)
    nbytes = 8 * (rcs.index(0) + 1)
    for move in (0, 1, 2, 3, 4):
        assert _probe(fn, abi=abi, args_bytes=nbytes, ndim=5, move=move, grid=0, nblobs=3) == 0
    assert _probe(fn, abi=abi, args_bytes=nbytes, ndim=5, move=5, grid=0, nblobs=3) == 3
    for other in (0, 2, 4):                                           # another number of blobs
        assert _probe(fn, abi=abi, args_bytes=nbytes, ndim=5, move=0, grid=0, nblobs=other) == 4
    assert _probe(fn, abi=abi, args_bytes=nbytes, ndim=6, move=0, grid=0, nblobs=3) == 2
    # the blob-free descriptor's constant, and those of the batch and PT launchers, are other values: answer 1
    others = [old_abi]
    for hpp in ("emx_fused_target.hpp", "emx_pt_fused.hpp"):
        others += [int(m.group(1), 0) for m in re.finditer(r"#define EMX_\w*FUSED\w*_ABI (0x[0-9a-fA-F]+|\d+)u", open(os.path.join(CSRC, hpp)).read())]
    assert len(others) >= 3 and abi not in others
    for o in others:
        assert _probe(fn, abi=o, args_bytes=nbytes, ndim=5, move=0, grid=0, nblobs=3) == 1
    # ... and the blob-free launcher answers 1 to the new descriptor, 0 to its own
    assert _probe(plain.launcher, abi=abi, args_bytes=nbytes, ndim=5, move=0, grid=0, nblobs=3) == 1
    assert _probe(plain.launcher, abi=old_abi, args_bytes=nbytes, ndim=5, move=0, grid=0) == 0


def test_a_blob_free_build_keeps_its_cache_entry(plain, built, cache):
    again = compile_fused_ensemble(SOURCE, "DiagModel", 5, name="diag5", cache_dir=cache, nblobs=0)
    assert again.path == plain.path and again.nblobs == 0
    other = compile_fused_ensemble(SOURCE, "DiagModel", 5, name="diag5", cache_dir=cache, nblobs=3)
    assert other.path != plain.path and other.nblobs == 3
    # the key of a blob-free build is what it was before nblobs existed: (kind, source, functor, ndim, name) and the flags
    import hashlib
    from emcee_amd import _build, targets
    h = hashlib.sha256(repr((("ensemble", SOURCE, "DiagModel", 5, "diag5") + (targets.FUSED_FLAGS + [],))).encode())
    for d in _build.DEPS:
        if d.endswith((".hpp", ".h")):
            h.update(open(d, "rb").read())
    assert os.path.basename(os.path.dirname(plain.path)) == h.hexdigest()[:24]


def test_header_declares_the_blob_abi():
    raw = open(os.path.join(ROOT, "include", "emx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    body = re.search(r"typedef\s+struct\s+emx_fused_ensemble_blobs_launch\s*\{([^}]*)\}\s*emx_fused_ensemble_blobs_launch\s*;", txt)
    assert body
    names = re.findall(r"\b(\w+)\s*[;,]", body.group(1))
    assert names == NAMES
    assert [n for n, _ in Launch._fields_] == names and [n for n, _ in _lib.FusedEnsembleBlobsLaunch._fields_] == names
    assert C.sizeof(_lib.FusedEnsembleBlobsLaunch) == C.sizeof(Launch) == 80
    assert _lib.FusedEnsembleBlobsLaunch.nblobs.offset == C.sizeof(_lib.FusedEnsembleLaunch) == 56      # the old one is its prefix
    assert re.search(r"int32_t\s+nblobs\s*,\s*reserved\s*;\s*double\s*\*\s*blobs_cur\s*;\s*double\s*\*\s*blobs_row\s*;", body.group(1))
    assert re.search(r"typedef\s+int\s*\(\s*\*\s*emx_fused_ensemble_blobs_fn\s*\)\s*\(\s*const\s+emx_fused_ensemble_blobs_launch\s*\*\s*\)\s*;", txt)
    lib = _lib.load()
    for name in NEW:
        m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, txt)
        assert m, "include/emx.h does not declare %s" % name
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(m.group(1).split(",")), name
        assert hasattr(lib, name)
    hpp = open(HEADER).read()
    assert re.search(r"#define\s+EMX_FUSED_ENSEMBLE_TARGET_BLOBS\(name, Functor, ndim, nblobs\)", hpp)
    assert "what: 0 chain" in raw and "2 blobs" in raw


def test_launch_rules_hold_for_every_ndim_and_blob_count(tmp_path):
    """a host program walks (D, NB): the LDS request stays within 48 KB, the tile is whole passes of the workgroup, and NB = 0 is
    exactly the blob-free rule"""
    src = tmp_path / "rules.cpp"
    src.write_text(r"""
#include <emx_fused_ensemble.hpp>
#include <cstdio>
int main() {
    int bad = 0, n = 0;
    for (int D = 1; D <= emx::FUSED_ENS_MAX_NDIM; ++D)
        for (int NB = 0; NB <= emx::FUSED_ENS_MAX_BLOBS; ++NB, ++n) {
            const emx::Shape s = emx::pick_shape(D, D);
            const int tile = emx::fused_ens_blobs_tile_rule(D, NB), gpb = (emx::FUSED_ENS_THREADS / 64) * (64 / s.G);
            const size_t lds = emx::fused_ens_blobs_lds_bytes(D, NB);
            if (lds > 48 * 1024 || lds < (size_t)tile * ((D | 1) * 8 + 12)) { ++bad; std::printf("lds %d %d\n", D, NB); }
            if (tile < gpb || tile % gpb != 0 || tile > emx::FUSED_ENS_THREADS) { ++bad; std::printf("tile %d %d\n", D, NB); }
            if (NB == 0 && (tile != emx::fused_ens_tile_rule(D) || lds != emx::fused_ens_lds_bytes(D))) { ++bad; std::printf("nb0 %d\n", D); }
        }
    std::printf("checked %d\n", n);
    return bad;
}
""")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "rules")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-x", "hip"] + ["-I" + d for d in get_include()] + [str(src), "-o", exe],
                   check=True, timeout=900, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "checked %d" % (256 * 33) in r.stdout, r.stdout
    assert "static_assert(lds <= 48 * 1024" in open(HEADER).read()


def test_argument_checks_touch_no_device():
    for bad in (-1, 33, 2.5, True, "4", None):
        with pytest.raises(ValueError, match="nblobs"):
            DeviceFused(0x1000, 5, nblobs=bad)
        with pytest.raises(ValueError, match="nblobs"):
            compile_fused_ensemble(SOURCE, "DiagModel", 5, nblobs=bad)
        with pytest.raises(ValueError, match="nblobs"):
            DeviceFusedLibrary("/nowhere.so", "x", 5, nblobs=bad)
    assert DeviceFused(0x1000, 5).nblobs == 0 and DeviceFused(0x1000, 5, None, 32).nblobs == 32
    assert DeviceFused(0x1000, 5, nblobs=np.int64(3)).nblobs == 3
    t = DeviceFused(0x1000, 5, nblobs=3)
    with pytest.raises(ValueError, match="blobs_dtype"):
        emcee_amd.EnsembleSampler(32, 5, t, blobs_dtype=np.float32)
    for ok in (None, np.float64, "f8"):
        s = emcee_amd.EnsembleSampler(32, 5, t, blobs_dtype=ok)
        assert s._ens is None and s._device_nblobs == 3
    assert emcee_amd.EnsembleSampler(32, 5, DeviceFused(0x1000, 5), blobs_dtype=np.float32)._device_nblobs == 0
    with pytest.raises(TypeError) as e:
        EnsembleBatch(4, 32, 5, t)
    assert "DeviceFused" in str(e.value)
    with pytest.raises(TypeError) as e:
        PTSampler(4, 16, 5, t, nbatch=2)
    assert "DeviceFused" in str(e.value)
    with pytest.raises(ValueError) as e:
        emcee_amd.EnsembleSampler(32, 5, t, distributed=True)
    assert "DeviceFused" in str(e.value) and "distributed" in str(e.value)


def test_states_and_backend_without_device_blobs_behave_as_before():
    """the lazy `blobs` of the device states and the backend's `blobs` property: host blobs pass through untouched"""
    import pickle
    from emcee_amd.backends import Backend
    from emcee_amd.state import DeviceState
    st = DeviceState(None, blobs=np.arange(3.0))
    assert np.array_equal(st.blobs, np.arange(3.0)) and len(st) == 4
    st._invalidate()
    assert st.blobs is not None                    # host blobs are the sampler's to replace, not the device's
    b = Backend()
    b.reset(4, 2)
    assert not b.has_blobs() and b.blobs is None
    b.grow(3, np.zeros((4, 2)))
    assert b.has_blobs() and b.blobs.shape == (3, 4, 2)
    c = pickle.loads(pickle.dumps(b))
    assert c.has_blobs() and c.blobs.shape == (3, 4, 2)
    legacy = dict(b.__dict__)
    legacy["blobs"] = legacy.pop("_blobs")         # a pickle written before `blobs` became a property
    d = Backend.__new__(Backend)
    d.__setstate__(legacy)
    assert d.has_blobs() and d.blobs.shape == (3, 4, 2)


def test_the_test_model_compiles(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    so = str(tmp_path / "libuser_ens_blobs.so")
    subprocess.run([hipcc] + ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DUSER_NDIM=3", "-DUSER_NBLOBS=4"] +
                   ["-I" + d for d in get_include()] + [os.path.join(ROOT, "tests", "c", "user_ensemble_fused_blobs.hip"), "-o", so],
                   check=True, timeout=900, capture_output=True)
    _lib.load()
    user = C.CDLL(so)
    for name in ("user_plain", "user_plain_box", "user_blobs", "user_blobs_box", "user_setup", "user_device_pointer", "user_teardown"):
        assert hasattr(user, name)
    assert user.user_nblobs() == 4
