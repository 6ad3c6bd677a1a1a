"""Fused tempered targets of PTSampler that sum over an object's data (targets.PTFused(..., ndata=) / compile_fused_pt(..., data=True);
emx_pt_fused_data.hpp), what needs no GPU: hipcc cross-compiles the user's translation unit, the launcher answers the grid = 0 probe,
the compiler's diagnostics, the C ABI's declaration and the argument checks made before any device is touched."""
import ctypes as C
import os
import re
import shutil
import subprocess
import time

import numpy as np
import pytest

import emcee_amd
from emcee_amd import EnsembleBatch, PTSampler, _lib
from emcee_amd.targets import PTFused, PTFusedLibrary, compile_fused_pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "emcee_amd", "csrc")

# a straight-line fit: the record of an object, the model with base and term, a prior functor, and a plain one-lane likelihood
SOURCE = r"""
struct line_rec { const double* x; const double* y; const double* ivar; int ntemps; };
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
        const line_rec* r = (const line_rec*)user;
        return line_term(x, r + member / r->ntemps, k);
    }
};
struct LineFunctor {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const { return line_base(x, ndim); }
};
struct Prior {
    __device__ double operator()(const double* x, int ndim, int, const void*) const { return x[0] > 9.0 ? -__builtin_inf() : 0.0; }
};
extern "C" __attribute__((visibility("default"))) int line_rec_bytes() { return (int)sizeof(line_rec); }
"""


class Launch(C.Structure):          # emx_pt_fused_launch of include/emx.h
    _fields_ = [("abi", C.c_uint32), ("args_bytes", C.c_uint32), ("ndim", C.c_int32), ("movesel", C.c_int32), ("grid", C.c_int32),
                ("threads", C.c_int32), ("lds_bytes", C.c_uint64), ("hip_stream", C.c_void_p), ("args", C.c_void_p),
                ("user", C.c_void_p), ("has_prior", C.c_int32)]


def _abis():
    vals = {}
    for hpp in sorted(os.listdir(CSRC)):
        if hpp.endswith(".hpp"):
            for m in re.finditer(r"#define (EMX_FUSED\w*_ABI) (0x[0-9a-fA-F]+|\d+)u", open(os.path.join(CSRC, hpp)).read()):
                assert m.group(1) not in vals
                vals[m.group(1)] = int(m.group(2), 0)
    return vals


@pytest.fixture(scope="module")
def cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("pt_fused_data_cache"))


@pytest.fixture(scope="module")
def built(cache):
    t0 = time.time()
    lib = compile_fused_pt(SOURCE, "LineModel", 5, name="line5", cache_dir=cache, data=True)
    print("compile_fused_pt(data=True): one model, ndim 5: %.1f s" % (time.time() - t0))
    return lib


@pytest.fixture(scope="module")
def built_prior(cache):
    return compile_fused_pt(SOURCE, "LineModel", 5, prior="Prior", name="line5p", cache_dir=cache, data=True)


@pytest.fixture(scope="module")
def plain(cache):
    return compile_fused_pt(SOURCE, "LineFunctor", 5, name="plain5", cache_dir=cache)


def _args_bytes(fn, abi):
    """sizeof(PtRunArgs) is internal: exactly one size is the library's"""
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(Launch)]
    rcs = [fn(C.byref(Launch(abi=abi, args_bytes=n, ndim=5, movesel=0, grid=0))) for n in range(8, 4096, 8)]
    assert sorted(set(rcs)) == [0, 1] and rcs.count(0) == 1
    return 8 * (rcs.index(0) + 1)


def test_compile_fused_pt_data_builds_caches_and_exports_the_launcher(built, built_prior, plain, cache):
    assert isinstance(built, PTFusedLibrary) and built.ndim == 5 and built.name == "line5" and built.data and not built.has_prior
    assert built_prior.data and built_prior.has_prior and built_prior.path != built.path
    assert os.path.exists(built.path) and built.path.startswith(cache)
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", built.path], capture_output=True, text=True, check=True).stdout
        assert re.search(r"\bT line5\b", out), out
    assert built.lib.line_rec_bytes() == 32            # the user's own extern "C" function of the source
    src = open(os.path.join(os.path.dirname(built.path), "line5.hip")).read()
    assert src.startswith("#include <emx_pt_fused_data.hpp>") and "EMX_FUSED_PT_DATA_TARGET(line5, LineModel, emx::NoFusedPrior, 5)" in src
    # a second call compiles nothing
    mtime = os.stat(built.path).st_mtime_ns
    t0 = time.time()
    again = compile_fused_pt(SOURCE, "LineModel", 5, name="line5", cache_dir=cache, data=True)
    assert again.path == built.path and os.stat(again.path).st_mtime_ns == mtime and time.time() - t0 < 2.0
    # data=False keeps the translation unit, the key and the cached library it always had: the key of the parent's compile_fused_pt
    assert built.path != plain.path and not plain.data
    assert compile_fused_pt(SOURCE, "LineFunctor", 5, name="plain5", cache_dir=cache, data=False).path == plain.path
    import hashlib
    from emcee_amd import _build, targets
    h = hashlib.sha256(repr(("pt", SOURCE, "LineFunctor", None, 5, "plain5") + (targets.FUSED_FLAGS + [],)).encode())
    for d in _build.DEPS:
        if d.endswith((".hpp", ".h")):
            h.update(open(d, "rb").read())
    assert os.path.basename(os.path.dirname(plain.path)) == h.hexdigest()[:24]
    assert os.path.join(CSRC, "emx_pt_fused_data.hpp") in _build.DEPS      # the new header is part of every build's and cache's hash
    src = open(os.path.join(os.path.dirname(plain.path), "plain5.hip")).read()
    assert src.startswith("#include <emx_pt_fused.hpp>") and "EMX_FUSED_PT_TARGET(plain5, LineFunctor, emx::NoFusedPrior, 5)" in src
    # target()
    t = built.target(user=1 << 20, ndata=[3, 0, 70])
    assert isinstance(t, PTFused) and t.ndim == 5 and t.user_address() == 1 << 20 and t.ndata == (3, 0, 70) and t.has_prior is False
    assert t.fn_ptr is built.launcher
    assert built.target(ndata=17).ndata == 17
    assert built.target(ndata=np.array([1, 2], dtype=np.int32)).ndata == (1, 2)
    with pytest.raises(ValueError) as e:               # a data library needs the counts, any other refuses them
        built.target(user=1 << 20)
    assert "data=True" in str(e.value)
    with pytest.raises(ValueError) as e:
        plain.target(ndata=4)
    assert "data=True" in str(e.value)
    assert plain.target().ndata is None


def test_the_launcher_answers_the_probe(built, built_prior, plain):
    """grid == 0 launches nothing, so the probe runs without a GPU"""
    vals = _abis()
    abi, abi_plain = vals["EMX_FUSED_PT_DATA_ABI"], vals["EMX_FUSED_PT_ABI"]
    fn = built.launcher
    nbytes = _args_bytes(fn, abi)                      # exactly one args_bytes is accepted
    good = dict(abi=abi, args_bytes=nbytes, ndim=5, movesel=0, grid=0)
    assert fn(C.byref(Launch(**good))) == 0
    assert fn(C.byref(Launch(**dict(good, abi=abi + 1)))) == 1
    assert fn(C.byref(Launch(**dict(good, ndim=6)))) == 2
    assert fn(C.byref(Launch(**dict(good, movesel=7)))) == 0
    assert fn(C.byref(Launch(**dict(good, movesel=3)))) == 3          # a selector that does not exist
    assert fn(None) == 1
    for lib, has in ((built, 0), (built_prior, 1)):                   # the probe reports the prior functor
        f = lib.launcher
        f.restype, f.argtypes = C.c_int, [C.POINTER(Launch)]
        L = Launch(**dict(good, has_prior=-1))
        assert f(C.byref(L)) == 0 and L.has_prior == has
    # a plain EMX_FUSED_PT_TARGET launcher probed with the data ABI answers 1, and the reverse
    pf = plain.launcher
    assert _args_bytes(pf, abi_plain) == nbytes                       # one PtRunArgs
    assert pf(C.byref(Launch(**dict(good, abi=abi_plain)))) == 0
    assert pf(C.byref(Launch(**good))) == 1
    assert fn(C.byref(Launch(**dict(good, abi=abi_plain)))) == 1


def test_a_launcher_with_the_stretch_kernel_alone_refuses_the_any_selector(cache):
    """the _MOVES variant: a selector that was not compiled in answers 3"""
    tail_src = SOURCE + "\nEMX_FUSED_PT_DATA_TARGET_MOVES(line5s, LineModel, emx::NoFusedPrior, 5, EMX_FUSED_MOVES_STRETCH)\n"
    lib = compile_fused_pt(tail_src, "LineModel", 5, name="line5_both", cache_dir=cache, data=True)
    fn = lib.lib.line5s
    abi = _abis()["EMX_FUSED_PT_DATA_ABI"]
    nbytes = _args_bytes(fn, abi)
    assert fn(C.byref(Launch(abi=abi, args_bytes=nbytes, ndim=5, movesel=0, grid=0))) == 0
    assert fn(C.byref(Launch(abi=abi, args_bytes=nbytes, ndim=5, movesel=7, grid=0))) == 3


def test_the_data_abi_differs_from_every_other_fused_abi():
    vals = _abis()
    assert "EMX_FUSED_PT_DATA_ABI" in vals and "EMX_FUSED_PT_ABI" in vals and len(vals) >= 8
    others = [v for k, v in vals.items() if k != "EMX_FUSED_PT_DATA_ABI"]
    assert vals["EMX_FUSED_PT_DATA_ABI"] not in others


def test_a_model_without_term_fails_with_the_one_line_diagnostic(cache):
    src = "struct NoTerm { __device__ double base(const double* x, int ndim, int member, const void* user) const { return 0.0; } };"
    with pytest.raises(RuntimeError) as e:
        compile_fused_pt(src, "NoTerm", 5, cache_dir=cache, data=True)
    msg = str(e.value)
    assert "error:" in msg and "hipcc failed" in msg
    assert re.search(r"EMX_FUSED_PT_DATA_TARGET: the model needs\s+__device__ double term\(", msg)
    assert "the model needs  __device__ double base(" not in msg
    with pytest.raises(RuntimeError) as e:             # the plain functor is not a data model
        compile_fused_pt(SOURCE, "LineFunctor", 5, cache_dir=cache, data=True)
    assert "error:" in str(e.value) and "the model needs  __device__ double base(" in str(e.value)


def test_argument_checks_touch_no_device(built, plain):
    for bad in (True, 2.0, -1, 2 ** 31, "7", [3, True], [3, 2.5], [3, -1], [3, 2 ** 31], np.array([1.0, 2.0])):
        with pytest.raises(ValueError) as e:
            PTFused(0x1000, 5, ndata=bad)
        assert "ndata" in str(e.value), bad
    assert PTFused(0x1000, 5, ndata=0).ndata == 0
    assert PTFused(0x1000, 5, ndata=2 ** 31 - 1).ndata == 2 ** 31 - 1
    assert PTFused(0x1000, 5, ndata=np.int64(9)).ndata == 9
    assert PTFused(0x1000, 5, ndata=(4, 0, 2 ** 31 - 1)).ndata == (4, 0, 2 ** 31 - 1)
    assert PTFused(0x1000, 5).ndata is None
    # the length of ndata against the number of OBJECTS, when the sampler takes the target
    t = PTFused(0x1000, 5, ndata=[1, 2, 3])
    with pytest.raises(ValueError) as e:
        PTSampler(4, 16, 5, t, nbatch=4)
    assert "nbatch = 4" in str(e.value) and "got 3" in str(e.value)
    with pytest.raises(ValueError):
        PTSampler(4, 16, 5, PTFused(0x1000, 5, ndata=[1] * 12), nbatch=3)      # one a member is not one an object
    for ok in (t, PTFused(0x1000, 5, ndata=6), built.target(ndata=[5, 0, 9])):
        pt = PTSampler(4, 16, 5, ok, nbatch=3, seeds=[1, 2, 3])               # accepted, and still no device touched
        assert pt._h is None and pt._b._h is None and pt._fused is ok
    with pytest.raises(ValueError) as e:               # ndim of the launcher != the sampler's
        PTSampler(4, 16, 6, t, nbatch=3)
    assert "ndim 5" in str(e.value) and "ndim 6" in str(e.value)
    # target(ndata=) on a plain library, and a data library without it
    with pytest.raises(ValueError):
        plain.target(ndata=[1, 2, 3])
    with pytest.raises(ValueError):
        built.target()
    # outside PTSampler a PTFused stays the TypeError it is, with or without ndata
    with pytest.raises(TypeError) as e:
        EnsembleBatch(3, 16, 5, t)
    assert "PTSampler" in str(e.value)
    with pytest.raises(TypeError):
        emcee_amd.EnsembleSampler(16, 5, t)


def test_header_declares_the_setter():
    raw = open(os.path.join(ROOT, "include", "emx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"int\s+emx_pt_set_target_fused_data\s*\(\s*emx_batch\s*\*\s*\w*\s*,\s*emx_pt_fused_fn\s+\w+\s*,\s*int32_t\s+\w+\s*,"
                     r"\s*const\s+void\s*\*\s*\w+\s*,\s*const\s+int64_t\s*\*\s*\w+\s*\)\s*;", txt)
    lib = _lib.load()
    assert hasattr(lib, "emx_pt_set_target_fused_data") and "emx_pt_set_target_fused_data" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["emx_pt_set_target_fused_data"][1]) == 5
    assert os.path.exists(os.path.join(CSRC, "emx_pt_fused_data.hpp"))
    for hpp in ("emx_fused_target_data.hpp", "emx_fused_ensemble_data.hpp"):      # PTSampler is no longer out of their scope
        scope = re.search(r"// Out of scope:[^\n]*", open(os.path.join(CSRC, hpp)).read()).group(0).split("(")[0]
        assert "PTSampler" not in scope
