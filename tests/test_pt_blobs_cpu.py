"""Blobs of a PTSampler, what needs no GPU: the argument checks made before any device is touched, the new entry points in include/emx.h
and _lib.SIGNATURES, emx_pt_fused_check_blobs against emx_pt_fused_check, the grid == 0 probe of a launcher emitted by
EMX_FUSED_PT_TARGET_BLOBS, compile_fused_pt's cache key, and pt_lds_layout (the one definition of k_pt_run's LDS map) exercised
alone in a host program built with -fsanitize=address,undefined."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from emcee_amd import PTSampler, _lib, moves
from emcee_amd.targets import BatchCallable, BatchKernel, PTFused, PTFusedLibrary, compile_fused_pt, get_include

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "emcee_amd", "csrc")

SOURCE = r"""
struct Like {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const {
        double acc = 0.0;
        for (int d = 0; d < ndim; ++d) acc = acc + x[d] * x[d];
        return -0.5 * acc;
    }
    __device__ double operator()(const double* x, int ndim, int member, const void* user, double* blobs) const {
        const double L = (*this)(x, ndim, member, user);
        blobs[0] = L;
        blobs[1] = (double)member;
        return L;
    }
};
"""


class Launch(C.Structure):          # emx_pt_fused_launch of include/emx.h
    _fields_ = [("abi", C.c_uint32), ("args_bytes", C.c_uint32), ("ndim", C.c_int32), ("movesel", C.c_int32), ("grid", C.c_int32),
                ("threads", C.c_int32), ("lds_bytes", C.c_uint64), ("hip_stream", C.c_void_p), ("args", C.c_void_p),
                ("user", C.c_void_p), ("has_prior", C.c_int32), ("nblobs", C.c_int32)]


def _hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_constructors_and_argument_checks_touch_no_device():
    t = PTFused(0x1000, 3, nblobs=4)
    assert t.nblobs == 4 and PTFused(0x1000, 3).nblobs == 0 and PTFused(0x1000, 3, None, 2, has_prior=True).nblobs == 2
    for bad in (-1, 33, 2.0, True):
        with pytest.raises(ValueError, match=r"PTFused: nblobs is an integer in \[0, 32\]"):
            PTFused(0x1000, 3, nblobs=bad)
        with pytest.raises(ValueError, match=r"compile_fused_pt: nblobs is an integer in \[0, 32\]"):
            compile_fused_pt(SOURCE, "Like", 3, nblobs=bad)
    with pytest.raises(ValueError) as e:
        PTFused(0x1000, 3, nblobs=2, ndata=7)
    assert str(e.value) == "PTFused: a target that sums over data (ndata) carries no blobs; nblobs=2 is refused"
    with pytest.raises(ValueError) as e:
        compile_fused_pt(SOURCE, "Like", 3, data=True, nblobs=2)
    assert str(e.value) == "compile_fused_pt: a data target (data=True) carries no blobs; nblobs=2 is refused"
    with pytest.raises(ValueError, match="data=True"):
        PTFusedLibrary("p", "n", 3, False, data=True, nblobs=2)
    # a likelihood with blobs is taken (and no device is touched); the sampler knows the count
    for like in (t, BatchKernel(0x2000, nblobs=4), BatchCallable(lambda q: (q.sum(-1), q[..., :4]), nblobs=4)):
        pt = PTSampler(4, 16, 3, like, nbatch=2, seeds=[1, 2], blobs=True)
        assert pt.nblobs == 4 and pt._h is None and pt._b._h is None
        with pytest.raises(TypeError) as e:              # recording is asked for
            PTSampler(4, 16, 3, like, nbatch=2, seeds=[1, 2])
        assert "blobs=True" in str(e.value) and "nblobs = 4" in str(e.value)
    with pytest.raises(ValueError, match="nblobs = 0"):
        PTSampler(4, 16, 3, PTFused(0x1000, 3), nbatch=2, blobs=True)
    pt = PTSampler(4, 16, 3, PTFused(0x1000, 3), nbatch=2)
    assert pt.nblobs == 0 and pt.get_blobs() is None
    # the prior produces none
    for prior in (BatchKernel(0x2000, nblobs=1), BatchCallable(lambda q: (q.sum(-1), q[..., :1]), nblobs=1)):
        with pytest.raises(TypeError) as e:
            PTSampler(4, 16, 3, BatchKernel(0x3000, nblobs=4), log_prior=prior, blobs=True)
        assert "prior produces no blobs" in str(e.value) and "nblobs = 1" in str(e.value)


def test_header_and_signatures_have_the_new_entry_points():
    raw = open(os.path.join(ROOT, "include", "emx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib.load()
    for name, nargs in (("emx_pt_set_target_fused_blobs", 5), ("emx_pt_fused_check_blobs", 8), ("emx_pt_get_blobs", 2)):
        m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs
    body = re.search(r"typedef\s+struct\s+emx_pt_fused_launch\s*\{([^}]*)\}\s*emx_pt_fused_launch\s*;", txt).group(1)
    names = re.findall(r"(\w+)\s*(?:,|;)", body)
    assert [f for f, _ in Launch._fields_] == names           # the blob count sits behind has_prior, in what was the struct's padding
    assert C.sizeof(Launch) == 64
    hdr = open(os.path.join(CSRC, "emx_pt_fused.hpp")).read()
    assert "#define EMX_FUSED_PT_TARGET_BLOBS(name, LikeFunctor, PriorFunctor, ndim, nblobs)" in hdr
    assert int(re.search(r"#define EMX_FUSED_PT_ABI (\d+)u", hdr).group(1)) >= 3


def test_check_blobs_with_no_blobs_is_emx_pt_fused_check():
    lib = _lib.load()
    a, b = C.create_string_buffer(512), C.create_string_buffer(512)
    schedules = [[moves.StretchMove()], [moves.DEMove(), moves.DESnookerMove()], [moves.StretchMove(nsplits=4)], [moves.GaussianMove(0.3)]]
    refused = accepted = 0
    for T in (0, 1, 2, 8, 16, 64):
        for N in (1, 2, 33, 64, 90, 100, 256, 1024):
            for D in (1, 3, 16, 32):
                for sched in schedules:
                    arr = (_lib.MoveDesc * len(sched))(*[m._desc(D) for m in sched])
                    a.value = b.value = b""
                    ra = lib.emx_pt_fused_check(T, N, D, len(sched), arr, a, 512)
                    rb = lib.emx_pt_fused_check_blobs(T, N, D, len(sched), arr, 0, b, 512)
                    assert ra == rb and a.value == b.value, (T, N, D)
                    refused += ra != 0
                    accepted += ra == 0
    assert refused > 50 and accepted > 50
    assert lib.emx_pt_fused_check_blobs(4, 32, 5, 0, None, 0, a, 512) == -1 and a.value == b"no moves"
    arr = (_lib.MoveDesc * 1)(moves.StretchMove()._desc(5))
    assert lib.emx_pt_fused_check_blobs(4, 32, 5, 1, arr, 32, a, 512) == 0
    for bad in (-1, 33):
        assert lib.emx_pt_fused_check_blobs(4, 32, 5, 1, arr, bad, a, 512) == -1 and b"blobs" in a.value


def test_a_shape_that_fits_only_without_blobs_is_refused_by_name():
    lib = _lib.load()
    T, D = 8, 16
    msg = C.create_string_buffer(512)
    arr = (_lib.MoveDesc * 1)(moves.StretchMove()._desc(D))
    N = max(n for n in range(2 * D, 1024, 2) if lib.emx_pt_fused_check(T, n, D, 1, arr, msg, 512) == 0)
    assert lib.emx_pt_fused_check_blobs(T, N, D, 1, arr, 8, msg, 512) == -1
    assert b"LDS" in msg.value and b"8 blobs" in msg.value and re.search(rb"\d+ bytes > \d+; \d+ without the blobs", msg.value)
    with pytest.raises(ValueError) as e:
        PTSampler(T, N, D, PTFused(0x1000, D, nblobs=8), moves=moves.StretchMove(), blobs=True)
    assert "LDS" in str(e.value) and "8 blobs" in str(e.value)
    # fewer walkers make room: the staging rows are halved before an object is refused
    assert lib.emx_pt_fused_check_blobs(T, N // 2, D, 1, arr, 8, msg, 512) == 0


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """tests/c/user_pt_fused_blobs.hip (the GPU tests' models) cross-compiled for gfx950 at ndim 3"""
    so = str(tmp_path_factory.mktemp("pt_fused_blobs") / "libuser_pt_fused_blobs.so")
    subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DUSER_NDIM=3"] +
                   ["-I" + d for d in get_include()] + [os.path.join(ROOT, "tests", "c", "user_pt_fused_blobs.hip"), "-o", so],
                   check=True, timeout=900, capture_output=True)
    _lib.load()
    return C.CDLL(so)


def test_the_probe_of_the_blob_launcher(models):
    """grid == 0 launches nothing, so the probe runs without a GPU"""
    for name in ("pt_fused_g", "pt_fused_gp", "pt_fused_g_blobs", "pt_fused_gp_blobs", "user_block_g", "user_block_g_blobs", "user_block_p",
                 "user_setup", "user_device_pointer", "user_teardown", "user_nblobs"):
        assert hasattr(models, name)
    assert models.user_nblobs() == 4
    txt = open(os.path.join(CSRC, "emx_pt_fused.hpp")).read()
    abi = int(re.search(r"#define EMX_FUSED_PT_ABI (\d+)u", txt).group(1))
    fn = models.pt_fused_g_blobs
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(Launch)]
    rcs = [fn(C.byref(Launch(abi=abi, args_bytes=n, ndim=3, movesel=0, grid=0, nblobs=4))) for n in range(8, 4096, 8)]
    assert sorted(set(rcs)) == [0, 1] and rcs.count(0) == 1      # sizeof(PtRunArgs) is internal: exactly one size is the library's
    nbytes = 8 * (rcs.index(0) + 1)
    ok = dict(abi=abi, args_bytes=nbytes, ndim=3, movesel=0, grid=0)
    assert fn(C.byref(Launch(nblobs=4, **ok))) == 0 and fn(C.byref(Launch(nblobs=4, **dict(ok, movesel=7)))) == 0
    for other in (0, 3, 5, 32):                                 # another count than the one compiled in
        assert fn(C.byref(Launch(nblobs=other, **ok))) == 4
    assert fn(C.byref(Launch(nblobs=4, **dict(ok, abi=abi + 1)))) == 1
    assert fn(C.byref(Launch(nblobs=4, **dict(ok, ndim=4)))) == 2
    assert fn(C.byref(Launch(nblobs=4, **dict(ok, movesel=3)))) == 3
    for name, has, nb in (("pt_fused_g", 0, 0), ("pt_fused_gp", 1, 0), ("pt_fused_g_blobs", 0, 4), ("pt_fused_gp_blobs", 1, 4)):
        f = getattr(models, name)
        f.restype, f.argtypes = C.c_int, [C.POINTER(Launch)]
        L = Launch(has_prior=-1, nblobs=nb, **ok)
        assert f(C.byref(L)) == 0 and L.has_prior == has          # the probe reports the prior functor
        assert f(C.byref(Launch(nblobs=4 - nb, **ok))) == 4       # and a blob-free launcher refuses a count as well


def test_compile_fused_pt_keys_the_cache_on_nblobs_only_when_there_are_blobs(tmp_path):
    cache = str(tmp_path)
    plain = compile_fused_pt(SOURCE, "Like", 3, name="like3", cache_dir=cache)
    mtime = os.stat(plain.path).st_mtime_ns
    zero = compile_fused_pt(SOURCE, "Like", 3, name="like3", cache_dir=cache, nblobs=0)
    assert zero.path == plain.path and os.stat(zero.path).st_mtime_ns == mtime          # the same cached library: nothing was compiled
    assert plain.nblobs == zero.nblobs == 0 and "nblobs" not in vars(plain) and plain.target().nblobs == 0
    src = open(os.path.join(os.path.dirname(plain.path), "like3.hip")).read()
    assert "EMX_FUSED_PT_TARGET(like3, Like, emx::NoFusedPrior, 3)" in src and "_BLOBS" not in src
    two = compile_fused_pt(SOURCE, "Like", 3, name="like3", cache_dir=cache, nblobs=2)
    assert two.path != plain.path and two.nblobs == 2 and not two.has_prior
    src = open(os.path.join(os.path.dirname(two.path), "like3.hip")).read()
    assert src.startswith("#include <emx_pt_fused.hpp>") and "EMX_FUSED_PT_TARGET_BLOBS(like3, Like, emx::NoFusedPrior, 3, 2)" in src
    t = two.target(user=1 << 20)
    assert isinstance(t, PTFused) and t.nblobs == 2 and t.user_address() == 1 << 20 and t.fn_ptr is two.launcher
    assert PTSampler(4, 16, 3, t, nbatch=2, blobs=True).nblobs == 2
    assert compile_fused_pt(SOURCE, "Like", 3, name="like3", cache_dir=cache, nblobs=3).path not in (plain.path, two.path)


LAYOUT_PROGRAM = r"""
// pt_lds_layout alone: K = 0 is the layout as it was (every offset and the total), the blob regions lie behind every other region,
// are 8-byte aligned, do not overlap and end inside `total`; every region is touched in a heap block of `total` bytes
#include <emx_pt_fused.hpp>

#include <cstdio>
#include <cstring>
#include <vector>

int main() {
    long checked = 0;
    for (int T : {1, 2, 3, 8, 16})
        for (int N : {2, 32, 33, 64, 100})
            for (int D : {1, 3, 7, 16})
                for (int B : {1, 2, 5})
                    for (int R : {1, 7, 17, 32}) {
                        const emx::PtLds z = emx::pt_lds_layout(T, N, D, B, R), z0 = emx::pt_lds_layout(T, N, D, B, R, 0);
                        if (std::memcmp(&z, &z0, sizeof z) != 0) return 1;
                        size_t before = z.total;
                        for (int K : {1, 2, 4, 31, 32}) {
                            const emx::PtLds o = emx::pt_lds_layout(T, N, D, B, R, K);
                            const uint32_t* a = &o.X;
                            const uint32_t* b = &z.X;
                            for (int f = 0; f < 23; ++f)
                                if (a[f] != b[f]) return 2;                                   // K moves no offset of a blob-free object
                            const size_t wb = (size_t)T * N * K * 8, sb = (size_t)T * R * K * 8;
                            if (o.wbl % 8 || o.sbl % 8 || o.wbl < (size_t)o.accs + (size_t)T * N) return 3;
                            if (o.sbl != o.wbl + wb || o.sbl + sb > o.total || o.total % 16 || o.total < z.total + wb + sb - 16) return 4;
                            if (o.total <= before && K > 1) return 5;                         // more blobs, more bytes
                            before = o.total;
                            std::vector<unsigned char> lds(o.total, 0);
                            double* w = reinterpret_cast<double*>(lds.data() + o.wbl);
                            double* s = reinterpret_cast<double*>(lds.data() + o.sbl);
                            for (size_t e = 0; e < (size_t)T * N * K; ++e) w[e] = 1.0;
                            for (size_t e = 0; e < (size_t)T * R * K; ++e) s[e] = 2.0;
                            for (size_t e = 0; e < (size_t)T * N; ++e)
                                if (lds[o.accs + e] != 0) return 6;                           // the last blob-free region stays untouched
                            ++checked;
                        }
                    }
    std::printf("pt_lds_layout: %ld layouts checked\n", checked);
    return 0;
}
"""


def test_pt_lds_layout_alone_under_the_sanitizers(tmp_path):
    src = tmp_path / "pt_lds_layout_check.hip"
    src.write_text(LAYOUT_PROGRAM)
    exe = str(tmp_path / "pt_lds_layout_check")
    r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=undefined"] + ["-I" + d for d in get_include()] + [str(src), "-o", exe],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stderr or r.stdout)[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, (r.returncode, (r.stderr or r.stdout)[-4000:])
    assert re.search(r"pt_lds_layout: \d+ layouts checked", r.stdout) and "runtime error" not in r.stderr
