"""Blobs of EnsembleBatch (targets with nblobs > 0), what needs no GPU: a blob functor cross-compiles for gfx950, the launcher's
probe (which launches nothing) accepts its own blob count and refuses another, an old header version and another ndim, the
header and the ctypes descriptor agree, the C ABI declares and exports the new entry points, and every argument check that
must fire before a device is touched."""
import ctypes as C
import os
import re
import shutil
import subprocess
import time

import numpy as np
import pytest

from emcee_amd import EnsembleBatch, PTSampler, _lib, batch, moves, targets
from emcee_amd.targets import BatchCallable, BatchFused, BatchKernel, compile_fused, get_include

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("emx_set_batch_target_fused_blobs", "emx_set_batch_target_callback_blobs", "emx_check_batch_blobs", "emx_get_blobs_batch",
       "emx_summary_batch_plane")

# the GPU tests' functor as a compile_fused source: blobs = {lp, x0 + x1, x0 * x1, member}
SOURCE = r"""
struct WithBlobs {
    __device__ double operator()(const double* x, int ndim, int member, const void* user, double* blobs) const {
        double acc = 0.0;
        for (int d = 0; d < ndim; ++d) acc = acc + x[d] * x[d];
        const double lp = -0.5 * acc;
        blobs[0] = lp;
        blobs[1] = x[0] + x[1];
        blobs[2] = x[0] * x[1];
        blobs[3] = (double)member;
        return lp;
    }
};
struct Plain {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const {
        double acc = 0.0;
        for (int d = 0; d < ndim; ++d) acc = acc + x[d] * x[d];
        return -0.5 * acc;
    }
};
"""


def header_text():
    return open(os.path.join(ROOT, "include", "emx.h")).read()


def header_code():
    return re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)


@pytest.fixture(scope="module")
def cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("blob_cache"))


@pytest.fixture(scope="module")
def built(cache):
    """the blob functor (nblobs 4) and the blob-free one, cross-compiled for gfx950 side by side"""
    t0 = time.time()
    blobs = compile_fused(SOURCE, "WithBlobs", 5, nblobs=4, name="with_blobs5", cache_dir=cache)
    plain = compile_fused(SOURCE, "Plain", 5, name="plain5", cache_dir=cache)
    print("compile_fused: a blob functor and a plain one, ndim 5: %.1f s" % (time.time() - t0))
    return blobs, plain


# ---------------------------------------------------------------------------------------------------------------- compile
def test_a_blob_functor_cross_compiles(built, cache):
    blobs, plain = built
    assert blobs.nblobs == 4 and plain.nblobs == 0 and blobs.path != plain.path
    src = open(os.path.join(os.path.dirname(blobs.path), "with_blobs5.hip")).read()
    assert "EMX_FUSED_BATCH_TARGET_BLOBS(with_blobs5, WithBlobs, 5, 4)" in src
    assert "EMX_FUSED_BATCH_TARGET(plain5, Plain, 5)" in open(os.path.join(os.path.dirname(plain.path), "plain5.hip")).read()
    t = blobs.target(user=1 << 20)
    assert isinstance(t, BatchFused) and t.nblobs == 4 and t.ndim == 5
    assert plain.target().nblobs == 0
    # the device code object carries a gfx950 kernel of the blob instantiation
    raw = open(blobs.path, "rb").read()
    assert b"gfx950" in raw and b"k_small_run" in raw and b"WithBlobs" in raw


def test_nblobs_is_part_of_the_cache_key(built, cache):
    blobs, _ = built
    mtime = os.stat(blobs.path).st_mtime_ns
    again = compile_fused(SOURCE, "WithBlobs", 5, nblobs=4, name="with_blobs5", cache_dir=cache)
    assert again.path == blobs.path and os.stat(again.path).st_mtime_ns == mtime          # nothing was compiled
    other = compile_fused(SOURCE, "WithBlobs", 5, nblobs=5, name="with_blobs5", cache_dir=cache)
    assert other.path != blobs.path and other.nblobs == 5
    with pytest.raises(RuntimeError) as e:              # the four-argument functor under the blob macro: the compiler says so
        compile_fused(SOURCE, "Plain", 5, nblobs=2, name="plain_as_blobs", cache_dir=cache)
    assert "error:" in str(e.value)


def test_the_test_models_compile(tmp_path):
    """tests/c/user_blobs_logprob.hip (the GPU tests' models, all three wrappings) cross-compiles and exports its entry points"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    so = str(tmp_path / "libuser_blobs.so")
    subprocess.run([hipcc] + ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DUSER_NDIM=3"] +
                   ["-I" + d for d in get_include()] + [os.path.join(ROOT, "tests", "c", "user_blobs_logprob.hip"), "-o", so],
                   check=True, timeout=900, capture_output=True)
    _lib.load()
    user = C.CDLL(so)
    for name in ("user_fused_g", "user_fused_g_blobs", "user_fused_x", "user_fused_x_blobs", "user_block_g_blobs", "user_block_x_blobs",
                 "user_setup", "user_device_pointer", "user_ninf", "user_teardown"):
        assert hasattr(user, name)
    assert user.user_nblobs() == 4


# ---------------------------------------------------------------------------------------------------------------- the probe
def _args_bytes(fn, abi, nblobs):
    """sizeof(SmallRunArgs) is internal: exactly one size is the library's"""
    rcs = [fn(C.byref(_lib.FusedLaunch(abi=abi, args_bytes=n, ndim=5, movesel=0, grid=0, nblobs=nblobs))) for n in range(8, 4096, 8)]
    assert sorted(set(rcs)) == [0, 1] and rcs.count(0) == 1
    return 8 * (rcs.index(0) + 1)


def test_the_probe_accepts_its_blob_count_and_refuses_the_rest(built):
    """grid == 0 launches nothing, so the probe runs without a GPU: 0 for this library's values, 4 for another blob count, 1 for
    another header version, 2 for another ndim and 3 for a move selector that is not compiled in (the existing codes)"""
    blobs, plain = built
    txt = open(os.path.join(ROOT, "emcee_amd", "csrc", "emx_fused_target.hpp")).read()
    abi = int(re.search(r"#define EMX_FUSED_ABI (\d+)u", txt).group(1))
    assert abi >= 2                                    # bumped with the grown SmallRunArgs / emx_fused_launch
    fb, fp = blobs.launcher, plain.launcher
    for fn in (fb, fp):
        fn.restype, fn.argtypes = C.c_int, [C.POINTER(_lib.FusedLaunch)]
    nbytes = _args_bytes(fb, abi, 4)
    L = lambda **kw: C.byref(_lib.FusedLaunch(**dict(dict(abi=abi, args_bytes=nbytes, ndim=5, movesel=0, grid=0, nblobs=4), **kw)))  # noqa: E731
    assert fb(L()) == 0 and fb(L(movesel=7)) == 0
    for k in (0, 1, 3, 5, 32):                          # a wrong nblobs, the blob-free 0 included
        assert fb(L(nblobs=k)) == 4
    assert fb(L(abi=abi - 1)) == 1 and fb(L(abi=abi + 1)) == 1           # an old (and a newer) ABI
    assert fb(L(args_bytes=nbytes - 8)) == 1
    assert fb(L(ndim=6)) == 2                          # a wrong ndim, with the existing code
    assert fb(L(movesel=3)) == 3
    # the blob-free launcher: the library's probe always carries `args`, and then a blob count is refused
    args = C.create_string_buffer(nbytes)
    assert _args_bytes(fp, abi, 0) == nbytes
    assert fp(L(nblobs=0, args=C.addressof(args))) == 0
    assert fp(L(nblobs=4, args=C.addressof(args))) == 4
    assert fp(L(nblobs=0, ndim=6, args=C.addressof(args))) == 2


def test_header_and_ctypes_agree_on_the_grown_descriptor():
    body = re.search(r"typedef\s+struct\s+emx_fused_launch\s*\{([^}]*)\}\s*emx_fused_launch\s*;", header_code()).group(1)
    ctype = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "void*": C.c_void_p, "const void*": C.c_void_p}
    want = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"^((?:const\s+)?\w+\s*\*?)\s*(.*)$", decl)
        typ = re.sub(r"\s*\*", "*", m.group(1).strip())
        for name in m.group(2).split(","):
            want.append((name.strip(), ctype[typ]))
    assert want == list(_lib.FusedLaunch._fields_), (want, _lib.FusedLaunch._fields_)
    assert [n for n, _ in want][-2:] == ["nblobs", "reserved"]
    assert C.sizeof(_lib.FusedLaunch) == 64 and _lib.FusedLaunch.nblobs.offset == 56


def test_header_declares_and_library_exports_the_entry_points():
    txt = header_code()
    lib = _lib.load()
    for name in NEW:
        m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, txt)
        assert m, "include/emx.h does not declare %s" % name
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(m.group(1).split(",")), name
        assert hasattr(lib, name)
    assert re.search(r"typedef\s+int\s*\(\s*\*\s*emx_batch_log_prob_blobs_fn\s*\)\s*\(([^)]*)\)", txt)
    params = re.search(r"emx_batch_log_prob_blobs_fn\s*\)\s*\(([^)]*)\)", txt).group(1)
    assert re.search(r"int32_t\s+nblobs\s*,\s*double\s*\*\s*blobs_dev", params) and len(params.split(",")) == 9
    # every one of them is documented, and the macro is public
    raw = header_text()
    for word in NEW + ("what 4", "plane 4", "EMX_FUSED_BATCH_TARGET_BLOBS"):
        assert word in raw, word
    hpp = open(os.path.join(ROOT, "emcee_amd", "csrc", "emx_fused_target.hpp")).read()
    assert re.search(r"#define\s+EMX_FUSED_BATCH_TARGET_BLOBS\(name, Functor, ndim, nblobs\)", hpp)
    # exports equal declarations: what the library exports under emx_ is what the header declares, the new names included
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        exported = set(re.findall(r"\bT (emx_\w+)", out))
        declared = set(re.findall(r"\b(emx_[a-z0-9_]+)\s*\(", txt))
        assert declared == set(_lib.SIGNATURES) and declared <= exported, declared ^ set(_lib.SIGNATURES)
        assert set(NEW) <= exported


# ---------------------------------------------------------------------------------------------------------------- arguments
@pytest.fixture
def no_device(monkeypatch):
    """any attempt to create the device handle fails the test"""
    def refuse(self):
        raise AssertionError("a device was touched before the arguments were checked")
    monkeypatch.setattr(EnsembleBatch, "_handle", refuse)


def test_nblobs_out_of_range_is_refused():
    for bad in (-1, 33, 2.5, True, "4", None):
        with pytest.raises(ValueError, match="nblobs"):
            BatchFused(0x1000, 5, nblobs=bad)
        with pytest.raises(ValueError, match="nblobs"):
            BatchCallable(lambda q: q, nblobs=bad)
        with pytest.raises(ValueError, match="nblobs"):
            BatchKernel(0x1000, nblobs=bad)
        with pytest.raises(ValueError, match="nblobs"):
            compile_fused(SOURCE, "WithBlobs", 5, nblobs=bad)
    assert BatchFused(0x1000, 5).nblobs == 0 and BatchFused(0x1000, 5, nblobs=32).nblobs == 32
    assert BatchCallable(lambda q: q).nblobs == 0 and BatchKernel(0x1000, nblobs=np.int64(3)).nblobs == 3
    assert _lib.MAX_BLOBS == 32
    # the C layer's own bound (host only), and no blobs for a built-in target
    lib = _lib.load()
    msg = C.create_string_buffer(320)
    arr = (_lib.MoveDesc * 1)(moves.StretchMove()._desc(5))
    assert lib.emx_check_batch_blobs(32, 5, _lib.TARGET_FUSED_USER, 1, arr, 4, msg, 320) == 0
    assert lib.emx_check_batch_blobs(32, 5, _lib.TARGET_CALLBACK, 1, arr, 32, msg, 320) == 0
    assert lib.emx_check_batch_blobs(32, 5, _lib.TARGET_FUSED_USER, 1, arr, 0, msg, 320) == 0
    for bad in (-1, 33):
        assert lib.emx_check_batch_blobs(32, 5, _lib.TARGET_FUSED_USER, 1, arr, bad, msg, 320) == -1 and b"blobs" in msg.value
    assert lib.emx_check_batch_blobs(32, 5, _lib.TARGET_ISO, 1, arr, 2, msg, 320) == -1 and b"built-in" in msg.value
    assert lib.emx_check_batch_blobs(32, 5, _lib.TARGET_FUSED_PT, 1, arr, 2, msg, 320) == -1


def test_a_member_that_fits_without_blobs_and_not_with_them_is_refused(no_device):
    """600 x 16 under a StretchMove: the member, one step's plans and the staging rows take 151 880 of the 153 600 bytes a
    workgroup may hold; four blobs a walker are 19 200 more"""
    lib = _lib.load()
    msg = C.create_string_buffer(320)
    arr = (_lib.MoveDesc * 1)(moves.StretchMove()._desc(16))
    assert lib.emx_batch_check(600, 16, _lib.TARGET_FUSED_USER, 1, arr, msg, 320) == 0
    assert lib.emx_check_batch_blobs(600, 16, _lib.TARGET_FUSED_USER, 1, arr, 0, msg, 320) == 0
    assert lib.emx_check_batch_blobs(600, 16, _lib.TARGET_FUSED_USER, 1, arr, 4, msg, 320) == -1
    assert b"LDS" in msg.value and b"4 blobs" in msg.value
    assert lib.emx_check_batch_blobs(600, 16, _lib.TARGET_CALLBACK, 1, arr, 4, msg, 320) == 0      # k_batch_cb keeps no member in LDS
    assert EnsembleBatch(2, 600, 16, BatchFused(0x1000, 16))._h is None
    with pytest.raises(ValueError) as e:
        EnsembleBatch(2, 600, 16, BatchFused(0x1000, 16, nblobs=4))
    assert "LDS" in str(e.value) and "blobs" in str(e.value)


def test_a_trampoline_result_of_the_wrong_shape_names_the_mismatch():
    lp, bl = np.zeros((3, 7)), np.zeros((3, 7, 2))
    out = batch._split_result((lp, bl), 3, 7, 2)
    assert out[0] is lp and out[1] is bl
    assert batch._split_result(np.zeros(21), 3, 7, 0)[1] is None          # (B * n) log-probs are accepted, as before
    with pytest.raises(ValueError, match=r"\(log_prob, blobs\)"):
        batch._split_result(lp, 3, 7, 2)                                 # no blobs returned
    with pytest.raises(ValueError) as e:
        batch._split_result((lp, np.zeros((3, 7, 3))), 3, 7, 2)
    assert "(3, 7, 3)" in str(e.value) and "(3, 7, 2)" in str(e.value)
    with pytest.raises(ValueError) as e:
        batch._split_result((lp, np.zeros((3, 14))), 3, 7, 2)              # the right count in the wrong shape
    assert "(3, 14)" in str(e.value)
    with pytest.raises(ValueError) as e:
        batch._split_result((np.zeros((3, 6)), bl), 3, 7, 2)
    assert "18 values for 3 members x 7 rows" in str(e.value)
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError) as e:
        batch._split_result((torch.zeros(3, 7), torch.zeros(7, 3, 2)), 3, 7, 2)
    assert "(7, 3, 2)" in str(e.value)


def test_ptsampler_refuses_a_target_with_blobs():
    for t in (BatchCallable(lambda q: (q.sum(-1), q[..., :2]), nblobs=2), BatchKernel(0x1000, nblobs=2)):
        with pytest.raises(TypeError) as e:
            PTSampler(4, 16, 3, t, nbatch=2)
        assert "blobs" in str(e.value) and "nblobs" in str(e.value)
    PTSampler(4, 16, 3, BatchCallable(lambda q: q.sum(-1)), nbatch=2)     # the same without blobs is taken


def test_without_blobs_get_blobs_is_none(no_device):
    for t in (targets.IsoGaussian(), BatchFused(0x1000, 5), BatchCallable(lambda q: q.sum(-1))):
        b = EnsembleBatch(4, 32, 5, t)
        assert b.nblobs == 0 and b.get_blobs() is None and b[1].get_blobs() is None
        with pytest.raises(ValueError, match="no blobs"):
            b.get_blob_summary()
        with pytest.raises(ValueError, match="no blobs"):
            b[0].get_blob_summary()
    b = EnsembleBatch(4, 32, 5, BatchFused(0x1000, 5, nblobs=3))
    assert b.nblobs == 3 and b._h is None
    with pytest.raises(AttributeError):                 # blobs, but nothing stored yet: get_chain's error
        b.get_blobs()
    with pytest.raises(ValueError, match="run the sampler"):
        b.get_blob_summary()
