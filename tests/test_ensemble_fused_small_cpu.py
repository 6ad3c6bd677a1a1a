"""Small ensembles of a DeviceFused target (EMX_FUSED_ENSEMBLE_SMALL_TARGET / emx_set_target_fused_small), what needs no GPU: hipcc
cross-compiles both launchers from one source, the small launcher's probe, the eligibility rule emx_small_fused_check against the
LDS formula written out here, the C ABI's declarations, and that a translation unit without the new macro is what it always was."""
import ctypes as C
import os
import re
import shutil
import subprocess
import time

import pytest

import emcee_amd
from emcee_amd import _lib
from emcee_amd.targets import DeviceFused, DeviceFusedLibrary, compile_fused_ensemble, get_include

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "emcee_amd", "csrc", "emx_fused_ensemble.hpp")

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
    __device__ double operator()(const double* x, int ndim, int member, const void* user, double* blobs) const {
        const double lp = (*this)(x, ndim, member, user);
        blobs[0] = lp;
        blobs[1] = x[0];
        blobs[2] = x[ndim - 1];
        return lp;
    }
};
"""

STRETCH, DE, SNOOKER, GAUSS, WALK = 0, 1, 2, 3, 5
LDS_MAX = 150 * 1024


def _abi(name):
    return int(re.search(r"#define %s (0x[0-9a-fA-F]+|\d+)u" % name, open(HEADER).read()).group(1), 0)


@pytest.fixture(scope="module")
def cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("fused_small_cache"))


@pytest.fixture(scope="module")
def built(cache):
    t0 = time.time()
    lib = compile_fused_ensemble(SOURCE, "DiagModel", 5, name="diag5", cache_dir=cache)
    print("compile_fused_ensemble, small=True: one model, ndim 5: %.1f s" % (time.time() - t0))
    return lib


@pytest.fixture(scope="module")
def built_blobs(cache):
    return compile_fused_ensemble(SOURCE, "DiagModel", 5, name="diag5b", cache_dir=cache, nblobs=3)


@pytest.fixture(scope="module")
def built_plain(cache):
    t0 = time.time()
    lib = compile_fused_ensemble(SOURCE, "DiagModel", 5, name="diag5", cache_dir=cache, small=False)
    print("compile_fused_ensemble, small=False: one model, ndim 5: %.1f s" % (time.time() - t0))
    return lib


def _exports(path):
    """the names of this file's entry points that the library exports"""
    _lib.load()                                      # one HIP runtime per process: the library's (torch's) first
    lib = C.CDLL(path)
    names = ("diag5", "diag5_small", "user_fused_a", "user_small_a", "user_fused_blobs", "user_small_blobs", "user_rows_a", "user_setup",
             "user_device_pointer", "user_teardown")
    return set(n for n in names if hasattr(lib, n))


def test_one_source_exports_both_launchers(built, built_plain):
    assert isinstance(built, DeviceFusedLibrary) and built.small_name == "diag5_small" and built.small_launcher is not None
    assert {"diag5", "diag5_small"} <= _exports(built.path)
    t = built.target(user=1 << 20)
    assert isinstance(t, DeviceFused) and t.fn_ptr is built.launcher and t.small_fn is built.small_launcher
    # small=False: today's library -- another cache entry, the half-step launcher alone, no k_small_run in the code object
    assert built_plain.path != built.path and built_plain.small_name is None and built_plain.small_launcher is None
    ex = _exports(built_plain.path)
    assert "diag5" in ex and "diag5_small" not in ex and not hasattr(built_plain.lib, "diag5_small")
    assert built_plain.target().small_fn is None
    assert b"k_small_run" in open(built.path, "rb").read() and b"k_small_run" not in open(built_plain.path, "rb").read()


def _small_args_bytes(fn, abi, ndim, nblobs):
    rcs = [fn(C.byref(_lib.FusedLaunch(abi=abi, args_bytes=n, ndim=ndim, movesel=STRETCH, grid=0, nblobs=nblobs))) for n in range(8, 4096, 8)]
    assert sorted(set(rcs)) == [0, 1] and rcs.count(0) == 1      # sizeof(SmallRunArgs) is internal: exactly one value is taken
    return 8 * (rcs.index(0) + 1)


def test_the_small_probe_checks_version_ndim_and_blob_count(built, built_blobs):
    """grid == 0 launches nothing, so the probe runs without a GPU"""
    abi = _abi("EMX_FUSED_ENSEMBLE_SMALL_ABI")
    for lib, K in ((built, 0), (built_blobs, 3)):
        fn = lib.small_launcher
        fn.restype, fn.argtypes = C.c_int, [C.POINTER(_lib.FusedLaunch)]
        nbytes = _small_args_bytes(fn, abi, 5, K)

        def probe(**kw):
            d = dict(abi=abi, args_bytes=nbytes, ndim=5, movesel=STRETCH, grid=0, nblobs=K)
            d.update(kw)
            return fn(C.byref(_lib.FusedLaunch(**d)))
        assert probe() == 0 and probe(movesel=7) == 0 and probe(reserved=1) == 0 and probe(movesel=7, reserved=1) == 0
        assert probe(abi=abi + 1) == 1
        assert probe(ndim=6) == 2
        assert probe(nblobs=K + 1) == 4 and probe(nblobs=2) == 4
        assert probe(movesel=DE) == 3 and probe(movesel=GAUSS) == 3 and probe(reserved=2) == 3
        # the other launcher types' constants are refused: the descriptor of a batch launcher starts with the same fields
        for other in ("emx_fused_target.hpp", "emx_pt_fused.hpp", "emx_fused_ensemble.hpp"):
            txt = open(os.path.join(ROOT, "emcee_amd", "csrc", other)).read()
            for m in re.finditer(r"#define (EMX_FUSED\w*_ABI) (0x[0-9a-fA-F]+|\d+)u", txt):
                if m.group(1) != "EMX_FUSED_ENSEMBLE_SMALL_ABI":
                    assert int(m.group(2), 0) != abi and probe(abi=int(m.group(2), 0)) == 1
        # a descriptor that asks for a launch without arguments, or with more than one workgroup, launches nothing
        assert probe(grid=1, threads=256) == 3 and probe(grid=2, threads=256) == 3


def test_the_half_step_launchers_answers_are_unchanged(built, built_plain):
    abi = _abi("EMX_FUSED_ENSEMBLE_ABI")

    class Launch(C.Structure):
        _fields_ = _lib.FusedEnsembleLaunch._fields_
    answers = []
    for lib in (built, built_plain):
        fn = lib.launcher
        fn.restype, fn.argtypes = C.c_int, [C.POINTER(Launch)]
        rcs = [fn(C.byref(Launch(abi=abi, args_bytes=n, ndim=5, move=0, grid=0))) for n in range(8, 4096, 8)]
        assert sorted(set(rcs)) == [0, 1] and rcs.count(0) == 1
        nbytes = 8 * (rcs.index(0) + 1)
        got = [fn(C.byref(Launch(abi=abi + 1, args_bytes=nbytes, ndim=5, move=0, grid=0))),
               fn(C.byref(Launch(abi=abi, args_bytes=nbytes, ndim=6, move=0, grid=0)))]
        got += [fn(C.byref(Launch(abi=abi, args_bytes=nbytes, ndim=5, move=mv, grid=0))) for mv in range(6)]
        got.append(fn(C.byref(Launch(abi=_abi("EMX_FUSED_ENSEMBLE_SMALL_ABI"), args_bytes=nbytes, ndim=5, move=0, grid=0))))
        answers.append((nbytes, got))
    assert answers[0] == answers[1] and answers[0][1] == [1, 2, 0, 0, 0, 0, 0, 3, 1]


# ---------------------------------------------------------------------------------------------- the eligibility rule
def _small_batch(N):
    return max(1, min(64, 1024 // N))


def _need(N, D, min_splits, nblobs):
    """emx_small_host.hpp written out: the ensemble (rows, log-probs, accept counts and flags), small_batch(N) steps' plans (three
    doubles and four ints an entry), 64 bytes of slack; the staging rows of the largest split at D | 1 doubles and a factor each,
    16 bytes of alignment; nblobs doubles a walker"""
    B = _small_batch(N)
    rows = (N + min_splits - 1) // min_splits
    return N * (D * 8 + 8 + 4 + 1) + B * N * (3 * 8 + 4 * 4) + 64 + 16 + rows * ((D | 1) * 8 + 8) + N * nblobs * 8


def _check(N, D, moves, rng, nblobs):
    arr = (_lib.MoveDesc * len(moves))(*[_lib.MoveDesc(kind=k, nsplits=s, reserved=r) for k, s, r in moves])
    msg = C.create_string_buffer(512)
    rc = _lib.load().emx_small_fused_check(N, D, len(moves), arr, rng, nblobs, msg, 512)
    assert rc in (0, -1) and (rc == 0) == (msg.value == b"")
    return rc == 0, msg.value.decode()


@pytest.mark.parametrize("nblobs", [0, 3])
@pytest.mark.parametrize("ndim", [5, 16, 33, 130])
def test_the_check_is_the_lds_formula(ndim, nblobs):
    for rng in (_lib.RNG_MT19937, _lib.RNG_PHILOX):
        for moves, smin in (([(STRETCH, 2, 0)], 2), ([(STRETCH, 3, 0)], 3), ([(DE, 2, 0), (SNOOKER, 4, 0)], 2)):
            fits = [N for N in range(4, 4097) if _need(N, ndim, smin, nblobs) <= LDS_MAX]
            largest = max(fits)
            assert 4 < largest < 4096
            print("ndim %d, nblobs %d, least nsplits %d: the largest admitted nwalkers is %d (%d bytes)" %
                  (ndim, nblobs, smin, largest, _need(largest, ndim, smin, nblobs)))
            ok, _ = _check(largest, ndim, moves, rng, nblobs)
            assert ok
            ok, why = _check(largest + 1, ndim, moves, rng, nblobs)
            assert not ok and "LDS" in why and str(largest + 1) in why
            if rng == _lib.RNG_PHILOX and smin == 2 and len(moves) == 1:      # the whole range once: the predicate IS the formula
                for N in range(4, 4097, 7):
                    assert _check(N, ndim, moves, rng, nblobs)[0] == (_need(N, ndim, smin, nblobs) <= LDS_MAX), N


def test_the_check_refuses_what_the_kernel_does_not_run():
    mt, ph = _lib.RNG_MT19937, _lib.RNG_PHILOX
    assert _check(32, 5, [(STRETCH, 2, 0)], mt, 0)[0] and _check(32, 5, [(STRETCH, 2, 0)], ph, 3)[0]
    # a DEMove whose complement is below 2: 3 walkers in 2 splits leave a complement of 1
    assert _check(4, 5, [(DE, 2, 0)], ph, 0)[0]
    ok, why = _check(3, 5, [(DE, 2, 0)], ph, 0)
    assert not ok and "complement" in why
    # a GaussianMove: Philox mode only
    assert _check(32, 5, [(GAUSS, 1, 0)], ph, 0)[0]
    ok, why = _check(32, 5, [(GAUSS, 1, 0)], mt, 0)
    assert not ok and "GaussianMove" in why
    ok, why = _check(32, 5, [(STRETCH, 2, 0), (GAUSS, 1, 0)], mt, 0)
    assert not ok and "GaussianMove" in why
    # WalkMove / KDEMove schedules stay on the general path
    for kind in (WALK, WALK + 1):
        ok, why = _check(32, 5, [(kind, 2, 0)], ph, 0)
        assert not ok and "only" in why
    ok, why = _check(32, 5, [(STRETCH, 2, 0)], ph, 33)
    assert not ok and "33" in why and "blobs" in why
    assert not _check(32, 5, [(STRETCH, 2, 0)], _lib.RNG_INPUTS, 0)[0]
    assert not _check(4097, 1, [(STRETCH, 2, 0)], ph, 0)[0] and not _check(32, 257, [(STRETCH, 2, 0)], ph, 0)[0]
    assert not _check(32, 5, [], ph, 0)[0]


def test_where_the_kernel_pays():
    """the measured rule of profiles/ensemble_fused_small.md, a narrowing of the check and never a widening of it"""
    pays = _lib.load().emx_small_fused_pays
    ph, mt = _lib.RNG_PHILOX, _lib.RNG_MT19937
    for N, D in ((32, 5), (100, 10), (128, 8), (200, 5), (256, 4), (512, 2)):          # measured faster with Philox plans
        assert pays(N, D, ph) == 1 and pays(N, D, mt) == 1
    for N, D in ((64, 16), (64, 32), (256, 16), (606, 16), (1000, 5), (103, 10), (94, 11)):      # measured slower, or beyond the measured bound
        assert pays(N, D, ph) == 0
    for N, D in ((256, 16), (606, 16), (1000, 5)):                                       # measured faster with the host's plans
        assert pays(N, D, mt) == 1
    assert pays(64, 17, mt) == 0 and pays(64, 130, mt) == 0


def test_header_declares_the_small_entry_points():
    raw = open(os.path.join(ROOT, "include", "emx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"int\s+emx_set_target_fused_small\s*\(\s*emx_ctx\s*\*\s*\w*\s*,\s*emx_fused_small_fn\s+\w+\s*\)\s*;", txt)
    assert re.search(r"typedef\s+int\s*\(\s*\*\s*emx_fused_small_fn\s*\)\s*\(\s*const\s+struct\s+emx_fused_launch\s*\*\s*\)\s*;", txt)
    assert re.search(r"int\s+emx_small_fused_check\s*\(", txt) and re.search(r"int\s+emx_small_info\s*\(\s*emx_ctx\s*\*\s*\w*\s*,\s*int64_t\s+\w+\[4\]\s*\)\s*;", txt)
    lib = _lib.load()
    assert re.search(r"int\s+emx_small_fused_pays\s*\(\s*int64_t\s+\w+\s*,\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*\)\s*;", txt)
    for name in ("emx_set_target_fused_small", "emx_small_fused_check", "emx_small_fused_pays", "emx_small_info"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert "never the one-workgroup kernel" not in raw


def test_device_fused_without_small_fn_constructs_as_before():
    t = DeviceFused(0x1000, 5)
    assert t.small_fn is None and t.nblobs == 0 and t.user_address() is None
    assert DeviceFused(0x1000, 5, None, 2).nblobs == 2                      # the positional form of the earlier signature
    assert DeviceFused(0x1000, 5, small_fn=0x2000).small_fn == 0x2000
    for bad in (0, True, "x", 1.5):
        with pytest.raises(TypeError):
            DeviceFused(0x1000, 5, small_fn=bad)
    s = emcee_amd.EnsembleSampler(32, 5, DeviceFused(0x1000, 5, small_fn=0x2000))      # accepted, and still no device touched
    assert s._ens is None


def test_the_test_models_compile(tmp_path):
    """tests/c/user_ensemble_fused_small.hip (the GPU tests' models, every wrapping) cross-compiles and exports its entry points"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    so = str(tmp_path / "libuser_small.so")
    subprocess.run([hipcc] + ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DUSER_NDIM=3", "-DUSER_NBLOBS=2"] +
                   ["-I" + d for d in get_include()] + [os.path.join(ROOT, "tests", "c", "user_ensemble_fused_small.hip"), "-o", so],
                   check=True, timeout=900, capture_output=True)
    assert {"user_fused_a", "user_small_a", "user_fused_blobs", "user_small_blobs", "user_rows_a", "user_setup", "user_device_pointer",
            "user_teardown"} <= _exports(so)
