"""What compile_fused, compile_fused_ensemble and compile_fused_pt hand to the shared build (targets._compile_cached: header, the
translation unit's tail, the parts of the cache key, the launcher's name, the flags) for every combination of their arguments,
and the library object each returns -- held to a literal table captured from the code as it was before the three functions
shared their identifier check, default name and data branch: a plain build keeps the key, and with it the cached library, it
always had.  Nothing is compiled and nothing is opened.  The same file pins the TypeError / ValueError texts of the three fused
target classes, the three library classes and the compile functions, one bad value for each check."""
import ctypes
import itertools

import numpy as np
import pytest

from emcee_amd import targets
from emcee_amd.targets import (BatchFused, BatchFusedLibrary, DeviceFused, DeviceFusedLibrary, PTFused, PTFusedLibrary, compile_fused,
                               compile_fused_ensemble, compile_fused_pt)

SRC = "struct F {};"


class _NothingOpened(object):
    def __getattr__(self, name):
        return 0x1000 + len(name)      # a non-null address stands for the launcher


@pytest.fixture
def recorded(monkeypatch):
    calls = []

    def fake(what, header, source, tail, key_parts, name, flags, cache_dir):
        assert source == SRC and cache_dir is None
        calls.append((what, header, tail, key_parts, name, list(flags)))
        return "/nowhere/lib%s.so" % name

    monkeypatch.setattr(targets, "_compile_cached", fake)
    monkeypatch.setattr(targets._lib, "load", lambda: None)
    monkeypatch.setattr(ctypes, "CDLL", lambda path: _NothingOpened())
    return calls


def _named(kw, named):
    return dict(kw, name="mine", flags=("-DK=1", 2)) if named else kw


def _matrix():
    """-> [(case, function, args, kwargs)]"""
    out = []
    for nblobs, data, named in itertools.product((0, 2), (False, True), (False, True)):
        if nblobs and data:
            continue
        out.append(("batch nblobs=%d data=%d named=%d" % (nblobs, data, named), compile_fused, (SRC, "ns::F", 5),
                    _named(dict(nblobs=nblobs, data=data), named)))
    for nblobs, small, data, named in itertools.product((0, 2), (True, False), (False, True), (False, True)):
        if nblobs and data:
            continue
        out.append(("ensemble nblobs=%d small=%d data=%d named=%d" % (nblobs, small, data, named), compile_fused_ensemble, (SRC, "ns::F", 5),
                    _named(dict(nblobs=nblobs, small=small, data=data), named)))
    for prior, data, named in itertools.product((None, "Pr"), (False, True), (False, True)):
        out.append(("pt prior=%s data=%d named=%d" % (prior, data, named), compile_fused_pt, (SRC, "ns::F", 5),
                    _named(dict(prior=prior, data=data), named)))
    return out


def _run_matrix(calls):
    got = []
    for case, fn, args, kw in _matrix():
        del calls[:]
        lib = fn(*args, **kw)
        assert len(calls) == 1, case
        attrs = {k: v for k, v in vars(lib).items() if k != "lib"}
        got.append((case,) + calls[0] + (type(lib).__name__, sorted(attrs.items())))
    return got


# (case, what, header, tail, key_parts, name, flags, library class, the library's attributes)
EXPECTED = [
    ('batch nblobs=0 data=0 named=0',
     'compile_fused',
     'emx_fused_target.hpp',
     'EMX_FUSED_BATCH_TARGET(emx_fused_ns__F_5, ns::F, 5)',
     ('batch', 'struct F {};', 'ns::F', 5, 'emx_fused_ns__F_5'),
     'emx_fused_ns__F_5',
     [],
     'BatchFusedLibrary',
     [('data', False), ('launcher', 4113), ('name', 'emx_fused_ns__F_5'), ('nblobs', 0), ('ndim', 5), ('path', '/nowhere/libemx_fused_ns__F_5.so')]),
    ('batch nblobs=0 data=0 named=1',
     'compile_fused',
     'emx_fused_target.hpp',
     'EMX_FUSED_BATCH_TARGET(mine, ns::F, 5)',
     ('batch', 'struct F {};', 'ns::F', 5, 'mine'),
     'mine',
     ['-DK=1', '2'],
     'BatchFusedLibrary',
     [('data', False), ('launcher', 4100), ('name', 'mine'), ('nblobs', 0), ('ndim', 5), ('path', '/nowhere/libmine.so')]),
    ('batch nblobs=0 data=1 named=0',
     'compile_fused',
     'emx_fused_target_data.hpp',
     'EMX_FUSED_BATCH_DATA_TARGET(emx_fused_ns__F_5, ns::F, 5)',
     ('batch', 'struct F {};', 'ns::F', 5, 'emx_fused_ns__F_5', 'data target'),
     'emx_fused_ns__F_5',
     [],
     'BatchFusedLibrary',
     [('data', True), ('launcher', 4113), ('name', 'emx_fused_ns__F_5'), ('nblobs', 0), ('ndim', 5), ('path', '/nowhere/libemx_fused_ns__F_5.so')]),
    ('batch nblobs=0 data=1 named=1',
     'compile_fused',
     'emx_fused_target_data.hpp',
     'EMX_FUSED_BATCH_DATA_TARGET(mine, ns::F, 5)',
     ('batch', 'struct F {};', 'ns::F', 5, 'mine', 'data target'),
     'mine',
     ['-DK=1', '2'],
     'BatchFusedLibrary',
     [('data', True), ('launcher', 4100), ('name', 'mine'), ('nblobs', 0), ('ndim', 5), ('path', '/nowhere/libmine.so')]),
    ('batch nblobs=2 data=0 named=0',
     'compile_fused',
     'emx_fused_target.hpp',
     'EMX_FUSED_BATCH_TARGET_BLOBS(emx_fused_ns__F_5, ns::F, 5, 2)',
     ('batch', 'struct F {};', 'ns::F', 5, 'emx_fused_ns__F_5', 'nblobs', 2),
     'emx_fused_ns__F_5',
     [],
     'BatchFusedLibrary',
     [('data', False), ('launcher', 4113), ('name', 'emx_fused_ns__F_5'), ('nblobs', 2), ('ndim', 5), ('path', '/nowhere/libemx_fused_ns__F_5.so')]),
    ('batch nblobs=2 data=0 named=1',
     'compile_fused',
     'emx_fused_target.hpp',
     'EMX_FUSED_BATCH_TARGET_BLOBS(mine, ns::F, 5, 2)',
     ('batch', 'struct F {};', 'ns::F', 5, 'mine', 'nblobs', 2),
     'mine',
     ['-DK=1', '2'],
     'BatchFusedLibrary',
     [('data', False), ('launcher', 4100), ('name', 'mine'), ('nblobs', 2), ('ndim', 5), ('path', '/nowhere/libmine.so')]),
    ('ensemble nblobs=0 small=1 data=0 named=0',
     'compile_fused_ensemble',
     'emx_fused_ensemble.hpp',
     'EMX_FUSED_ENSEMBLE_TARGET(emx_fused_ensemble_ns__F_5, ns::F, 5)\nEMX_FUSED_ENSEMBLE_SMALL_TARGET(emx_fused_ensemble_ns__F_5_small, ns::F, 5)',
     ('ensemble', 'struct F {};', 'ns::F', 5, 'emx_fused_ensemble_ns__F_5'),
     'emx_fused_ensemble_ns__F_5',
     [],
     'DeviceFusedLibrary',
     [('data', False),
      ('launcher', 4122),
      ('name', 'emx_fused_ensemble_ns__F_5'),
      ('nblobs', 0),
      ('ndim', 5),
      ('path', '/nowhere/libemx_fused_ensemble_ns__F_5.so'),
      ('small_launcher', 4128),
      ('small_name', 'emx_fused_ensemble_ns__F_5_small')]),
    ('ensemble nblobs=0 small=1 data=0 named=1',
     'compile_fused_ensemble',
     'emx_fused_ensemble.hpp',
     'EMX_FUSED_ENSEMBLE_TARGET(mine, ns::F, 5)\nEMX_FUSED_ENSEMBLE_SMALL_TARGET(mine_small, ns::F, 5)',
     ('ensemble', 'struct F {};', 'ns::F', 5, 'mine'),
     'mine',
     ['-DK=1', '2'],
     'DeviceFusedLibrary',
     [('data', False),
      ('launcher', 4100),
      ('name', 'mine'),
      ('nblobs', 0),
      ('ndim', 5),
      ('path', '/nowhere/libmine.so'),
      ('small_launcher', 4106),
      ('small_name', 'mine_small')]),
    ('ensemble nblobs=0 small=1 data=1 named=0',
     'compile_fused_ensemble',
     'emx_fused_ensemble_data.hpp',
     'EMX_FUSED_ENSEMBLE_DATA_TARGET(emx_fused_ensemble_ns__F_5, ns::F, 5)',
     ('ensemble', 'struct F {};', 'ns::F', 5, 'emx_fused_ensemble_ns__F_5', 'data target'),
     'emx_fused_ensemble_ns__F_5',
     [],
     'DeviceFusedLibrary',
     [('data', True),
      ('launcher', 4122),
      ('name', 'emx_fused_ensemble_ns__F_5'),
      ('nblobs', 0),
      ('ndim', 5),
      ('path', '/nowhere/libemx_fused_ensemble_ns__F_5.so'),
      ('small_launcher', None),
      ('small_name', None)]),
    ('ensemble nblobs=0 small=1 data=1 named=1',
     'compile_fused_ensemble',
     'emx_fused_ensemble_data.hpp',
     'EMX_FUSED_ENSEMBLE_DATA_TARGET(mine, ns::F, 5)',
     ('ensemble', 'struct F {};', 'ns::F', 5, 'mine', 'data target'),
     'mine',
     ['-DK=1', '2'],
     'DeviceFusedLibrary',
     [('data', True),
      ('launcher', 4100),
      ('name', 'mine'),
      ('nblobs', 0),
      ('ndim', 5),
      ('path', '/nowhere/libmine.so'),
      ('small_launcher', None),
      ('small_name', None)]),
    ('ensemble nblobs=0 small=0 data=0 named=0',
     'compile_fused_ensemble',
     'emx_fused_ensemble.hpp',
     'EMX_FUSED_ENSEMBLE_TARGET(emx_fused_ensemble_ns__F_5, ns::F, 5)',
     ('ensemble', 'struct F {};', 'ns::F', 5, 'emx_fused_ensemble_ns__F_5', 'half-step launcher only'),
     'emx_fused_ensemble_ns__F_5',
     [],
     'DeviceFusedLibrary',
     [('data', False),
      ('launcher', 4122),
      ('name', 'emx_fused_ensemble_ns__F_5'),
      ('nblobs', 0),
      ('ndim', 5),
      ('path', '/nowhere/libemx_fused_ensemble_ns__F_5.so'),
      ('small_launcher', None),
      ('small_name', None)]),
    ('ensemble nblobs=0 small=0 data=0 named=1',
     'compile_fused_ensemble',
     'emx_fused_ensemble.hpp',
     'EMX_FUSED_ENSEMBLE_TARGET(mine, ns::F, 5)',
     ('ensemble', 'struct F {};', 'ns::F', 5, 'mine', 'half-step launcher only'),
     'mine',
     ['-DK=1', '2'],
     'DeviceFusedLibrary',
     [('data', False),
      ('launcher', 4100),
      ('name', 'mine'),
      ('nblobs', 0),
      ('ndim', 5),
      ('path', '/nowhere/libmine.so'),
      ('small_launcher', None),
      ('small_name', None)]),
    ('ensemble nblobs=0 small=0 data=1 named=0',
     'compile_fused_ensemble',
     'emx_fused_ensemble_data.hpp',
     'EMX_FUSED_ENSEMBLE_DATA_TARGET(emx_fused_ensemble_ns__F_5, ns::F, 5)',
     ('ensemble', 'struct F {};', 'ns::F', 5, 'emx_fused_ensemble_ns__F_5', 'data target'),
     'emx_fused_ensemble_ns__F_5',
     [],
     'DeviceFusedLibrary',
     [('data', True),
      ('launcher', 4122),
      ('name', 'emx_fused_ensemble_ns__F_5'),
      ('nblobs', 0),
      ('ndim', 5),
      ('path', '/nowhere/libemx_fused_ensemble_ns__F_5.so'),
      ('small_launcher', None),
      ('small_name', None)]),
    ('ensemble nblobs=0 small=0 data=1 named=1',
     'compile_fused_ensemble',
     'emx_fused_ensemble_data.hpp',
     'EMX_FUSED_ENSEMBLE_DATA_TARGET(mine, ns::F, 5)',
     ('ensemble', 'struct F {};', 'ns::F', 5, 'mine', 'data target'),
     'mine',
     ['-DK=1', '2'],
     'DeviceFusedLibrary',
     [('data', True),
      ('launcher', 4100),
      ('name', 'mine'),
      ('nblobs', 0),
      ('ndim', 5),
      ('path', '/nowhere/libmine.so'),
      ('small_launcher', None),
      ('small_name', None)]),
    ('ensemble nblobs=2 small=1 data=0 named=0',
     'compile_fused_ensemble',
     'emx_fused_ensemble.hpp',
     'EMX_FUSED_ENSEMBLE_TARGET_BLOBS(emx_fused_ensemble_ns__F_5, ns::F, 5, 2)\n'
     'EMX_FUSED_ENSEMBLE_SMALL_TARGET_BLOBS(emx_fused_ensemble_ns__F_5_small, ns::F, 5, 2)',
     ('ensemble', 'struct F {};', 'ns::F', 5, 'emx_fused_ensemble_ns__F_5', 'nblobs', 2),
     'emx_fused_ensemble_ns__F_5',
     [],
     'DeviceFusedLibrary',
     [('data', False),
      ('launcher', 4122),
      ('name', 'emx_fused_ensemble_ns__F_5'),
      ('nblobs', 2),
      ('ndim', 5),
      ('path', '/nowhere/libemx_fused_ensemble_ns__F_5.so'),
      ('small_launcher', 4128),
      ('small_name', 'emx_fused_ensemble_ns__F_5_small')]),
    ('ensemble nblobs=2 small=1 data=0 named=1',
     'compile_fused_ensemble',
     'emx_fused_ensemble.hpp',
     'EMX_FUSED_ENSEMBLE_TARGET_BLOBS(mine, ns::F, 5, 2)\nEMX_FUSED_ENSEMBLE_SMALL_TARGET_BLOBS(mine_small, ns::F, 5, 2)',
     ('ensemble', 'struct F {};', 'ns::F', 5, 'mine', 'nblobs', 2),
     'mine',
     ['-DK=1', '2'],
     'DeviceFusedLibrary',
     [('data', False),
      ('launcher', 4100),
      ('name', 'mine'),
      ('nblobs', 2),
      ('ndim', 5),
      ('path', '/nowhere/libmine.so'),
      ('small_launcher', 4106),
      ('small_name', 'mine_small')]),
    ('ensemble nblobs=2 small=0 data=0 named=0',
     'compile_fused_ensemble',
     'emx_fused_ensemble.hpp',
     'EMX_FUSED_ENSEMBLE_TARGET_BLOBS(emx_fused_ensemble_ns__F_5, ns::F, 5, 2)',
     ('ensemble', 'struct F {};', 'ns::F', 5, 'emx_fused_ensemble_ns__F_5', 'nblobs', 2, 'half-step launcher only'),
     'emx_fused_ensemble_ns__F_5',
     [],
     'DeviceFusedLibrary',
     [('data', False),
      ('launcher', 4122),
      ('name', 'emx_fused_ensemble_ns__F_5'),
      ('nblobs', 2),
      ('ndim', 5),
      ('path', '/nowhere/libemx_fused_ensemble_ns__F_5.so'),
      ('small_launcher', None),
      ('small_name', None)]),
    ('ensemble nblobs=2 small=0 data=0 named=1',
     'compile_fused_ensemble',
     'emx_fused_ensemble.hpp',
     'EMX_FUSED_ENSEMBLE_TARGET_BLOBS(mine, ns::F, 5, 2)',
     ('ensemble', 'struct F {};', 'ns::F', 5, 'mine', 'nblobs', 2, 'half-step launcher only'),
     'mine',
     ['-DK=1', '2'],
     'DeviceFusedLibrary',
     [('data', False),
      ('launcher', 4100),
      ('name', 'mine'),
      ('nblobs', 2),
      ('ndim', 5),
      ('path', '/nowhere/libmine.so'),
      ('small_launcher', None),
      ('small_name', None)]),
    ('pt prior=None data=0 named=0',
     'compile_fused_pt',
     'emx_pt_fused.hpp',
     'EMX_FUSED_PT_TARGET(emx_pt_fused_ns__F_5, ns::F, emx::NoFusedPrior, 5)',
     ('pt', 'struct F {};', 'ns::F', None, 5, 'emx_pt_fused_ns__F_5'),
     'emx_pt_fused_ns__F_5',
     [],
     'PTFusedLibrary',
     [('data', False),
      ('has_prior', False),
      ('launcher', 4116),
      ('name', 'emx_pt_fused_ns__F_5'),
      ('ndim', 5),
      ('path', '/nowhere/libemx_pt_fused_ns__F_5.so')]),
    ('pt prior=None data=0 named=1',
     'compile_fused_pt',
     'emx_pt_fused.hpp',
     'EMX_FUSED_PT_TARGET(mine, ns::F, emx::NoFusedPrior, 5)',
     ('pt', 'struct F {};', 'ns::F', None, 5, 'mine'),
     'mine',
     ['-DK=1', '2'],
     'PTFusedLibrary',
     [('data', False), ('has_prior', False), ('launcher', 4100), ('name', 'mine'), ('ndim', 5), ('path', '/nowhere/libmine.so')]),
    ('pt prior=None data=1 named=0',
     'compile_fused_pt',
     'emx_pt_fused_data.hpp',
     'EMX_FUSED_PT_DATA_TARGET(emx_pt_fused_ns__F_5, ns::F, emx::NoFusedPrior, 5)',
     ('pt', 'struct F {};', 'ns::F', None, 5, 'emx_pt_fused_ns__F_5', 'data target'),
     'emx_pt_fused_ns__F_5',
     [],
     'PTFusedLibrary',
     [('data', True),
      ('has_prior', False),
      ('launcher', 4116),
      ('name', 'emx_pt_fused_ns__F_5'),
      ('ndim', 5),
      ('path', '/nowhere/libemx_pt_fused_ns__F_5.so')]),
    ('pt prior=None data=1 named=1',
     'compile_fused_pt',
     'emx_pt_fused_data.hpp',
     'EMX_FUSED_PT_DATA_TARGET(mine, ns::F, emx::NoFusedPrior, 5)',
     ('pt', 'struct F {};', 'ns::F', None, 5, 'mine', 'data target'),
     'mine',
     ['-DK=1', '2'],
     'PTFusedLibrary',
     [('data', True), ('has_prior', False), ('launcher', 4100), ('name', 'mine'), ('ndim', 5), ('path', '/nowhere/libmine.so')]),
    ('pt prior=Pr data=0 named=0',
     'compile_fused_pt',
     'emx_pt_fused.hpp',
     'EMX_FUSED_PT_TARGET(emx_pt_fused_ns__F_5, ns::F, Pr, 5)',
     ('pt', 'struct F {};', 'ns::F', 'Pr', 5, 'emx_pt_fused_ns__F_5'),
     'emx_pt_fused_ns__F_5',
     [],
     'PTFusedLibrary',
     [('data', False),
      ('has_prior', True),
      ('launcher', 4116),
      ('name', 'emx_pt_fused_ns__F_5'),
      ('ndim', 5),
      ('path', '/nowhere/libemx_pt_fused_ns__F_5.so')]),
    ('pt prior=Pr data=0 named=1',
     'compile_fused_pt',
     'emx_pt_fused.hpp',
     'EMX_FUSED_PT_TARGET(mine, ns::F, Pr, 5)',
     ('pt', 'struct F {};', 'ns::F', 'Pr', 5, 'mine'),
     'mine',
     ['-DK=1', '2'],
     'PTFusedLibrary',
     [('data', False), ('has_prior', True), ('launcher', 4100), ('name', 'mine'), ('ndim', 5), ('path', '/nowhere/libmine.so')]),
    ('pt prior=Pr data=1 named=0',
     'compile_fused_pt',
     'emx_pt_fused_data.hpp',
     'EMX_FUSED_PT_DATA_TARGET(emx_pt_fused_ns__F_5, ns::F, Pr, 5)',
     ('pt', 'struct F {};', 'ns::F', 'Pr', 5, 'emx_pt_fused_ns__F_5', 'data target'),
     'emx_pt_fused_ns__F_5',
     [],
     'PTFusedLibrary',
     [('data', True),
      ('has_prior', True),
      ('launcher', 4116),
      ('name', 'emx_pt_fused_ns__F_5'),
      ('ndim', 5),
      ('path', '/nowhere/libemx_pt_fused_ns__F_5.so')]),
    ('pt prior=Pr data=1 named=1',
     'compile_fused_pt',
     'emx_pt_fused_data.hpp',
     'EMX_FUSED_PT_DATA_TARGET(mine, ns::F, Pr, 5)',
     ('pt', 'struct F {};', 'ns::F', 'Pr', 5, 'mine', 'data target'),
     'mine',
     ['-DK=1', '2'],
     'PTFusedLibrary',
     [('data', True), ('has_prior', True), ('launcher', 4100), ('name', 'mine'), ('ndim', 5), ('path', '/nowhere/libmine.so')]),
]


def test_every_combination_reaches_the_shared_build_as_it_always_did(recorded):
    got = _run_matrix(recorded)
    assert [g[0] for g in got] == [e[0] for e in EXPECTED]
    wrong = [(g, e) for g, e in zip(got, EXPECTED) if g != e]
    assert not wrong, "got, expected: %r" % wrong[:3]


def test_the_table_covers_the_matrix():
    cases = [e[0] for e in EXPECTED]
    assert len(cases) == len(set(cases)) == 6 + 12 + 8
    assert {e[1] for e in EXPECTED} == {"compile_fused", "compile_fused_ensemble", "compile_fused_pt"}
    assert {e[2] for e in EXPECTED} == {"emx_fused_target.hpp", "emx_fused_target_data.hpp", "emx_fused_ensemble.hpp", "emx_fused_ensemble_data.hpp",
                                        "emx_pt_fused.hpp", "emx_pt_fused_data.hpp"}
    # a key never depends on how a default is spelt: the plain builds carry no marker of blobs, data or the small launcher
    plain = [e for e in EXPECTED if "nblobs=2" not in e[0] and "data=1" not in e[0] and "small=0" not in e[0]]
    assert all(len(e[4]) == (6 if e[1] == "compile_fused_pt" else 5) for e in plain)


class _HostTensor(object):
    is_cuda = False

    def data_ptr(self):
        return 64


FN = 0x1000          # a non-null address: what the classes take for a launcher
LAUNCHER = "a ctypes function or a non-null address"
USER = "'s user is a device pointer: None, an integer, a ctypes.c_void_p or a torch CUDA tensor"
NBLOBS = ": nblobs is an integer in [0, 32] (float64 blobs a sample); got 33"
NDATA = ": ndata is an integer in [0, 2**31) (the data the target's term runs over), or None; got -1"

REFUSALS = [
    (lambda: DeviceFused(0, 5), TypeError, "DeviceFused needs an emx_fused_ensemble_fn: " + LAUNCHER),
    (lambda: DeviceFused(ctypes.c_void_p(0), 5), TypeError, "DeviceFused needs an emx_fused_ensemble_fn: " + LAUNCHER),
    (lambda: DeviceFused(True, 5), TypeError, "DeviceFused needs an emx_fused_ensemble_fn: " + LAUNCHER),
    (lambda: DeviceFused(FN, 257), TypeError, "DeviceFused needs the ndim its launcher was compiled for, an integer in [1, 256]; got 257"),
    (lambda: DeviceFused(FN, 5, user="x"), TypeError, "DeviceFused" + USER),
    (lambda: DeviceFused(FN, 5, user=True), TypeError, "DeviceFused" + USER),
    (lambda: DeviceFused(FN, 5, user=_HostTensor()), TypeError, "DeviceFused's user tensor must live on the GPU (the functor reads it on the device)"),
    (lambda: DeviceFused(FN, 5, small_fn=0), TypeError,
     "DeviceFused's small_fn is an EMX_FUSED_ENSEMBLE_SMALL_TARGET launcher: a ctypes function, a non-null address or None"),
    (lambda: DeviceFused(FN, 5, nblobs=33), ValueError, "DeviceFused" + NBLOBS),
    (lambda: DeviceFused(FN, 5, ndata=-1), ValueError, "DeviceFused" + NDATA),
    (lambda: DeviceFused(FN, 5, nblobs=2, ndata=7), ValueError,
     "DeviceFused: a target that sums over data (ndata) carries no blobs; nblobs=2 is refused"),
    (lambda: DeviceFused(FN, 5, small_fn=FN, ndata=7), ValueError,
     "DeviceFused: a target that sums over data (ndata) has no one-workgroup form; small_fn is refused"),
    (lambda: BatchFused(0, 5), TypeError, "BatchFused needs an emx_fused_batch_fn: " + LAUNCHER),
    (lambda: BatchFused(FN, 0), TypeError, "BatchFused needs the ndim its launcher was compiled for, an integer >= 1; got 0"),
    (lambda: BatchFused(FN, 5, user=1.5), TypeError, "BatchFused" + USER),
    (lambda: BatchFused(FN, 5, user=_HostTensor()), TypeError, "BatchFused's user tensor must live on the GPU (the functor reads it on the device)"),
    (lambda: BatchFused(FN, 5, nblobs=33), ValueError, "BatchFused" + NBLOBS),
    (lambda: BatchFused(FN, 5, ndata=-1), ValueError, "BatchFused" + NDATA),
    (lambda: BatchFused(FN, 5, ndata=[3, -1]), ValueError, "BatchFused" + NDATA),
    (lambda: BatchFused(FN, 5, ndata=np.array([3, -1])), ValueError, "BatchFused" + NDATA.replace("-1", repr(np.int64(-1)))),
    (lambda: BatchFused(FN, 5, ndata=2.0), ValueError, "BatchFused" + NDATA.replace("-1", "2.0")),
    (lambda: BatchFused(FN, 5, nblobs=2, ndata=[3, 4]), ValueError,
     "BatchFused: a target that sums over data (ndata) carries no blobs; nblobs=2 is refused"),
    (lambda: PTFused(0, 5), TypeError, "PTFused needs an emx_pt_fused_fn: " + LAUNCHER),
    (lambda: PTFused(FN, 0), TypeError, "PTFused needs the ndim its launcher was compiled for, an integer >= 1; got 0"),
    (lambda: PTFused(FN, 5, user="x"), TypeError, "PTFused" + USER),
    (lambda: PTFused(FN, 5, user=_HostTensor()), TypeError, "PTFused's user tensor must live on the GPU (the functors read it on the device)"),
    (lambda: PTFused(FN, 5, ndata=-1), ValueError, "PTFused" + NDATA),
    (lambda: PTFused(FN, 5, ndata=(3, -1)), ValueError, "PTFused" + NDATA),
    (lambda: targets.BatchKernel(0), TypeError, "BatchKernel needs an emx_batch_log_prob_fn: " + LAUNCHER),
    (lambda: BatchFusedLibrary("p", "n", 5, data=True).target(), ValueError,
     "BatchFusedLibrary.target: the library was built with data=True; give ndata, the members' numbers of data"),
    (lambda: BatchFusedLibrary("p", "n", 5).target(ndata=3), ValueError,
     "BatchFusedLibrary.target: ndata is for a library built with compile_fused(..., data=True)"),
    (lambda: DeviceFusedLibrary("p", "n", 5, data=True).target(), ValueError,
     "DeviceFusedLibrary.target: the library was built with data=True; give ndata, the number of data"),
    (lambda: DeviceFusedLibrary("p", "n", 5).target(ndata=3), ValueError,
     "DeviceFusedLibrary.target: ndata is for a library built with compile_fused_ensemble(..., data=True)"),
    (lambda: DeviceFusedLibrary("p", "n", 5, nblobs=33), ValueError, "DeviceFusedLibrary" + NBLOBS),
    (lambda: PTFusedLibrary("p", "n", 5, False, data=True).target(), ValueError,
     "PTFusedLibrary.target: the library was built with data=True; give ndata, the objects' numbers of data"),
    (lambda: PTFusedLibrary("p", "n", 5, False).target(ndata=3), ValueError,
     "PTFusedLibrary.target: ndata is for a library built with compile_fused_pt(..., data=True)"),
    (lambda: compile_fused(SRC, "F", 257), ValueError, "compile_fused: 1 <= ndim <= 256; got 257"),
    (lambda: compile_fused(SRC, "F", 5, nblobs=33), ValueError, "compile_fused" + NBLOBS),
    (lambda: compile_fused(SRC, "F", 5, nblobs=2, data=True), ValueError,
     "compile_fused: a data target (data=True) carries no blobs; nblobs=2 is refused"),
    (lambda: compile_fused(SRC, "F()", 5), ValueError, "compile_fused: functor must be a C++ identifier; got 'F()'"),
    (lambda: compile_fused(SRC, "F", 5, name="9x"), ValueError, "compile_fused: name must be a C++ identifier; got '9x'"),
    (lambda: compile_fused_ensemble(SRC, "F", 0), ValueError, "compile_fused_ensemble: 1 <= ndim <= 256; got 0"),
    (lambda: compile_fused_ensemble(SRC, "F", 5, nblobs=33), ValueError, "compile_fused_ensemble" + NBLOBS),
    (lambda: compile_fused_ensemble(SRC, "F", 5, nblobs=2, data=True), ValueError,
     "compile_fused_ensemble: a data target (data=True) carries no blobs; nblobs=2 is refused"),
    (lambda: compile_fused_ensemble(SRC, None, 5), ValueError, "compile_fused_ensemble: functor must be a C++ identifier; got None"),
    (lambda: compile_fused_ensemble(SRC, "F", 5, name="a b"), ValueError, "compile_fused_ensemble: name must be a C++ identifier; got 'a b'"),
    (lambda: compile_fused_pt(SRC, "F", 257), ValueError, "compile_fused_pt: 1 <= ndim <= 256; got 257"),
    (lambda: compile_fused_pt(SRC, 7, 5), ValueError, "compile_fused_pt: likelihood must be a C++ identifier; got 7"),
    (lambda: compile_fused_pt(SRC, "F", 5, prior="P<1>"), ValueError, "compile_fused_pt: prior must be a C++ identifier; got 'P<1>'"),
    (lambda: compile_fused_pt(SRC, "F", 5, name="-"), ValueError, "compile_fused_pt: name must be a C++ identifier; got '-'"),
]


@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_every_refusal_keeps_its_class_and_text(recorded, i):
    call, exc, text = REFUSALS[i]
    with pytest.raises(exc) as e:
        call()
    assert type(e.value) is exc and str(e.value) == text
    assert not recorded                   # refused before anything would be compiled


def test_what_the_checks_accept_is_kept(recorded):
    t = DeviceFused(ctypes.c_void_p(FN), np.int64(5), user=ctypes.c_void_p(96), ndata=np.int32(7))
    assert (t.ndim, t.ndata, t.user_address()) == (5, 7, 96) and type(t.ndata) is int
    assert BatchFused(FN, 5).user_address() is None and BatchFused(FN, 5, user=np.int64(32)).user_address() == 32
    assert BatchFused(FN, 5, ndata=np.array([3, 4])).ndata == (3, 4) and BatchFused(FN, 5, ndata=np.int64(3)).ndata == 3
    assert PTFused(FN, 5, ndata=[1, 2], has_prior=1).has_prior is True and PTFused(FN, 5, ndata=range(2)).ndata == (0, 1)
    assert PTFused(FN, 5).user_address() is None and PTFused(FN, 5, user=8).user_address() == 8
    lib = DeviceFusedLibrary("p", "n", 5, 2, "n_small")
    t = lib.target(user=16)
    assert (t.fn_ptr, t.small_fn, t.nblobs, t.ndata, t._library) == (0x1001, 0x1007, 2, None, lib)
