"""The answers of the launchers of a fused batch target (plain, with blobs, with data, with the stretch selector alone) and of a
fused tempered target (without a prior, with one, with data) to descriptors they refuse, or accept without launching
(emx_fused_target.hpp: fused_launch_checks, and the checks each launcher keeps at its call site).
tests/c/fused_batch_launch_answers.hip is a stand-alone host program that hands each launcher one descriptor per check of its
ladder, and the pairs of simultaneous faults whose answers depend on the order -- the order of the checks is part of the
contract.  Every descriptor with a non-zero grid carries a fault its launcher refuses, so none reaches a launch; the program runs
as a child with every device hidden, and exits before its first call where one is visible all the same."""
import os
import shutil
import subprocess

import pytest

from emcee_amd.targets import FUSED_FLAGS, get_include

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "fused_batch_launch_answers.hip")

# (launcher, case, answer, has_prior): 0 the probe, 1 other headers or the sibling form's descriptor, 2 another ndim, 3 a move
# selector or launch shape that is not served (or no counts), 4 another number of blobs or no blob array.  has_prior: the field
# as a tempered launcher left it (-1: not written; None: a batch launcher, whose descriptor has none).
# The table the program printed when it was built against the headers as they were before the four launchers' checks became
# one function.
ANSWERS = [
    ("plain", "null_descriptor", 1, None),
    ("plain", "other_abi", 1, None),
    ("plain", "sibling_abi", 1, None),
    ("plain", "other_args_bytes", 1, None),
    ("plain", "other_ndim", 2, None),
    ("plain", "movesel_5", 3, None),
    ("plain", "movesel_minus_1", 3, None),
    ("plain", "probe", 0, None),
    ("plain", "any_selector+probe", 0, None),
    ("plain", "null_args", 3, None),
    ("plain", "negative_grid", 3, None),
    ("plain", "threads_0", 3, None),
    ("plain", "threads_32", 3, None),
    ("plain", "threads_96", 3, None),
    ("plain", "threads_over", 3, None),
    ("plain", "args_other_ndim", 2, None),
    ("plain", "other_abi+other_ndim", 1, None),
    ("plain", "other_args_bytes+other_ndim", 1, None),
    ("plain", "other_ndim+movesel_5", 2, None),
    ("plain", "movesel_5+probe", 3, None),
    ("plain", "probe+threads_96", 0, None),
    ("plain", "probe+null_args", 0, None),
    ("plain", "probe+args_other_ndim", 0, None),
    ("plain", "threads_96+args_other_ndim", 3, None),
    ("plain", "negative_grid+args_other_ndim", 3, None),
    ("plain", "nblobs_other", 4, None),
    ("plain", "nblobs_other+null_args", 3, None),
    ("plain", "nblobs_other+null_args+probe", 0, None),
    ("plain", "movesel_5+nblobs_other", 3, None),
    ("plain", "nblobs_other+probe", 4, None),
    ("plain", "nblobs_other+threads_96", 4, None),
    ("plain", "args_nblobs_other", 4, None),
    ("plain", "threads_96+args_nblobs_other", 3, None),
    ("plain", "args_other_ndim+args_nblobs_other", 2, None),
    ("blobs", "null_descriptor", 1, None),
    ("blobs", "other_abi", 1, None),
    ("blobs", "sibling_abi", 1, None),
    ("blobs", "other_args_bytes", 1, None),
    ("blobs", "other_ndim", 2, None),
    ("blobs", "movesel_5", 3, None),
    ("blobs", "movesel_minus_1", 3, None),
    ("blobs", "probe", 0, None),
    ("blobs", "any_selector+probe", 0, None),
    ("blobs", "null_args", 3, None),
    ("blobs", "negative_grid", 3, None),
    ("blobs", "threads_0", 3, None),
    ("blobs", "threads_32", 3, None),
    ("blobs", "threads_96", 3, None),
    ("blobs", "threads_over", 3, None),
    ("blobs", "args_other_ndim", 2, None),
    ("blobs", "other_abi+other_ndim", 1, None),
    ("blobs", "other_args_bytes+other_ndim", 1, None),
    ("blobs", "other_ndim+movesel_5", 2, None),
    ("blobs", "movesel_5+probe", 3, None),
    ("blobs", "probe+threads_96", 0, None),
    ("blobs", "probe+null_args", 0, None),
    ("blobs", "probe+args_other_ndim", 0, None),
    ("blobs", "threads_96+args_other_ndim", 3, None),
    ("blobs", "negative_grid+args_other_ndim", 3, None),
    ("blobs", "nblobs_other", 4, None),
    ("blobs", "nblobs_other+null_args", 4, None),
    ("blobs", "nblobs_other+null_args+probe", 4, None),
    ("blobs", "movesel_5+nblobs_other", 3, None),
    ("blobs", "nblobs_other+probe", 4, None),
    ("blobs", "nblobs_other+threads_96", 4, None),
    ("blobs", "args_nblobs_other", 4, None),
    ("blobs", "threads_96+args_nblobs_other", 3, None),
    ("blobs", "args_other_ndim+args_nblobs_other", 2, None),
    ("blobs", "args_null_blobs", 4, None),
    ("blobs", "probe+args_null_blobs", 0, None),
    ("blobs", "threads_96+args_null_blobs", 3, None),
    ("blobs", "args_other_ndim+args_null_blobs", 2, None),
    ("data", "null_descriptor", 1, None),
    ("data", "other_abi", 1, None),
    ("data", "sibling_abi", 1, None),
    ("data", "other_args_bytes", 1, None),
    ("data", "other_ndim", 2, None),
    ("data", "movesel_5", 3, None),
    ("data", "movesel_minus_1", 3, None),
    ("data", "probe", 0, None),
    ("data", "any_selector+probe", 0, None),
    ("data", "null_args", 3, None),
    ("data", "negative_grid", 3, None),
    ("data", "threads_0", 3, None),
    ("data", "threads_32", 3, None),
    ("data", "threads_96", 3, None),
    ("data", "threads_over", 3, None),
    ("data", "args_other_ndim", 2, None),
    ("data", "other_abi+other_ndim", 1, None),
    ("data", "other_args_bytes+other_ndim", 1, None),
    ("data", "other_ndim+movesel_5", 2, None),
    ("data", "movesel_5+probe", 3, None),
    ("data", "probe+threads_96", 0, None),
    ("data", "probe+null_args", 0, None),
    ("data", "probe+args_other_ndim", 0, None),
    ("data", "threads_96+args_other_ndim", 3, None),
    ("data", "negative_grid+args_other_ndim", 3, None),
    ("data", "nblobs_other", 4, None),
    ("data", "nblobs_other+null_args", 4, None),
    ("data", "nblobs_other+null_args+probe", 4, None),
    ("data", "movesel_5+nblobs_other", 3, None),
    ("data", "nblobs_other+probe", 4, None),
    ("data", "nblobs_other+threads_96", 4, None),
    ("data", "args_nblobs_other", 4, None),
    ("data", "threads_96+args_nblobs_other", 3, None),
    ("data", "args_other_ndim+args_nblobs_other", 2, None),
    ("data", "null_ndata", 3, None),
    ("data", "probe+null_ndata", 0, None),
    ("data", "nblobs_other+null_ndata", 4, None),
    ("data", "null_ndata+args_other_ndim", 3, None),
    ("data", "null_ndata+args_nblobs_other", 3, None),
    ("stretch_only", "null_descriptor", 1, None),
    ("stretch_only", "other_abi", 1, None),
    ("stretch_only", "sibling_abi", 1, None),
    ("stretch_only", "other_args_bytes", 1, None),
    ("stretch_only", "other_ndim", 2, None),
    ("stretch_only", "movesel_5", 3, None),
    ("stretch_only", "movesel_minus_1", 3, None),
    ("stretch_only", "probe", 0, None),
    ("stretch_only", "any_selector+probe", 3, None),
    ("stretch_only", "null_args", 3, None),
    ("stretch_only", "negative_grid", 3, None),
    ("stretch_only", "threads_0", 3, None),
    ("stretch_only", "threads_32", 3, None),
    ("stretch_only", "threads_96", 3, None),
    ("stretch_only", "threads_over", 3, None),
    ("stretch_only", "args_other_ndim", 2, None),
    ("stretch_only", "other_abi+other_ndim", 1, None),
    ("stretch_only", "other_args_bytes+other_ndim", 1, None),
    ("stretch_only", "other_ndim+movesel_5", 2, None),
    ("stretch_only", "movesel_5+probe", 3, None),
    ("stretch_only", "probe+threads_96", 0, None),
    ("stretch_only", "probe+null_args", 0, None),
    ("stretch_only", "probe+args_other_ndim", 0, None),
    ("stretch_only", "threads_96+args_other_ndim", 3, None),
    ("stretch_only", "negative_grid+args_other_ndim", 3, None),
    ("stretch_only", "nblobs_other", 4, None),
    ("stretch_only", "nblobs_other+null_args", 3, None),
    ("stretch_only", "nblobs_other+null_args+probe", 0, None),
    ("stretch_only", "movesel_5+nblobs_other", 3, None),
    ("stretch_only", "nblobs_other+probe", 4, None),
    ("stretch_only", "nblobs_other+threads_96", 4, None),
    ("stretch_only", "args_nblobs_other", 4, None),
    ("stretch_only", "threads_96+args_nblobs_other", 3, None),
    ("stretch_only", "args_other_ndim+args_nblobs_other", 2, None),
    ("stretch_only", "any_selector", 3, None),
    ("stretch_only", "other_ndim+any_selector", 2, None),
    ("stretch_only", "any_selector+nblobs_other", 3, None),
    ("stretch_only", "any_selector+args_other_ndim", 3, None),
    ("pt", "null_descriptor", 1, -1),
    ("pt", "other_abi", 1, -1),
    ("pt", "sibling_abi", 1, -1),
    ("pt", "other_args_bytes", 1, -1),
    ("pt", "other_ndim", 2, -1),
    ("pt", "movesel_5", 3, -1),
    ("pt", "movesel_minus_1", 3, -1),
    ("pt", "probe", 0, 0),
    ("pt", "any_selector+probe", 0, 0),
    ("pt", "null_args", 3, 0),
    ("pt", "negative_grid", 3, 0),
    ("pt", "threads_0", 3, 0),
    ("pt", "threads_32", 3, 0),
    ("pt", "threads_96", 3, 0),
    ("pt", "threads_over", 3, 0),
    ("pt", "args_other_ndim", 2, 0),
    ("pt", "other_abi+other_ndim", 1, -1),
    ("pt", "other_args_bytes+other_ndim", 1, -1),
    ("pt", "other_ndim+movesel_5", 2, -1),
    ("pt", "movesel_5+probe", 3, -1),
    ("pt", "probe+threads_96", 0, 0),
    ("pt", "probe+null_args", 0, 0),
    ("pt", "probe+args_other_ndim", 0, 0),
    ("pt", "threads_96+args_other_ndim", 3, 0),
    ("pt", "negative_grid+args_other_ndim", 3, 0),
    ("pt", "threads_1088", 3, 0),
    ("pt_prior", "null_descriptor", 1, -1),
    ("pt_prior", "other_abi", 1, -1),
    ("pt_prior", "sibling_abi", 1, -1),
    ("pt_prior", "other_args_bytes", 1, -1),
    ("pt_prior", "other_ndim", 2, -1),
    ("pt_prior", "movesel_5", 3, -1),
    ("pt_prior", "movesel_minus_1", 3, -1),
    ("pt_prior", "probe", 0, 1),
    ("pt_prior", "any_selector+probe", 0, 1),
    ("pt_prior", "null_args", 3, 1),
    ("pt_prior", "negative_grid", 3, 1),
    ("pt_prior", "threads_0", 3, 1),
    ("pt_prior", "threads_32", 3, 1),
    ("pt_prior", "threads_96", 3, 1),
    ("pt_prior", "threads_over", 3, 1),
    ("pt_prior", "args_other_ndim", 2, 1),
    ("pt_prior", "other_abi+other_ndim", 1, -1),
    ("pt_prior", "other_args_bytes+other_ndim", 1, -1),
    ("pt_prior", "other_ndim+movesel_5", 2, -1),
    ("pt_prior", "movesel_5+probe", 3, -1),
    ("pt_prior", "probe+threads_96", 0, 1),
    ("pt_prior", "probe+null_args", 0, 1),
    ("pt_prior", "probe+args_other_ndim", 0, 1),
    ("pt_prior", "threads_96+args_other_ndim", 3, 1),
    ("pt_prior", "negative_grid+args_other_ndim", 3, 1),
    ("pt_data", "null_descriptor", 1, -1),
    ("pt_data", "other_abi", 1, -1),
    ("pt_data", "sibling_abi", 1, -1),
    ("pt_data", "other_args_bytes", 1, -1),
    ("pt_data", "other_ndim", 2, -1),
    ("pt_data", "movesel_5", 3, -1),
    ("pt_data", "movesel_minus_1", 3, -1),
    ("pt_data", "probe", 0, 1),
    ("pt_data", "any_selector+probe", 0, 1),
    ("pt_data", "null_args", 3, 1),
    ("pt_data", "negative_grid", 3, 1),
    ("pt_data", "threads_0", 3, 1),
    ("pt_data", "threads_32", 3, 1),
    ("pt_data", "threads_96", 3, 1),
    ("pt_data", "threads_over", 3, 1),
    ("pt_data", "args_other_ndim", 2, 1),
    ("pt_data", "other_abi+other_ndim", 1, -1),
    ("pt_data", "other_args_bytes+other_ndim", 1, -1),
    ("pt_data", "other_ndim+movesel_5", 2, -1),
    ("pt_data", "movesel_5+probe", 3, -1),
    ("pt_data", "probe+threads_96", 0, 1),
    ("pt_data", "probe+null_args", 0, 1),
    ("pt_data", "probe+args_other_ndim", 0, 1),
    ("pt_data", "threads_96+args_other_ndim", 3, 1),
    ("pt_data", "negative_grid+args_other_ndim", 3, 1),
    ("pt_data", "args_null_ndata", 3, 1),
    ("pt_data", "probe+args_null_ndata", 0, 1),
    ("pt_data", "threads_96+args_null_ndata", 3, 1),
    ("pt_data", "args_other_ndim+args_null_ndata", 2, 1),
]
LAUNCHERS = {"plain", "blobs", "data", "stretch_only", "pt", "pt_prior", "pt_data"}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("fused_batch_launch_answers") / "fused_batch_launch_answers")
    flags = [f for f in FUSED_FLAGS if f not in ("-shared", "-fPIC")]
    r = subprocess.run([hipcc] + flags + ["-I" + d for d in get_include()] + [SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stderr or r.stdout)[-4000:]
    return exe


def test_every_launcher_answers_every_refusal_as_it_always_did(program):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    r = subprocess.run([program], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    got = []
    for line in r.stdout.splitlines():
        f = line.split()
        assert len(f) in (3, 4), line
        got.append((f[0], f[1], int(f[2]), int(f[3]) if len(f) == 4 else None))
    assert not [g for g in got if g[2] >= 100], "a descriptor reached a launch"
    assert [g[:2] for g in got] == [a[:2] for a in ANSWERS]          # the cases, in the program's order
    wrong = [(g, a[2:]) for g, a in zip(got, ANSWERS) if g != a]
    assert not wrong, "(launcher, case, answer, has_prior) and the (answer, has_prior) expected: %r" % wrong


def test_the_table_covers_every_answer_and_every_launcher():
    assert {a[0] for a in ANSWERS} == LAUNCHERS
    # a tempered descriptor has no blob count: its launchers never answer 4
    for who in LAUNCHERS:
        answers = {0, 1, 2, 3} if who.startswith("pt") else {0, 1, 2, 3, 4}
        assert {a[2] for a in ANSWERS if a[0] == who} == answers, who
    assert len({a[:2] for a in ANSWERS}) == len(ANSWERS)
    # the probe reports the prior; a descriptor refused ahead of the selectors is not written
    assert {a[3] for a in ANSWERS if a[0] == "pt" and a[2] == 0} == {0}
    assert {a[3] for a in ANSWERS if a[0] in ("pt_prior", "pt_data") and a[2] == 0} == {1}
    assert {a[3] for a in ANSWERS if a[0].startswith("pt") and a[2] == 1} == {-1}
    assert {a[3] for a in ANSWERS if not a[0].startswith("pt")} == {None}
