"""The answers of the three half-step launchers of a fused user target to descriptors they refuse, or accept without launching
(emx_fused_ensemble.hpp: fused_ens_launch_checks; the header's list of answers).  tests/c/fused_launch_answers.hip is a stand-alone
host program that hands each launcher one descriptor per check, and the pairs of simultaneous faults whose answers differ -- the
order of the checks is part of the contract: a launcher built against other headers, for another ndim AND another move must say
"other headers".  No descriptor reaches a launch, no HIP call is made, no device is needed."""
import os
import shutil
import subprocess

import pytest

from emcee_amd.targets import FUSED_FLAGS, get_include

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "fused_launch_answers.hip")

# (launcher, case, answer): 0 nothing to do, 1 other headers or another launcher type's descriptor, 2 another ndim, 3 a move or
# launch shape that was not compiled in, 4 another number of blobs or no blob array, 5 a launch that carries an exchange.
# The table the program printed when it was built against the headers as they were before the launchers' checks became one function.
ANSWERS = [
    ("plain", "null_descriptor", 1),
    ("plain", "other_abi", 1),
    ("plain", "other_args_bytes", 1),
    ("plain", "other_ndim", 2),
    ("plain", "move_5", 3),
    ("plain", "move_minus_1", 3),
    ("plain", "probe", 0),
    ("plain", "null_args", 3),
    ("plain", "negative_grid", 3),
    ("plain", "threads_128", 3),
    ("plain", "lds_one_byte_short", 3),
    ("plain", "args_other_ndim", 2),
    ("plain", "args_sendbuf", 5),
    ("plain", "args_desc", 5),
    ("plain", "args_t_hi_dev", 5),
    ("plain", "args_peers", 5),
    ("plain", "args_npeer", 5),
    ("plain", "args_declp", 5),
    ("plain", "args_push_peers", 5),
    ("plain", "args_npush", 5),
    ("plain", "empty_split", 0),
    ("plain", "reversed_split", 0),
    ("plain", "other_abi+other_ndim", 1),
    ("plain", "other_ndim+move_5", 2),
    ("plain", "move_5+probe", 3),
    ("plain", "probe+threads_128", 0),
    ("plain", "probe+null_args", 0),
    ("plain", "threads_128+args_other_ndim", 3),
    ("plain", "threads_128+args_npeer", 3),
    ("plain", "args_other_ndim+args_npeer", 2),
    ("plain", "args_npeer+reversed_split", 5),
    ("blobs", "null_descriptor", 1),
    ("blobs", "other_abi", 1),
    ("blobs", "other_args_bytes", 1),
    ("blobs", "other_ndim", 2),
    ("blobs", "move_5", 3),
    ("blobs", "move_minus_1", 3),
    ("blobs", "probe", 0),
    ("blobs", "null_args", 3),
    ("blobs", "negative_grid", 3),
    ("blobs", "threads_128", 3),
    ("blobs", "lds_one_byte_short", 3),
    ("blobs", "args_other_ndim", 2),
    ("blobs", "args_sendbuf", 5),
    ("blobs", "args_desc", 5),
    ("blobs", "args_t_hi_dev", 5),
    ("blobs", "args_peers", 5),
    ("blobs", "args_npeer", 5),
    ("blobs", "args_declp", 5),
    ("blobs", "args_push_peers", 5),
    ("blobs", "args_npush", 5),
    ("blobs", "empty_split", 0),
    ("blobs", "reversed_split", 0),
    ("blobs", "other_abi+other_ndim", 1),
    ("blobs", "other_ndim+move_5", 2),
    ("blobs", "move_5+probe", 3),
    ("blobs", "probe+threads_128", 0),
    ("blobs", "probe+null_args", 0),
    ("blobs", "threads_128+args_other_ndim", 3),
    ("blobs", "threads_128+args_npeer", 3),
    ("blobs", "args_other_ndim+args_npeer", 2),
    ("blobs", "args_npeer+reversed_split", 5),
    ("data", "null_descriptor", 1),
    ("data", "other_abi", 1),
    ("data", "other_args_bytes", 1),
    ("data", "other_ndim", 2),
    ("data", "move_5", 3),
    ("data", "move_minus_1", 3),
    ("data", "probe", 0),
    ("data", "null_args", 3),
    ("data", "negative_grid", 3),
    ("data", "threads_128", 3),
    ("data", "lds_one_byte_short", 3),
    ("data", "args_other_ndim", 2),
    ("data", "args_sendbuf", 5),
    ("data", "args_desc", 5),
    ("data", "args_t_hi_dev", 5),
    ("data", "args_peers", 5),
    ("data", "args_npeer", 5),
    ("data", "args_declp", 5),
    ("data", "args_push_peers", 5),
    ("data", "args_npush", 5),
    ("data", "empty_split", 0),
    ("data", "reversed_split", 0),
    ("data", "other_abi+other_ndim", 1),
    ("data", "other_ndim+move_5", 2),
    ("data", "move_5+probe", 3),
    ("data", "probe+threads_128", 0),
    ("data", "probe+null_args", 0),
    ("data", "threads_128+args_other_ndim", 3),
    ("data", "threads_128+args_npeer", 3),
    ("data", "args_other_ndim+args_npeer", 2),
    ("data", "args_npeer+reversed_split", 5),
    ("blobs", "nblobs_3", 4),
    ("blobs", "null_blobs_cur", 4),
    ("blobs", "move_5+nblobs_3", 3),
    ("blobs", "nblobs_3+probe", 4),
    ("blobs", "nblobs_3+threads_128", 4),
    ("blobs", "probe+null_blobs_cur", 0),
    ("blobs", "threads_128+null_blobs_cur", 3),
    ("blobs", "null_args+null_blobs_cur", 3),
    ("blobs", "null_blobs_cur+args_other_ndim", 4),
    ("blobs", "null_blobs_cur+args_npeer", 4),
    ("data", "rows_3", 3),
    ("data", "rows_4", 0),
    ("data", "rows_tile", 0),
    ("data", "rows_tile+lds_of_8_rows", 3),
    ("data", "rows_tile_plus_1", 3),
    ("data", "ndata_minus_1", 3),
    ("data", "ndata_0", 0),
    ("data", "ndata_2^31", 3),
    ("data", "probe+rows_3", 0),
    ("data", "rows_3+null_args", 3),
    ("data", "rows_3+args_other_ndim", 3),
    ("data", "rows_3+args_npeer", 3),
    ("data", "ndata_2^31+args_other_ndim", 3),
]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("fused_launch_answers") / "fused_launch_answers")
    flags = [f for f in FUSED_FLAGS if f not in ("-shared", "-fPIC")]
    r = subprocess.run([hipcc] + flags + ["-I" + d for d in get_include()] + [SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stderr or r.stdout)[-4000:]
    return exe


def test_every_launcher_answers_every_refusal_as_it_always_did(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [tuple(line.split()) for line in r.stdout.splitlines()]
    assert all(len(g) == 3 for g in got), r.stdout[-2000:]
    got = [(who, case, int(answer)) for who, case, answer in got]
    assert [g[:2] for g in got] == [a[:2] for a in ANSWERS]          # the cases, in the program's order
    wrong = [(g, a[2]) for g, a in zip(got, ANSWERS) if g != a]
    assert not wrong, "(launcher, case, answer) and the answer expected: %r" % wrong


def test_the_table_covers_every_answer_and_every_launcher():
    assert {a[0] for a in ANSWERS} == {"plain", "blobs", "data"}
    for who, answers in (("plain", {0, 1, 2, 3, 5}), ("blobs", {0, 1, 2, 3, 4, 5}), ("data", {0, 1, 2, 3, 5})):
        assert {a[2] for a in ANSWERS if a[0] == who} == answers
    assert len({a[:2] for a in ANSWERS}) == len(ANSWERS)
