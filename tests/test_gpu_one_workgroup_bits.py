"""The one-workgroup kernels (k_small_run, k_pt_run, k_batch_cb) against recorded bits: tools/one_workgroup_bits.py drives the public
API through every form of the three kernels -- EnsembleSampler's small path (element-wise, dense, exact MT19937 plans),
EnsembleBatch (built-in, dense, fused, fused with blobs, fused over ragged data, batched callback) and PTSampler (fused and fused
over data, swaps every 2 steps, the adaptive ladder, one object too large to stage a whole split) -- with each move alone, a
weighted mixture, uneven thirds, a two-doubles-a-lane two-chunk row layout and more steps than a plan batch, and hashes what every
run leaves behind.  tests/golden/one_workgroup_bits.json is that tool's output on an MI355X at the parent of the commit that added
this test, before any of the kernels' repeated text was shared: whatever is done to their text, these runs keep their bits.

The cases must also stay on the paths they were chosen for (a change of the eligibility rules could move one onto the general path
with the same bits, and the guard would cover nothing): test_the_runs_took_the_one_workgroup_paths holds what the samplers report.
Two properties are NOT reported by any sampler and rest on the host rules as read: that 72 steps exceed the plan batch of the
single sampler's small path (emx_small_host.hpp: small_batch(32) = 32; the batched and tempered paths report theirs, and it is
asserted), and that pt_fused/chunked stages fewer rows than its split has (emx_batch.hip: pt_stage_rows)."""
import importlib.util
import json
import os

import pytest

pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "one_workgroup_bits.json")) as f:
    GOLDEN = json.load(f)


@pytest.fixture(scope="module")
def computed():
    """(digests, paths); the 16 user libraries are compiled on the first run only (cached under build/ by source and headers)"""
    spec = importlib.util.spec_from_file_location("one_workgroup_bits", os.path.join(ROOT, "tools", "one_workgroup_bits.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    paths = {}
    return tool.run_all(tool.compile_all(os.path.join(ROOT, "build", "one_workgroup_bits")), paths), paths


def test_the_cases_are_the_recorded_ones(computed):
    assert sorted(computed[0]) == sorted(GOLDEN) and len(GOLDEN) == 75


@pytest.mark.parametrize("case", sorted(GOLDEN))
def test_a_run_leaves_the_recorded_bits(computed, case):
    got = computed[0][case]
    assert got == GOLDEN[case], sorted(k for k in GOLDEN[case] if got.get(k) != GOLDEN[case][k])


def test_the_runs_took_the_one_workgroup_paths(computed):
    paths = computed[1]
    assert sorted(paths) == sorted(GOLDEN)
    for case, p in sorted(paths.items()):
        kind = case.split("/")[0]
        if kind.startswith("ensemble"):
            # every proposal step of the run was made by k_small_run, in one launch
            assert p["steps"] == p["nsteps"] and p["launches"] == 1, (case, p)
        elif kind == "batch_callback":
            assert p["plan_steps"] == 0 and p["launches"] > p["nsteps"], (case, p)         # k_batch_cb: launches a phase, no plan batch
        elif kind.startswith("batch"):
            assert p["launches"] == 2 and p["plan_steps"] >= 1, (case, p)                  # the initial log-probs, then ONE launch
        else:
            # k_pt_run: the initial state, then ONE launch (the callback path takes several a step).  pt_fused/chunked fits one
            # workgroup's LDS only with fewer staging rows than its split has (emx_batch.hip: pt_stage_rows), so that launch ran
            # the half-steps in chunks
            assert p["launches"] == 2 and p["plan_steps"] >= 1, (case, p)
        if p["nsteps"] == 72 and kind != "batch_callback" and not kind.startswith("ensemble"):
            assert 1 <= p["plan_steps"] < 72, (case, p)                                    # more steps than a plan batch holds
