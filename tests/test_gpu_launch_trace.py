"""The kernels a verification enqueues, in order, against tests/golden/launch_traces.json, -m gpu.

verify_pipeline (charon_amd/csrc/hipbls.hip) decides which kernels run, in which order, from the
call's shape and the knobs (vplan.h); the verdict tests see that choice only through its
consequences.  The fixture holds the launch sequence (hbls_timing / hbls_timing_read) of every path
-- small calls, the per-batch check, the slot-wide check with both combinations, several chunks of
groups, the adaptive skip, the first-error mode, hbls_slot_device's variants, the host path --
recorded by tests/golden/make_launch_traces.py with the library of the commit before the pipeline
was split into a plan and phases (the first-error and per-device-shard host traces: of the commit
before the host paths' grouping moved into hgroup.h; both recorded in two separate processes, which
agreed); a change that is not meant to alter the sequence must reproduce it exactly, name by name.
The cases and their inputs are the generator's own (CASES).  The large call's traces of the same
file (traces_large) are checked by tests/test_gpu_robustness.py, on its fixture.  The slot select calls
and the duty adds have a fixture of their own: tests/golden/select_traces.json (tests/test_gpu_select_trace.py).
"""
import json
import os
import sys

import pytest

from charon_amd import _lib

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

import make_launch_traces as mk  # noqa: E402


@pytest.fixture(scope="module")
def cx(hipbls):
    return mk.Ctx(_lib.load_library())


@pytest.fixture(scope="module")
def golden():
    with open(mk.PATH) as f:
        return json.load(f)["traces"]


def test_every_recorded_trace_has_a_case(golden):
    """The fixture and the cases name the same traces (no case dropped, none unrecorded)."""
    want = set(mk.CASES) - {"adaptive", "host"} | {"adaptive_1_failed", "adaptive_2_skipped", "adaptive_3_skipped_clean",
                                                  "host_no_key_cache", "host_key_cache", "host_first_error",
                                                  "host_split2"}
    assert set(golden) == want


@pytest.mark.parametrize("case", list(mk.CASES))
def test_launch_sequence(cx, golden, case):
    got = mk.CASES[case](cx)
    assert got, case
    for name, names in got.items():
        assert names == golden[name], (name, _first_difference(names, golden[name]))


def _first_difference(got, want):
    for k, (a, b) in enumerate(zip(got, want)):
        if a != b:
            return f"launch {k}: {a} (recorded: {b})"
    return f"{len(got)} launches (recorded: {len(want)})"


def test_paths_differ(golden):
    """The cases do take different paths: the marks of each strategy are where they belong."""
    assert "k_msm_bucket" in golden["slot_wide_per_item"] and "k_msm_bucket" not in golden["per_batch"]
    assert "k_plan" in golden["slot_wide_chunked"] and "k_plan" not in golden["slot_wide_per_item"]
    assert "k_msm_bucket" not in golden["slot_wide_two_chunks"]  # more groups than one chunk: no slot-wide check
    assert "k_batch_verdict" not in golden["small_groups"] and "k_pair3" in golden["small_groups"]
    assert golden["per_batch_two_chunks"].count("k_batch_verdict") == 2
    assert "k_msm_bucket" in golden["adaptive_1_failed"]
    assert "k_msm_bucket" not in golden["adaptive_2_skipped"] and "k_msm_bucket" not in golden["adaptive_3_skipped_clean"]
    assert "k_first_group" in golden["first_error_batched"] and "k_first_group" not in golden["first_error_small"]
    assert "k_first_item" in golden["first_error_small"]
    assert "k_lines_at_p" in golden["slot_deferred_slot_wide"] and "k_lines_at_p" not in golden["slot_deferred_per_batch"]
    assert "k_pk_lookup" not in golden["slot_tables"] and "k_pk_lookup" in golden["slot_dv_src"]
    assert "k_first_item" in golden["host_first_error"] and "k_first_item" not in golden["host_no_key_cache"]
    # two contexts, each a small call of 65 groups with its own hashing and signature-cache put
    assert golden["host_split2"].count("k_hash_to_g2") == 2 and golden["host_split2"].count("k_sc_put") == 2
    assert "k_batch_verdict" not in golden["host_split2"] and "k_batch_verdict" in golden["host_no_key_cache"]
