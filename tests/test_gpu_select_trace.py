"""The kernels the slot select calls and the duty adds enqueue, in order, against
tests/golden/select_traces.json, -m gpu.

tests/test_gpu_launch_trace.py pins verify_pipeline, hbls_slot_device and the host Verify paths; this
file does the same for hbls_slot_select_device, hbls_slot_select_batch, hbls_duty_add,
hbls_duty_add_sets and hbls_duty_add_sets_first (charon_amd/csrc/hipbls.hip), which share one
selection-and-aggregation tail and whose duty adds run as a sequence of named steps.  The fixture was
recorded by tests/golden/make_select_traces.py with the library of the commit before the two copies
of that tail became one; a change that is not meant to alter the sequence must reproduce it.  The
cases and their inputs are the generator's own (CASES).

How a case is compared: a call on one shard, and a two-phase set add on two (its contexts are taken
on the calling thread, in ascending order, before any shard thread starts), name by name.  SORTED
names the other two-shard cases, the plain one-segment path, where each shard thread takes its
context itself and the threads race: each shard's own sequence is fixed, but the fixture holds one
run, so what it shows of the two shards' records beside each other is not known to hold for another;
such a case is compared as the sorted list of names (the same kernels, each as often).
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

import make_select_traces as ms  # noqa: E402

mk = ms.mk
SORTED = {"select_host_split2"}


@pytest.fixture(scope="module")
def cx(hipbls):
    return mk.Ctx(_lib.load_library())


@pytest.fixture(scope="module")
def golden():
    with open(ms.PATH) as f:
        return json.load(f)["traces"]


def test_every_recorded_trace_has_a_case(golden):
    """The fixture and the cases name the same traces (no case dropped, none unrecorded)."""
    assert set(golden) == {t for c in ms.CASES for t in ms.TRACES.get(c, [c])}
    assert SORTED <= set(golden)


@pytest.mark.parametrize("case", list(ms.CASES))
def test_launch_sequence(cx, golden, case):
    got = ms.CASES[case](cx)
    assert sorted(got) == sorted(ms.TRACES.get(case, [case]))
    for name, names in got.items():
        assert names, name
        if name in SORTED:
            assert sorted(names) == sorted(golden[name]), (name, _first_difference(sorted(names), sorted(golden[name])))
        else:
            assert names == golden[name], (name, _first_difference(names, golden[name]))


def _first_difference(got, want):
    for k, (a, b) in enumerate(zip(got, want)):
        if a != b:
            return f"launch {k}: {a} (recorded: {b})"
    return f"{len(got)} launches (recorded: {len(want)})"


def test_paths_differ(golden):
    """The cases do take different paths: the marks of each are where they belong."""
    select = [n for n in golden if n.startswith("select_")]
    duty = [n for n in golden if n.startswith("duty_")]
    sets = [n for n in duty if n.startswith("duty_add_sets")]
    assert len(select) == 9 and len(duty) == 11 and len(sets) == 8
    # what fills the candidates: k_ta_select in a slot, k_duty_gather in a duty (and only where a group fired)
    for n in select:
        assert "k_ta_select" in golden[n] and "k_duty_gather" not in golden[n], n
    for n in duty:
        assert "k_ta_select" not in golden[n], n
        fires = not n.endswith("_rejected") and n != "duty_add_no_fire"
        for k in ("k_duty_gather", "k_ta_sel_scan", "k_ta_sel_fill", "k_ta_sel_scatter", "k_ta_sel_verdicts"):
            assert golden[n].count(k) == ((2 if n.endswith("_split2_clean") else 1) if fires else 0), (n, k)
        assert "k_duty_store" in golden[n] and "k_duty_copy" in golden[n], n
    # the gate belongs to the set adds; k_duty_set_first to hbls_duty_add_sets alone (the segmented
    # verification of hbls_duty_add_sets_first leaves the sets' first failures itself)
    for n in duty:
        assert ("k_duty_gate" in golden[n]) == (n in sets), n
        assert ("k_duty_set_first" in golden[n]) == (n in sets and "_first" not in n), n
    # two shards: everything twice
    for n in sets:
        assert golden[n].count("k_duty_gate") == (2 if "_split2" in n else 1), n
    assert golden["select_host_split2"].count("k_ta_select") == 2 and golden["select_host"].count("k_ta_select") == 1
    # threshold 1: neither the small-scalar nor the joint aggregation
    assert "k_ta_small" not in golden["duty_t1"] and "k_ta_small" in golden["duty_add_fires"]
    # no partials: the early return
    assert golden["select_device_no_partials"] == ["k_ta_select", "k_ta_sel_scatter", "k_ta_sel_verdicts"]
    # the messages' lines.  Shared messages, or fewer groups than the batched sizes (a shard of 65):
    # phase 1 computes them with the hashing.  One message per validator at the batched sizes: both
    # verifications defer them into their own checks (the slot-wide one at its point, the per-batch
    # one per chain) -- unless the aggregates are too few for that: then phase 4 computes them first
    def after(n, k):
        return golden[n][golden[n].index(k) + 1]
    for n in select:
        if n == "select_device_no_partials":
            continue
        deferred = "_distinct_" in n or n == "select_host"
        assert golden[n][0] == "k_hash_to_g2" and (golden[n][1] == "k_lines_msg") == (not deferred), n
        assert (after(n, "k_ta_sel_scatter") == "k_lines_msg") == (n == "select_device_distinct_lines_msg"), n
        if not deferred:
            assert golden[n].count("k_lines_msg") == (2 if n == "select_host_split2" else 1), n
    for n in ("select_device_distinct_per_batch", "select_device_distinct_lines_msg", "select_host"):
        assert golden[n].count("k_lines_msg") == 2 and after(n, "k_rlc") == "k_lines_msg", n
    assert "k_lines_at_p" in golden["select_device_distinct_slot_wide"] and "k_lines_at_p" not in golden["select_device_distinct_per_batch"]
    assert "k_msm_bucket" in golden["select_device_shared_slot_wide"] and "k_msm_bucket" not in golden["select_device_shared_per_batch"]
    assert "k_pk_lookup" not in golden["select_device_tables"] and "k_pk_lookup" in golden["select_device_shared_slot_wide"]
