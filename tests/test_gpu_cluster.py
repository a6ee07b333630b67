"""Cluster handles through the ABI (hbls_cluster_open / _close / _stats, hbls_duty_open_cluster and the
three add entry points on a cluster duty), -m gpu: duties that take their keys from the lock.

The cases are tests/gpu_helpers/cluster_cases.py (on the clusters and clean streams of
tests/test_gpu_duty.py, every call against a twin plain duty under the defining property of
include/hipbls.h; tests/gpu_helpers/cluster.py is the plumbing).  They run ONCE, in a child pytest process
with the default four hardware queues, and each test here asserts on its case's outcome; none is
deselected or skipped.

Why a child: tests/test_gpu_duty_first.py's reason.  The runtime reserves scratch per hardware queue for
the largest kernel the queue has run, and a run of the whole tests/ directory is at the device's scratch
with nothing to spare.  hbls_cluster_open runs k_cluster_wide (3 096 B per lane, k_pk_wide's arithmetic)
on the library stream of every context it shards over, streams the suite's other tests leave to smaller
kernels, and these cases drive duties of 1 792 partials in one call on one and two contexts.  In a
process of their own, which ends with them, the cases reserve nothing in the suite's process.
"""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join("tests", "gpu_helpers", "cluster_cases.py")
IDS = ['test_clean_streams_equal_the_twin_and_the_construction[add]',
       'test_clean_streams_equal_the_twin_and_the_construction[sets]',
       'test_clean_streams_equal_the_twin_and_the_construction[first]',
       'test_planted_errors[add]',
       'test_planted_errors[sets]',
       'test_planted_errors[first]',
       'test_call_errors_write_nothing',
       'test_a_duty_outlives_its_closed_cluster',
       'test_the_learned_key_cache_is_left_alone',
       'test_two_contexts[2]',
       'test_a_cluster_keeps_the_shard_layout_it_was_opened_under',
       'test_a_real_lock',
       'test_parsig_duty_on_a_cluster']


@pytest.fixture(scope="module")
def outcome(hipbls):
    """case id -> PASSED / FAILED / ..., and the child's whole output"""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")  # the count a process has by default, whatever this one was started with
    r = subprocess.run([sys.executable, "-m", "pytest", CASES, "-v", "-x", "-p", "no:cacheprovider"], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    text = r.stdout + r.stderr
    return dict(re.findall(r"cluster_cases\.py::(\S+) (PASSED|FAILED|ERROR|SKIPPED|XFAIL|XPASS)", text)), text


@pytest.mark.parametrize("case", IDS)
def test_case(outcome, case):
    got, text = outcome
    assert got.get(case) == "PASSED", f"{case}: {got.get(case, 'not run')}\n" + text[-6000:]


def test_every_case_of_the_file_is_listed(outcome):
    assert sorted(outcome[0]) == sorted(IDS), "tests/gpu_helpers/cluster_cases.py and IDS name the same cases"
