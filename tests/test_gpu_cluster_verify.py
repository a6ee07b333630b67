"""hbls_cluster_verify_batch, hbls_cluster_verify_aggregate and hbls_cluster_verify_stats through the ABI
and callers.Cluster, -m gpu: signatures checked under the lock's resident keys.

The cases are tests/gpu_helpers/cluster_verify_cases.py (the 6-validator lock of
tests/gpu_helpers/lock_check_cases.py and the four reference locks of tests/golden/kat_reference.json; the
reference is the two twins of include/hipbls.h, hbls_verify_batch and hbls_verify_aggregate_batch over the
lock's own 48-byte keys).  They run ONCE, in a child pytest process with the default four hardware queues,
and each test here asserts on its case's outcome; none is deselected or skipped.

Why a child: tests/test_gpu_lock_check.py's reason.  The cases open clusters under one, two and three
contexts, with ladder tables (k_cluster_wide, 3 096 B of scratch per lane on each context's library
stream), and run duties on them, and a run of the whole tests/ directory is at the device's per-queue
scratch reservations with nothing to spare.  In a process of their own, which ends with them, the cases
reserve nothing in the suite's process.  k_cluster_row_sum itself keeps 8 B of scratch per lane; its
kernel tests (tests/test_gpu_cluster_sum_kernels.py) run in the suite's process.
"""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join("tests", "gpu_helpers", "cluster_verify_cases.py")
IDS = ['test_reference_locks',
       'test_twin_of_verify_batch',
       'test_twin_of_verify_aggregate',
       'test_shards[2]',
       'test_shards[3]',
       'test_verifies_only_read',
       'test_call_errors_write_nothing',
       'test_launch_traces',
       'test_callers_cluster']


@pytest.fixture(scope="module")
def outcome(hipbls):
    """case id -> PASSED / FAILED / ..., and the child's whole output"""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")  # the count a process has by default, whatever this one was started with
    r = subprocess.run([sys.executable, "-m", "pytest", CASES, "-v", "-x", "-p", "no:cacheprovider"], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    text = r.stdout + r.stderr
    return dict(re.findall(r"cluster_verify_cases\.py::(\S+) (PASSED|FAILED|ERROR|SKIPPED|XFAIL|XPASS)", text)), text


@pytest.mark.parametrize("case", IDS)
def test_case(outcome, case):
    got, text = outcome
    assert got.get(case) == "PASSED", f"{case}: {got.get(case, 'not run')}\n" + text[-6000:]


def test_every_case_of_the_file_is_listed(outcome):
    assert sorted(outcome[0]) == sorted(IDS), "tests/gpu_helpers/cluster_verify_cases.py and IDS name the same cases"
