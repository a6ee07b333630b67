"""hbls_cluster_check through the ABI and callers.Cluster, -m gpu: do a lock's pubshares interpolate to its
DV keys.

The cases are tests/gpu_helpers/lock_check_cases.py (a 6-validator lock built with the library's own
hbls_threshold_split and hbls_secret_to_public_key_batch; expected statuses and window masks from the
criterion and from its oracle restatement, tests/gpu_helpers/lock_check.py).  They run ONCE, in a child
pytest process with the default four hardware queues, and each test here asserts on its case's outcome;
none is deselected or skipped.

Why a child: tests/test_gpu_cluster.py's reason.  The cases open clusters under one, two and three contexts
(with ladder tables once: k_cluster_wide, 3 096 B of scratch per lane on each context's library stream)
and run duties on them, and a run of the whole tests/ directory is at the device's per-queue scratch
reservations with nothing to spare.  In a process of their own, which ends with them, the cases reserve
nothing in the suite's process.  k_lock_check itself keeps 8 B of scratch per lane; its kernel tests
(tests/test_gpu_lock_check_kernels.py) run in the suite's process.
"""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join("tests", "gpu_helpers", "lock_check_cases.py")
IDS = ['test_an_honest_lock',
       'test_a_lock_with_swapped_pubshares_and_a_wrong_dv_key',
       'test_call_errors_write_nothing',
       'test_an_unusable_row_is_not_an_inconsistent_one',
       'test_shards[2]',
       'test_shards[3]',
       'test_a_check_changes_nothing_a_duty_returns',
       'test_callers_cluster']


@pytest.fixture(scope="module")
def outcome(hipbls):
    """case id -> PASSED / FAILED / ..., and the child's whole output"""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")  # the count a process has by default, whatever this one was started with
    r = subprocess.run([sys.executable, "-m", "pytest", CASES, "-v", "-x", "-p", "no:cacheprovider"], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    text = r.stdout + r.stderr
    return dict(re.findall(r"lock_check_cases\.py::(\S+) (PASSED|FAILED|ERROR|SKIPPED|XFAIL|XPASS)", text)), text


@pytest.mark.parametrize("case", IDS)
def test_case(outcome, case):
    got, text = outcome
    assert got.get(case) == "PASSED", f"{case}: {got.get(case, 'not run')}\n" + text[-6000:]


def test_every_case_of_the_file_is_listed(outcome):
    assert sorted(outcome[0]) == sorted(IDS), "tests/gpu_helpers/lock_check_cases.py and IDS name the same cases"
