"""First-error duty set adds through the ABI (hbls_duty_add_sets_first / hbls_duty_first_stats), -m gpu:
a rejected set is stopped at its first failure.

The cases are tests/gpu_helpers/duty_first_cases.py (on the clusters and streams of tests/test_gpu_duty.py,
every call against a twin duty on hbls_duty_add_sets under the defining property and the vstatus
contract of include/hipbls.h).  They run ONCE, in a child pytest process with the default four hardware
queues, and each test here asserts on its case's outcome.

Why a child.  The runtime reserves scratch per hardware queue for the largest kernel the queue has run
(tests/gpu_helpers/hash_harness.py has the sizing).  A run of the whole tests/ directory has 32 hardware
queues (tests/test_bench_launcher.py imports bench.py before HIP starts) and is, by that file's count, at
the device's scratch with nothing to spare.  These cases drive a duty of 1 792 partials in one call
through the slot-wide, per-batch, chunked and per-item paths, on one to three contexts, and so run the
scratch-heavy kernels (k_pk_wide 3 096 B per lane, k_rlc 1 536, k_dec_sig_pt 584) on queues that the
suite's other duty tests leave to smaller ones.  In the suite's process that reservation ran queues out
of scratch (HSA_STATUS_ERROR_OUT_OF_RESOURCES): first in this file's own three-context case, then, with
only that case moved out, in tests/test_gpu_duty_sets.py's two-context case behind it.  In a process of
their own, which ends with them, the cases reserve nothing in the suite's process.
"""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join("tests", "gpu_helpers", "duty_first_cases.py")
IDS = ['test_clean_one_set_per_call_and_all_sets_in_one_call',
       'test_one_corrupted_partial[first]',
       'test_one_corrupted_partial[middle]',
       'test_one_corrupted_partial[last]',
       'test_sets_cut_across_the_batches',
       'test_head_batch_failing_through_the_previous_set_only',
       'test_a_set_with_bad_partials_in_many_batches_is_left_unchecked_behind_the_first',
       'test_all_undecodable_and_all_wrong',
       'test_slot_wide_check_and_the_adaptive_per_batch_path',
       'test_chunked_groups',
       'test_below_the_batched_final_exponentiation_statuses_are_exact',
       'test_device_split[2]',
       'test_device_split[3]',
       'test_the_three_add_calls_mixed_on_one_duty',
       'test_call_errors',
       'test_parsig_duty_first_error']


@pytest.fixture(scope="module")
def outcome(hipbls):
    """case id -> PASSED / FAILED / ..., and the child's whole output"""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")  # the count a process has by default, whatever this one was started with
    r = subprocess.run([sys.executable, "-m", "pytest", CASES, "-v", "-x", "-p", "no:cacheprovider"], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    text = r.stdout + r.stderr
    return dict(re.findall(r"duty_first_cases\.py::(\S+) (PASSED|FAILED|ERROR|SKIPPED|XFAIL|XPASS)", text)), text


@pytest.mark.parametrize("case", IDS)
def test_case(outcome, case):
    got, text = outcome
    assert got.get(case) == "PASSED", f"{case}: {got.get(case, 'not run')}\n" + text[-6000:]


def test_every_case_of_the_file_is_listed(outcome):
    assert sorted(outcome[0]) == sorted(IDS), "tests/gpu_helpers/duty_first_cases.py and IDS name the same cases"
