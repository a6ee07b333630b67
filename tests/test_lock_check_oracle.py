"""The criterion of hbls_cluster_check -- a row lies on a polynomial of degree < t iff its t-th forward
differences vanish -- restated over the oracle (tests/gpu_helpers/lock_check.py) and held to the
properties include/hipbls.h states, on (n, t) = (4, 3), (4, 4), (3, 2), (5, 1); the restatement is what
the GPU tests compare the kernels with.  And Cluster.inconsistent's candidate rule
(charon_amd/callers.py lock_check_candidates) on masks alone.  No GPU.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPERS = os.path.join(ROOT, "tests", "gpu_helpers")
if HELPERS not in sys.path:
    sys.path.insert(0, HELPERS)

import lock_check as lc  # noqa: E402

SHAPES = [(4, 3), (4, 4), (3, 2), (5, 1)]


def both(scalars, t, statuses=None):
    """the oracle's group law and the construction agree; -> (status, mask)"""
    st = statuses or [0] * len(scalars)
    got = lc.check_points([lc.point(s) for s in scalars], st, t)
    assert got == lc.check_scalars(scalars, st, t)
    return got


@pytest.mark.parametrize("n,t", SHAPES)
def test_honest_rows_pass(n, t):
    for seed in range(3):
        assert both(lc.honest(n, t, seed), t) == (lc.OK, 0)


@pytest.mark.parametrize("n,t", SHAPES)
def test_a_single_wrong_key_fails_exactly_its_windows(n, t):
    for p in range(n + 1):
        s = lc.honest(n, t, p)
        s[p] = (s[p] + 12345) % lc.B.R
        assert both(s, t) == (lc.NOT_VERIFIED, lc.window_mask(n, t, p)), p
        s[p] = 0  # the key replaced by the point at infinity: the identity in the sums, wrong all the same
        assert both(s, t) == (lc.NOT_VERIFIED, lc.window_mask(n, t, p)), p


@pytest.mark.parametrize("n,t", [(n, t) for n, t in SHAPES if t < n])
def test_a_row_of_degree_t_fails_at_t_and_passes_above(n, t):
    s = lc.honest(n, t, 5, degree=t)
    assert both(s, t) == (lc.NOT_VERIFIED, (1 << (n - t + 1)) - 1), "every window: the t-th difference is t! a_t"
    assert both(s, t + 1) == (lc.OK, 0)


@pytest.mark.parametrize("n,t", [(n, t) for n, t in SHAPES if t >= 2])
def test_a_row_of_lower_degree_passes(n, t):
    assert both(lc.honest(n, t, 6, degree=t - 2), t) == (lc.OK, 0)


def test_a_bad_status_decides_before_anything_is_computed():
    s = lc.honest(4, 3, 1)
    s[2] += 1
    for p in range(5):
        st = [0] * 5
        st[p] = 1
        assert both(s, 3, st) == (lc.BAD_PUBKEY, 0)


def test_a_row_at_infinity_passes():
    assert both([0] * 6, 1) == (lc.OK, 0) and both([0] * 5, 3) == (lc.OK, 0)


def test_swapped_pubshares_fail():
    s = lc.honest(4, 3, 2)
    s[1], s[3] = s[3], s[1]
    st, mask = both(s, 3)
    assert st == lc.NOT_VERIFIED and mask == 0b11


def test_golden_rows_are_the_oracles():
    """tests/golden/lock_rows.json holds every full-size key of the 64-share rows; a sample recomputed"""
    want = sorted({s for n, t in lc.BIG_SHAPES for _, scalars, _ in lc.big_rows(n, t) for s in scalars if s.bit_length() > 64})
    assert sorted(lc.golden_keys()) == want
    for s in want[::40]:
        assert lc.golden_keys()[s] == lc.key(s, cached=False)


@pytest.mark.parametrize("n,t", lc.BIG_SHAPES)
def test_the_64_share_rows_by_construction(n, t):
    """the construction's verdicts for the rows the kernel tests run at 64 shares: honest passes, a single
    wrong key fails its windows"""
    got = {name: lc.check_scalars(s, st, t) for name, s, st in lc.big_rows(n, t)}
    mid = n // 2
    assert got["honest0"] == (lc.OK, 0) and got["status1"] == (lc.BAD_PUBKEY, 0)
    assert got["replace0"] == (lc.NOT_VERIFIED, lc.window_mask(n, t, 0))
    assert got["replace_n"] == (lc.NOT_VERIFIED, lc.window_mask(n, t, n))
    assert got["replace_mid"] == got["infinity"] == (lc.NOT_VERIFIED, lc.window_mask(n, t, mid))
    assert got["swapped"] == (lc.NOT_VERIFIED, lc.window_mask(n, t, 1) | lc.window_mask(n, t, n))


# ---- Cluster.inconsistent's candidate rule, on masks alone

def test_candidates_of_a_single_wrong_key():
    from charon_amd.callers import lock_check_candidates
    for n, t in SHAPES + [(10, 7), (64, 33), (64, 64)]:
        for p in range(n + 1):
            got = lock_check_candidates(n, t, lc.window_mask(n, t, p))
            assert p in got
            # every candidate has the same windows as p: the windows cannot tell them apart
            assert all(lc.window_mask(n, t, q) == lc.window_mask(n, t, p) for q in got)
            assert got == [q for q in range(n + 1) if lc.window_mask(n, t, q) == lc.window_mask(n, t, p)]


def test_candidates_are_unique_where_the_windows_determine_the_position():
    from charon_amd.callers import lock_check_candidates
    # (10, 7): windows 0 .. 3 hold 0..7, 1..8, 2..9, 3..10
    assert lock_check_candidates(10, 7, 0b0001) == [0]
    assert lock_check_candidates(10, 7, 0b0011) == [1]
    assert lock_check_candidates(10, 7, 0b0111) == [2]
    assert lock_check_candidates(10, 7, 0b1111) == [3, 4, 5, 6, 7]
    assert lock_check_candidates(10, 7, 0b1110) == [8]
    assert lock_check_candidates(10, 7, 0b1000) == [10]
    # one window only: every position is a candidate
    assert lock_check_candidates(4, 4, 1) == [0, 1, 2, 3, 4]


def test_no_candidate_without_a_failure_or_without_a_single_explanation():
    from charon_amd.callers import lock_check_candidates
    assert lock_check_candidates(10, 7, 0) == []
    assert lock_check_candidates(10, 7, 0b0101) == [], "no single position fails windows 0 and 2 but not 1"
    assert lock_check_candidates(5, 1, 0b10001) == []


def test_candidates_refuse_a_mask_outside_its_windows():
    from charon_amd.callers import lock_check_candidates
    from charon_amd.tbls import TblsError
    for n, t, w in ((10, 7, 1 << 4), (4, 0, 0), (4, 5, 0)):
        with pytest.raises(TblsError):
            lock_check_candidates(n, t, w)
