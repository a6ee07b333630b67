"""The kernels of hbls_cluster_check on the GPU, one launcher at a time, through the device harness
tests/native/lockcheckdev.hip (which compiles the product's charon_amd/csrc/lockcheck.hip):
k_lock_check's verdict per (row, window) and k_lock_fold's row_status and row_windows against the
criterion restated over the oracle (tests/gpu_helpers/lock_check.py), exactly.  Every output array
carries sentinel entries behind it, and a row with a bad-status key must leave its verdict bytes and its
row_windows word as the test preset them.

Shapes, each for the branch it reaches: (4, 3) x 23 rows = 46 lanes, a partial wave; (10, 7) x 23 rows =
92 lanes, two waves with wrong keys on both sides of the boundary (charon's shape; 64 / 4 rows fill a wave,
so no row straddles it) and (10, 6) x 23 rows, 5 windows a row, where row 12 does; (5, 1) x 14 rows, every window
P_{k+1} - P_k of equal points (the cancellation branch), one row all at infinity; (3, 2) with a row
P, P, P, P (degree 0: the doubling branch of the addition); (64, 33), 31-bit coefficients and 32
windows; (64, 64), coefficients above 2^32 and one window.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPERS = os.path.join(ROOT, "tests", "gpu_helpers")
if HELPERS not in sys.path:
    sys.path.insert(0, HELPERS)

import lock_check as lc  # noqa: E402

PAD = 8
S8, S64 = 0xA5, 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def D(hipbls):
    from gpu_helpers import harness
    lib = harness.load("lockcheckdev")
    I, V, U32 = ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32
    lib.ld_check.argtypes = [I, U32, U32, V, V, I, V, V, V]
    return lib


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def run(D, n, t, rows):
    """rows: [(name, scalars, statuses)] -> (verdict rows x W, row_status, row_windows), sentinels checked"""
    W, nr = n - t + 1, len(rows)
    pks = np.frombuffer(b"".join(lc.compress(s) for _, s, _ in rows), np.uint8).copy()
    st = np.array([x for _, _, stt in rows for x in stt], np.uint8)
    assert len(pks) == 48 * nr * (n + 1) and len(st) == nr * (n + 1)
    verdict = np.full(nr * W + PAD, S8, np.uint8)
    status = np.full(nr + PAD, S8, np.uint8)
    windows = np.full(nr + PAD, S64, np.uint64)
    rc = D.ld_check(nr, n, t, _p(pks), _p(st), PAD, _p(verdict), _p(status), _p(windows))
    assert rc == 0
    assert (verdict[nr * W:] == S8).all() and (status[nr:] == S8).all() and (windows[nr:] == S64).all(), "sentinels"
    return verdict[:nr * W].reshape(nr, W), status[:nr], windows[:nr]


def compare(D, n, t, rows, reference):
    verdict, status, windows = run(D, n, t, rows)
    W = n - t + 1
    seen = set()
    for g, (name, s, st) in enumerate(rows):
        want_st, want_mask = reference(s, st)
        seen.add(want_st)
        assert status[g] == want_st, (name, g)
        if want_st == lc.BAD_PUBKEY:  # nothing computed, nothing of its own written
            assert windows[g] == S64 and (verdict[g] == S8).all(), (name, g)
        else:
            assert int(windows[g]) == want_mask, (name, g, bin(int(windows[g])), bin(want_mask))
            assert verdict[g].tolist() == [(want_mask >> k) & 1 for k in range(W)], (name, g)
    assert seen == {lc.OK, lc.BAD_PUBKEY, lc.NOT_VERIFIED}, "the rows reach every status"
    return status, windows


def by_points(t):
    return lambda s, st: lc.check_points([lc.point(x) for x in s], st, t)


def by_scalars(t):
    return lambda s, st: lc.check_scalars(s, st, t)


def test_partial_wave_4_3(D):
    rows = lc.shape_rows(4, 3, honest_rows=17)
    assert len(rows) * 2 == 46
    status, windows = compare(D, 4, 3, rows, by_points(3))
    names = [r[0] for r in rows]
    assert int(windows[names.index("replace0")]) == lc.window_mask(4, 3, 0) == 0b01
    assert int(windows[names.index("replace_n")]) == lc.window_mask(4, 3, 4) == 0b10
    assert int(windows[names.index("replace_mid")]) == int(windows[names.index("infinity")]) == 0b11


def test_two_waves_10_7(D):
    rows = lc.shape_rows(10, 7, honest_rows=17)
    # the special rows at 12 .. 17: lanes 48 .. 71, on both sides of the wave boundary (row 16 starts wave 1)
    rows = rows[:12] + rows[17:] + rows[12:17]
    assert len(rows) == 23 and len(rows) * 4 == 92
    status, windows = compare(D, 10, 7, rows, by_points(7))
    for g, (name, _, _) in enumerate(rows):
        if name.startswith("replace"):
            p = {"replace0": 0, "replace_n": 10, "replace_mid": 5}[name]
            assert int(windows[g]) == lc.window_mask(10, 7, p)


def test_rows_straddle_the_wave_boundary_10_6(D):
    """(10, 6): 5 windows a row, so row 12 holds lanes 60 .. 64 -- a row on both sides of the boundary"""
    rows = lc.shape_rows(10, 6, honest_rows=17)
    rows = rows[:10] + rows[17:] + rows[10:17]  # the special rows at 10 .. 15
    assert rows[12][0] == "replace_mid" and 12 * 5 < 64 < 13 * 5 and len(rows) * 5 == 115
    status, windows = compare(D, 10, 6, rows, by_points(6))
    assert int(windows[12]) == lc.window_mask(10, 6, 5) == 0b11111


def test_cancellation_5_1(D):
    rows = lc.shape_rows(5, 1, honest_rows=7)
    rows.append(("all_infinity", [0] * 6, [0] * 6))
    assert len(rows) == 14
    status, windows = compare(D, 5, 1, rows, by_points(1))
    names = [r[0] for r in rows]
    assert status[names.index("all_infinity")] == lc.OK and int(windows[names.index("all_infinity")]) == 0
    assert status[names.index("swapped")] == lc.OK, "a constant row: the swap changes nothing"
    assert int(windows[names.index("replace_mid")]) == 0b00110


def test_degree_zero_3_2(D):
    rows = lc.shape_rows(3, 2)
    rows.append(("constant", [777] * 4, [0] * 4))  # P, P, P, P: P - 2P + P, the addition's doubling branch
    rows.append(("degree2", lc.honest(3, 2, 9, degree=2), [0] * 4))
    status, windows = compare(D, 3, 2, rows, by_points(2))
    names = [r[0] for r in rows]
    assert status[names.index("constant")] == lc.OK
    assert int(windows[names.index("degree2")]) == 0b11


@pytest.mark.parametrize("n,t", lc.BIG_SHAPES)
def test_64_shares(D, n, t):
    rows = lc.big_rows(n, t)
    status, windows = compare(D, n, t, rows, by_scalars(t))
    names = [r[0] for r in rows]
    assert status[names.index("honest0")] == lc.OK
    assert int(windows[names.index("replace_n")]) == lc.window_mask(n, t, n)


def test_refused_shapes(D):
    pks = np.frombuffer(lc.compress([1] * 5), np.uint8).copy()
    st = np.zeros(5, np.uint8)
    out = np.full(16, S8, np.uint8)
    w = np.full(16, S64, np.uint64)
    for t in (0, 5):
        assert D.ld_check(1, 4, t, _p(pks), _p(st), PAD, _p(out), _p(out), _p(w)) == 2
    assert (out == S8).all() and (w == S64).all()
