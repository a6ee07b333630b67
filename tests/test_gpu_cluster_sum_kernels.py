"""k_cluster_row_sum on the GPU, through the device harness tests/native/more/clustersumdev.hip (which
compiles the product's charon_amd/csrc/cluster.hip), followed by what hbls_cluster_verify_aggregate runs
behind it: the k_seg_sum<false> passes (segments of 32, as hipbls.hip plans them) and k_va_point, through
the vb block harness.  Expected values are the oracle's group law (oracle/bls12381.py g1_add) over the
test's own points; the row sums, the affine result and the flags are compared exactly.  Every output
array carries sentinel entries behind it.

Shapes: 1, 33 (one more than a segment), 63 and 65 rows (a wave edge) of n_shares 1, 4 and 64.  Row
contents, each for the branch it reaches: two equal selected keys (the doubling branch of the addition), a
key and its inverse (the identity mid-sum, then more keys where the row has them), a selected entry at
infinity, every selected key cancelling across rows (the total is the identity), a selected bad-status
entry (the flag set; the sum's value is not compared), an unselected bad-status entry (the flag clear)
and the empty selection.
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

import blocks_ref as R  # noqa: E402
import lock_check as lc  # noqa: E402
from oracle import bls12381 as B  # noqa: E402

PAD = 5
S8, S32 = 0xEE, 0xC3A5C3A5  # a sentinel byte is no status; a sentinel "value" is above 2p
SEG = 32                    # hipbls.hip VA_SEG
ROWS = [1, 33, 63, 65]
SHARES = [1, 4, 64]
POOL = [3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41]  # small scalars of H: short oracle ladders, cached


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _ok(rc, what):
    if rc in (-5, -6):  # devblocks.h DB_E_LAUNCH, DB_E_SYNC: a GPU error; nothing more is started on the card
        pytest.exit(f"{what} returned {rc}: the GPU reported an error; no further test is run", returncode=3)
    assert rc == 0, f"{what} returned {rc}"


@pytest.fixture(scope="module")
def D(hipbls):
    from gpu_helpers import harness, more_harness
    lib = more_harness.load("clustersumdev")
    I, V, U32, U64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    lib.csd_row_sum.argtypes = [I, U32, U64, U32, V, V, I, V, V]
    assert lib.csd_sum_bytes() == 4 * 36
    vb = harness.load_devblocks("vb")
    vb.db_vb_seg_sum.argtypes = [I, V, V, U32, V, U32, V, V, U32]
    vb.db_vb_va_point.argtypes = [V, U32, V, U32, V, U32]
    return lib, vb


def selected(n_shares, mask, with_dv):
    return [j for j in range(n_shares + 1) if (with_dv == 1 if j == 0 else (mask >> (j - 1)) & 1)]


def oracle_sum(scalars):
    """the oracle's group law over the points [s] H (None: infinity), left to right"""
    acc = None
    for s in scalars:
        acc = B.g1_add(acc, lc.point(s))
    return acc


def decode(words):
    w = [int(v) for v in words]
    assert all(R.from_words(w[12 * k:12 * k + 12]) < 2 * B.P for k in range(3)), "a stored word is not below 2p"
    return R.entry_affine(1, w)


def pipeline(D, n_shares, mask, with_dv, rows, statuses):
    """rows: per row the 1 + n_shares scalars of H (0: infinity); statuses: per row its bytes.
    -> (row sums as oracle points, row flags, the affine result or None, the final flag)"""
    lib, vb = D
    nr = len(rows)
    pks = np.frombuffer(b"".join(lc.key(s) if s % B.R else lc.INF for r in rows for s in r), np.uint8).copy()
    st = np.array([x for r in statuses for x in r], np.uint8)
    assert len(pks) == 48 * nr * (1 + n_shares) and len(st) == nr * (1 + n_shares)
    sums = np.full((nr + PAD, 36), S32, np.uint32)
    flags = np.full(nr + PAD, S8, np.uint8)
    _ok(lib.csd_row_sum(nr, n_shares, mask, with_dv, _p(pks), _p(st), PAD, _p(sums), _p(flags)), "csd_row_sum")
    assert (sums[nr:] == S32).all() and (flags[nr:] == S8).all(), "sentinels behind the row sums / flags"
    row_pts = [decode(sums[g]) for g in range(nr)]
    row_flags = flags[:nr].tolist()
    # the k_seg_sum<false> passes of one group, down to one point and one flag
    cur, cur_st = np.ascontiguousarray(sums[:nr]), np.ascontiguousarray(flags[:nr])
    while True:
        n = len(cur)
        off = np.array(list(range(0, n, SEG)) + [n], np.uint32)
        n_seg = len(off) - 1
        out = np.full((n_seg + PAD, 36), S32, np.uint32)
        out_st = np.full(n_seg + PAD, S8, np.uint8)
        _ok(vb.db_vb_seg_sum(0, _p(cur), _p(cur_st), n, _p(off), n_seg, _p(out), _p(out_st), n_seg + PAD), "db_vb_seg_sum")
        assert (out[n_seg:] == S32).all() and (out_st[n_seg:] == S8).all(), "sentinels behind a pass"
        cur, cur_st = np.ascontiguousarray(out[:n_seg]), np.ascontiguousarray(out_st[:n_seg])
        if n_seg == 1:
            break
    sog = np.array([0], np.uint32)
    pt = np.full((1 + PAD, 28), S32, np.uint32)
    _ok(vb.db_vb_va_point(_p(cur), 1, _p(sog), 1, _p(pt), 1 + PAD), "db_vb_va_point")
    assert (pt[1:] == S32).all(), "sentinels behind the affine point"
    w = [int(v) for v in pt[0]]
    assert w[25:] == [0, 0, 0] and w[24] in (0, 1)
    x, y = R.from_words(w[:12]), R.from_words(w[12:24])
    assert x < 2 * B.P and y < 2 * B.P
    final = None if w[24] else (R.unmont(x), R.unmont(y))
    if w[24]:
        assert (x, y) == (0, 0)
    return row_pts, row_flags, final, int(cur_st[0])


def check(D, n_shares, mask, with_dv, rows, statuses):
    sel = selected(n_shares, mask, with_dv)
    row_pts, row_flags, final, flag = pipeline(D, n_shares, mask, with_dv, rows, statuses)
    want_flags = [int(np.bitwise_or.reduce([st[j] for j in sel] or [0])) for st in statuses]
    assert row_flags == want_flags
    assert flag == int(np.bitwise_or.reduce(want_flags))
    total = None
    for g, r in enumerate(rows):
        want = oracle_sum([r[j] for j in sel])
        if not want_flags[g]:
            assert row_pts[g] == want, ("row", g)
        total = B.g1_add(total, want)
    if not flag:
        assert final == total
    return row_pts, final, flag


def base_rows(nr, n_shares, seed):
    return [[POOL[(seed + 5 * g + 3 * j) % len(POOL)] + 97 * ((g + j) % 3) for j in range(n_shares + 1)] for g in range(nr)]


def clean(nr, n_shares):
    return [[0] * (n_shares + 1) for _ in range(nr)]


@pytest.mark.parametrize("n_shares", SHARES)
@pytest.mark.parametrize("nr", ROWS)
def test_row_contents(D, nr, n_shares):
    """all shares and the DV key selected: equal keys, a key and its inverse, an entry at infinity"""
    rows = base_rows(nr, n_shares, 1)
    mask = (1 << n_shares) - 1
    g_eq, g_inv, g_inf = 0, nr // 2, nr - 1
    rows[g_eq][1] = rows[g_eq][0]                      # P, P, ...: the doubling branch
    rows[g_inv] = list(rows[g_inv])
    rows[g_inv][1] = B.R - rows[g_inv][0]              # P, -P, then the row's other keys
    rows[g_inf][n_shares] = 0                          # a selected entry at infinity
    if nr == 1:
        rows[0][1] = rows[0][0]
    row_pts, final, flag = check(D, n_shares, mask, 1, rows, clean(nr, n_shares))
    assert flag == 0 and final is not None
    if n_shares == 1 and nr > 1:
        assert row_pts[g_inv] is None, "a key and its inverse alone: the identity"
        assert row_pts[g_eq] == B.g1_add(lc.point(rows[g_eq][0]), lc.point(rows[g_eq][0]))
    # every row of entries at infinity
    inf_rows = [[0] * (n_shares + 1) for _ in range(nr)]
    row_pts, final, flag = check(D, n_shares, mask, 1, inf_rows, clean(nr, n_shares))
    assert row_pts == [None] * nr and final is None and flag == 0


@pytest.mark.parametrize("n_shares", SHARES)
@pytest.mark.parametrize("nr", ROWS)
def test_every_selected_key_cancels_across_rows(D, nr, n_shares):
    """row 2i + 1 holds the inverses of row 2i's selected keys (an odd last row cancels within itself or is at
    infinity): the total is the identity, through every pass"""
    mask = (1 << n_shares) - 1 if n_shares < 64 else 0x5A5A5A5A5A5A5A5B
    sel = selected(n_shares, mask, 0)
    rows = base_rows(nr, n_shares, 2)
    for g in range(1, nr, 2):
        rows[g] = [(B.R - s) if j in sel else s for j, s in enumerate(rows[g - 1])]
    if nr % 2:
        last = rows[nr - 1]  # pairs (a, -a) over the selected entries; an odd one out at infinity
        for k in range(0, len(sel) - 1, 2):
            last[sel[k + 1]] = B.R - last[sel[k]]
        if len(sel) % 2:
            last[sel[-1]] = 0
    row_pts, final, flag = check(D, n_shares, mask, 0, rows, clean(nr, n_shares))
    assert final is None and flag == 0
    if nr > 1:
        assert row_pts[0] is not None and row_pts[1] == B.g1_neg(row_pts[0])


@pytest.mark.parametrize("n_shares", SHARES)
@pytest.mark.parametrize("nr", ROWS)
def test_statuses_and_selections(D, nr, n_shares):
    rows = base_rows(nr, n_shares, 3)
    st = clean(nr, n_shares)
    g = nr - 1
    st[g][n_shares] = B.ST_BAD_PUBKEY  # the last pubshare of the last row
    all_shares = (1 << n_shares) - 1
    # selected: the flag is set, in the row and at the end (the sum's value is not compared)
    _, _, flag = check(D, n_shares, all_shares, 0, rows, st)
    assert flag == B.ST_BAD_PUBKEY
    # unselected: the DV key alone, or the shares below the bad one -- the flag is clear and the sum exact
    _, final, flag = check(D, n_shares, 0, 1, rows, st)
    assert flag == 0 and final == oracle_sum([r[0] for r in rows])
    if n_shares > 1:
        _, final, flag = check(D, n_shares, all_shares >> 1, 0, rows, st)
        assert flag == 0 and final is not None
    # a bad DV key, unselected and selected
    st2 = clean(nr, n_shares)
    st2[0][0] = 4
    assert check(D, n_shares, all_shares, 0, rows, st2)[2] == 0
    assert check(D, n_shares, all_shares, 1, rows, st2)[2] == 4
    # single shares: the lowest and the highest valid bit
    for j in {1, n_shares}:
        _, final, flag = check(D, n_shares, 1 << (j - 1), 0, rows, clean(nr, n_shares))
        assert flag == 0 and final == oracle_sum([r[j] for r in rows])
    # the empty selection: every row sum is the identity, nothing is flagged whatever the statuses
    row_pts, final, flag = check(D, n_shares, 0, 0, rows, st)
    assert row_pts == [None] * nr and final is None and flag == 0


def test_the_harness_refuses_what_the_rule_refuses(D):
    lib, _ = D
    pks = np.frombuffer(lc.key(3) * 5, np.uint8).copy()
    st = np.zeros(5, np.uint8)
    sums, flags = np.full((1 + PAD, 36), S32, np.uint32), np.full(1 + PAD, S8, np.uint8)
    for mask, with_dv in ((1 << 4, 0), (1, 2), (1 << 63, 1)):
        assert lib.csd_row_sum(1, 4, mask, with_dv, _p(pks), _p(st), PAD, _p(sums), _p(flags)) == 2
    assert (sums == S32).all() and (flags == S8).all()
