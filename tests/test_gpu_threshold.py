"""The threshold-aggregation kernels (charon_amd/csrc/threshold.hip) on the GPU, one launcher at a
time, against Python integers.

This is the stage that turns decompressed partials and share indices into the per-member Jacobian sums
k_group_sum compresses.  Through the C ABI a test sees 96 bytes and a status per group and cannot see
which of the three paths per group (small-scalar, joint, per-member) produced them; on honest share
indices most of them are never taken: the small-scalar path takes every wave that shares one index set
of up to 16 small indices, and no other GPU test hands the later kernels a wave whose digits agree while
that split is refused (t > 16, an index of 2^31 or more), so the wave-uniform NAF branch of k_ta_straus
and the whole of k_ta_jtab / k_ta_jladder are observed only here, on digits given directly.  The test-only ta harness (tests/native/devblocks_threshold.hip, a
library of its own that compiles the product's threshold.hip itself) runs one product launcher, or one
launcher sequence the product issues, per call; every output array is pre-filled with a sentinel and
copied back in full, so the entries a kernel must not write are compared too.

References (tests/blocks_ref.py, pinned on the CPU by tests/test_blocks_ref.py; the code under test is
never the reference): lambda_j(0) as exact rationals reduced mod r (ta_lambda), its base-z digits
(ta_digits), the small-scalar split from Python integers (ta_small_split).  Every member point is k Q for
one fixed Q of order r, so [lambda] sigma is [(lambda k) mod r] Q and the sum for ARBITRARY digits,
sum_i a_i (-1)^i psi^i(sigma), is [(sum_i a_i z^i) k mod r] Q: one fixed-base multiplication per expected
output.  The selection rule is tests/test_tasel_host.py's rule() and tests/test_hslot.py's matching().
All comparisons are exact: Montgomery Jacobian records are decoded to affine group elements, every stored
coordinate must be below 2p and infinity must have Z = 0.  There is no tolerance anywhere in this file.

All kernels here assume members of G2 or infinity (the product replaces anything else by infinity before
this stage); the tests keep to that.  k_group_sum is hipbls.hip's, next to the C ABI, and is not compiled
into the harness: the tests sum a group's t output slots themselves, and the ABI tests keep covering
k_group_sum's status precedence.

The one value this file leaves unasserted: the sum of a joint lane that holds a member at INFINITY inside
a wave-uniform chunk (k_ta_jtab / k_ta_jladder).  By the comment above odd_tables_affine that lane's sum
is unspecified -- the member is an undecodable partial and the product discards the group by its member
flags -- so test_joint_infinite_member asserts that every OTHER lane of the wave is exact, that the lane
wrote its own cnt slots and nothing else, and that the same input is exact on k_ta_jgeneral.

Where the kernel's rule, not the issue of the day, decides a value, the docstring of the test says so:
k_ta_lambda flags member j when ANOTHER member's index is 0 or equals j's; k_ta_sprep writes csm = 0 for
every refused group it looks at, t = 1 included (only t > 16 and nonuni leave csm untouched).

Which shape reaches which branch:
  k_ta_layout / k_ta_lambda
                 n = 1 / 64 / 65 / 130 (and 51, 63, 66), groups of 1, 2, 3, 7, 17 mixed and uniform; the
                 1/d table up to |d| = 64 and the Fermat path from 65, indices at +-(2^62 - 1), 2^62,
                 INT64_MAX, INT64_MIN; a remainder above 2^63 in each of divmod_xabs's three divisions;
                 index 0 and duplicates; mode 1; skipped groups; nonuni set / untouched / null.
  k_ta_straus    n = 1 / 63 / 64 / 65 / 130, share-position-major (t = 1, n_groups = 1 among them) and
                 plain (guard 1, n no multiple of n_groups); per wave: uniform digits (NAF), one lane off
                 (general), every lane its own digits (general); the first lanes skipped (the schedule from
                 the first valid lane), a wave all skipped; every special digit vector on both branches;
                 members at infinity; src null and a permutation; guard 0.
  launch_ta_joint (1,2,2) (64,4,2) (65,4,2: a wave over two chunk positions -> general) (33,5,2: cnt 2 and
                 1 in one wave -> general) (64,5,2: the last chunk of cnt 1 uniform) (64,8,8) (70,7,3)
                 (64,17,8), each with one shared index set (k_ta_jtab + k_ta_jladder where a wave is
                 uniform) and with per-validator sets (k_ta_jgeneral); skip on lane 0, inside a wave and
                 over a whole wave (128,2,2); nonuni = 1; R = T, sigma and -sigma, a vanishing sum, an
                 infinite member inside uniform chunks.
  k_ta_sprep / launch_ta_small
                 n_groups 1 / 32 / 33 / 64 / 65 / 100, t 2 / 3 / 7 / 16, one lane per validator and lane
                 pairs; uniform waves (done 1), a wave with one validator on another set or one refused
                 group (done 0, out untouched), both in one call; t = 1, t = 17, nonuni = 1; a member at
                 infinity, Q = infinity (done 2), equal and opposite members.
  selection      n_groups 1 / 64 / 65 / 130, t 2 / 4, both modes: groups with exactly t, more, fewer, mixed
                 messages, none, a repeated share index, offsets beyond n_cand; the histogram, the counters
                 from a non-zero start; k_ta_sel_fill's class order as properties; k_ta_sel_scatter with
                 rows16 1 / 0, perm null, the optional outputs null and given; k_ta_sel_verdicts.
"""
import ctypes
import random

import numpy as np
import pytest

import blocks_ref as R
import test_gpu_vbatch as VB
import test_hslot as HS
import test_tasel_host as TS
from oracle import bls12381 as B

pytestmark = pytest.mark.gpu

Z = R.TA_Z
SENT32, SENT8, SENT64 = VB.SENT32, VB.SENT8, 0xEEEEEEEEEEEEEEEE  # no coordinate, no status, no digit (>= z)
SENTI = -0x1111111111111112  # SENT64 as a signed word: no coefficient of a cluster's index set
DB_E_ARG = -1
INT64_MAX, INT64_MIN = 2 ** 63 - 1, -2 ** 63
_ok, _ptr, _u32, _u8, untouched = VB._ok, VB._ptr, VB._u32, VB._u8, VB.untouched
W_SEL = ["n", "n_cand", "n_groups", "t", "mode"]
A_SEL = ["vstatus", "msg_idx", "src", "idx", "grp_off", "chosen", "cidx", "ta_count", "key", "state", "gmsg", "hist", "off",
         "cur", "perm", "pmem", "pgoff", "pidx", "ctr"]


def _i64(a):
    return np.ascontiguousarray(np.array([int(x) for x in a], dtype=np.int64))


def _u64(a, width=None):
    a = np.ascontiguousarray(np.array([[int(x) for x in r] for r in a] if width else [int(x) for x in a], dtype=np.uint64))
    return a.reshape(-1, width) if width else a


def _sent64(*shape):
    return np.full(shape, SENT64, dtype=np.uint64)


def _flag(v):
    return 2 if v is None else int(v)


class TA:
    def __init__(self, lib):
        self.lib = lib
        c = (ctypes.c_uint32 * 27)()
        assert lib.db_ta_consts(c) == 27
        c = list(c)
        assert c[:3] == [4 * R.HM_WORDS, 4 * 72, 32]
        self.SMALL_MAX, self.JOINT_MAX, self.INV_N, self.KEYS, self.KEY_NONE, self.NONE = c[4:10]
        assert (self.SMALL_MAX, self.JOINT_MAX, self.INV_N) == (R.TA_SMALL_T[-1], 8, 64)
        assert (self.KEYS, self.KEY_NONE, self.NONE) == (HS.KEY_NONE + 1, HS.KEY_NONE, TS.NONE)
        self.M_OK, self.M_BAD_SIG, self.M_BAD_IDX = c[10:13]
        assert len({self.M_OK, self.M_BAD_SIG, self.M_BAD_IDX}) == 3 and self.M_OK == 0
        assert c[13:16] == [TS.ST_OK, TS.ST_FEW, TS.ST_MIXED] and c[16:18] == [HS.FIRST, HS.MATCHING]
        self.OK, self.FEW, self.MIXED = c[13:16]
        self.SEL_SEEN, self.SEL_FEW, self.SEL_SHIFTED, self.SEL_SMALL, n_ctr = c[18:23]
        assert n_ctr == 4 and sorted(c[18:22]) == [0, 1, 2, 3]
        self.ST_OK, self.ST_BAD_INPUT, self.ST_UNCHECKED, self.ST_COMBINE = c[23:27]
        assert (self.ST_OK, self.ST_COMBINE) == (B.ST_OK, B.ST_COMBINE_FAILED) and self.ST_BAD_INPUT != self.ST_UNCHECKED
        assert (lib.db_ta_sel_words(), lib.db_ta_sel_ptrs()) == (len(W_SEL), len(A_SEL))
        V, U, I = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
        lib.db_ta_layout.argtypes = [V, U, U, V]
        lib.db_ta_lambda.argtypes = [V, V, U, U, U, I, U, V, V, V, V]
        lib.db_ta_member_status.argtypes = [V, U, V, U, V, U]
        lib.db_ta_straus.argtypes = [V, U, V, V, U, U, V, U, V, U]
        lib.db_ta_joint.argtypes = [V, U, V, V, U, U, U, V, U, V, U]
        lib.db_ta_sprep.argtypes = [V, U, U, U, V, V, V]
        lib.db_ta_small.argtypes = [V, U, V, V, U, U, U, U, V, V, V, V, V, U]
        lib.db_ta_select.argtypes = lib.db_ta_sel_fill.argtypes = [V, V]
        lib.db_ta_sel_scatter.argtypes = [U, V, V, V, V, V, V, I, V, V, V, V, V]
        lib.db_ta_sel_verdicts.argtypes = [V, U, V, U]

    @staticmethod
    def _done(got, what, rc):
        if rc:
            assert got == rc, (what, got, rc)
        else:
            _ok(got, what)

    def layout(self, off, t_u, start=0, rc=0):
        nonuni, o = _u8([start]), _u32(off)
        self._done(self.lib.db_ta_layout(_ptr(o), len(off) - 1, t_u, _ptr(nonuni)), "db_ta_layout", rc)
        return int(nonuni[0])

    def lam(self, idx, off, mode=0, t_u=0, nonuni=0, skip=None, mstat=None, pad=3, rc=0):
        """-> (dig [n_buf, 4], mstat [n_buf], nonuni or None); nonuni: the byte's start value or None (null)"""
        n = off[-1]
        nb = n + pad
        ix, o = _i64(list(idx) + [7] * (nb - len(idx))), _u32(off)
        dig = _sent64(nb, 4)
        ms = np.full(nb, SENT8, dtype=np.uint8)
        ms[:n] = self.M_OK if mstat is None else mstat
        nu = None if nonuni is None else _u8([nonuni])
        sk = None if skip is None else _u8(skip)
        got = self.lib.db_ta_lambda(_ptr(ix), _ptr(o), len(off) - 1, n, nb, mode, t_u, _ptr(nu), _ptr(sk), _ptr(dig), _ptr(ms))
        self._done(got, "db_ta_lambda", rc)
        return dig, ms, None if nu is None else int(nu[0])

    def member_status(self, sig_st, src, n_buf, rc=0):
        st, s, ms = _u8(sig_st), _u32(src), np.full(n_buf, SENT8, dtype=np.uint8)
        self._done(self.lib.db_ta_member_status(_ptr(st), len(st), _ptr(s), len(s), _ptr(ms), n_buf), "db_ta_member_status", rc)
        return ms

    def straus(self, pts, src, dig, n_groups, skip=None, guard=None, pad=2, out=None, rc=0):
        n = len(dig)
        out = np.full((n + pad, 72), SENT32, dtype=np.uint32) if out is None else out.copy()
        s = None if src is None else _u32(src)
        sk = None if skip is None else _u8(skip)
        d = _u64(dig, 4)
        got = self.lib.db_ta_straus(_ptr(pts), len(pts), _ptr(s), _ptr(d), n, n_groups, _ptr(sk), _flag(guard), _ptr(out), len(out))
        self._done(got, "db_ta_straus", rc)
        return out

    def joint(self, pts, src, dig, n_groups, t, c, skip=None, nonuni=None, pad=2, rc=0):
        out = np.full((n_groups * t + pad, 72), SENT32, dtype=np.uint32)
        s = None if src is None else _u32(src)
        sk = None if skip is None else _u8(skip)
        d = _u64(dig, 4)
        got = self.lib.db_ta_joint(_ptr(pts), len(pts), _ptr(s), _ptr(d), n_groups, t, c, _ptr(sk), _flag(nonuni), _ptr(out),
                                   len(out))
        self._done(got, "db_ta_joint", rc)
        return out

    def sprep(self, idx, n_groups, t, nonuni=None, rc=0):
        ix = _i64(idx)
        csm, sdig, sok = np.full(n_groups * t, SENTI, dtype=np.int64), _sent64(n_groups, 4), np.full(n_groups, SENT8, np.uint8)
        got = self.lib.db_ta_sprep(_ptr(ix), n_groups, t, _flag(nonuni), _ptr(csm), _ptr(sdig), _ptr(sok))
        self._done(got, "db_ta_sprep", rc)
        return csm.reshape(n_groups, t), sdig, sok

    def small(self, pts, src, idx, n_groups, t, pair, nonuni=None, pad=2, rc=0):
        ix = _i64(idx)
        s = None if src is None else _u32(src)
        csm, sdig, sok = np.full(n_groups * t, SENTI, dtype=np.int64), _sent64(n_groups, 4), np.full(n_groups, SENT8, np.uint8)
        done, out = np.full(n_groups, SENT8, np.uint8), np.full((n_groups * t + pad, 72), SENT32, dtype=np.uint32)
        got = self.lib.db_ta_small(_ptr(pts), len(pts), _ptr(s), _ptr(ix), n_groups, t, pair, _flag(nonuni), _ptr(csm), _ptr(sdig),
                                   _ptr(sok), _ptr(done), _ptr(out), len(out))
        self._done(got, "db_ta_small", rc)
        return dict(csm=csm.reshape(n_groups, t), sdig=sdig, sok=sok, done=done, out=out)

    def _sel(self, f, what, w, a, rc):
        wa = _u32([w[k] for k in W_SEL])
        pa = (ctypes.c_void_p * len(A_SEL))(*[_ptr(a.get(k)) for k in A_SEL])
        self._done(f(_ptr(wa), pa), what, rc)

    def select(self, w, a, rc=0):
        self._sel(self.lib.db_ta_select, "db_ta_select", w, a, rc)

    def sel_fill(self, w, a, rc=0):
        self._sel(self.lib.db_ta_sel_fill, "db_ta_sel_fill", w, a, rc)

    def sel_scatter(self, ng, perm, state, pout, pstatus, ppt, sdone, rows16, ta_out, ta_status, agg_pt, agg_st, ctr, rc=0):
        got = self.lib.db_ta_sel_scatter(ng, _ptr(perm), _ptr(state), _ptr(pout), _ptr(pstatus), _ptr(ppt), _ptr(sdone), rows16,
                                         _ptr(ta_out), _ptr(ta_status), _ptr(agg_pt), _ptr(agg_st), _ptr(ctr))
        self._done(got, "db_ta_sel_scatter", rc)

    def sel_verdicts(self, ta_status, agg, rc=0):
        st = _u8(ta_status)
        self._done(self.lib.db_ta_sel_verdicts(_ptr(st), len(st), _ptr(agg), len(agg)), "db_ta_sel_verdicts", rc)


@pytest.fixture(scope="module")
def ta():
    """The ta harness, loaded only if it was built from this tree (its embedded id); otherwise built now,
    and a failure of that fails the tests with the id in the message."""
    from gpu_helpers import harness
    return TA(harness.load_devblocks("ta"))


@pytest.fixture(scope="module")
def vw():
    """the members: sig[i] = k[i] Q (tests/test_gpu_vbatch.py's world, 48 points)"""
    return VB.World()


def hm_rows(vw, scalars):
    """HmEntry rows of [s] Q per scalar; None: the decompression's infinity (zero coordinates, inf set)"""
    return _u32([VB.hme(None if s is None else vw.f2.mul(s)) for s in scalars], 52)


def elem(row):
    return VB.decode(2, row)


def check_rows(vw, rows, want):
    """rows[i] is [want[i]] Q (a scalar; 0: infinity) or, for want[i] None, still the sentinel"""
    assert len(rows) == len(want)
    for i, s in enumerate(want):
        if s is None:
            assert untouched(rows[i]), i
        else:
            assert elem(rows[i]) == vw.f2.mul(s), i


def lane_member(L, n, n_groups, plain):
    """launch_ta_straus's lane -> member map: share-position-major when every group has n / n_groups members"""
    if plain or n % n_groups:
        return L
    t = n // n_groups
    return (L % n_groups) * t + L // n_groups


# ---- k_ta_layout / k_ta_lambda ------------------------------------------------------------------
def divmod_crossings(v):
    """per division of k_ta_lambda's three: does divmod_xabs's running remainder reach 2^63 (the
    `r >> 63` branch, where the shifted remainder no longer fits 64 bits)?"""
    out = []
    for _ in range(3):
        r, crossed = 0, False
        for bit in range(255, -1, -1):
            crossed = crossed or r >> 63 != 0
            r = (r << 1) | ((v >> bit) & 1)
            if r >= Z:
                r -= Z
        out.append(crossed)
        v //= Z
    return out


def lambda_expect(ta, groups, mode, mstat, skip):
    """(digits or None per member, mstat per member).  The kernel's rule for a combine failure: member
    j is flagged when ANOTHER member's index is 0 or equals its own (blocks_ref.ta_lambda's None), unless it
    is already undecodable; a flagged member, a group of one and mode 1 have the digits (1, 0, 0, 0)."""
    dig, ms, j = [], [], 0
    for g, ids in enumerate(groups):
        lam = R.ta_lambda(ids)
        for k in range(len(ids)):
            st = int(mstat[j])
            if skip is not None and skip[g]:
                dig.append(None)
            elif mode == 1 or len(ids) == 1:
                dig.append([1, 0, 0, 0])
            elif lam[k] is None:
                dig.append([1, 0, 0, 0])
                st = ta.M_BAD_IDX if st == ta.M_OK else st
            else:
                dig.append(R.ta_digits(lam[k]))
            ms.append(st)
            j += 1
    return dig, ms


def nonuni_expect(off, t_u, start, lanes_only):
    """k_ta_layout's rule per group; k_ta_lambda applies it from its lanes, so only to groups with members"""
    hit = any((off[g + 1] - off[g] != t_u or off[g] != g * t_u) and (not lanes_only or off[g + 1] > off[g])
              for g in range(len(off) - 1))
    return 1 if (t_u and hit) else start


def run_lambda(ta, groups, mode=0, t_u=0, nonuni=0, skip=None, mstat=None):
    off = VB._offsets([len(g) for g in groups])
    n = off[-1]
    idx = [x for g in groups for x in g]
    ms_in = [ta.M_OK] * n if mstat is None else mstat
    dig, ms, nu = ta.lam(idx, off, mode, t_u, nonuni, skip, ms_in)
    want_d, want_m = lambda_expect(ta, groups, mode, ms_in, skip)
    for j in range(n):
        assert [int(x) for x in dig[j]] == (want_d[j] if want_d[j] is not None else [SENT64] * 4), (j, idx[j])
    assert [int(x) for x in ms[:n]] == want_m
    assert (dig[n:] == SENT64).all() and untouched(ms[n:])
    if nonuni is None:
        assert nu is None
    else:
        assert nu == nonuni_expect(off, t_u, nonuni, True)
        if t_u:  # k_ta_layout agrees (every group of these layouts has members, or the rule fires before it)
            assert ta.layout(off, t_u, nonuni) == nonuni_expect(off, t_u, nonuni, False) == nu
    return dig


def index_set(rng, size, kind):
    """`size` distinct non-zero share indices: 0 a prefix 1..size, 1 shuffled out of 1..10 (or 1..size + 3),
    2 signed"""
    if kind == 0:
        return list(range(1, size + 1))
    if kind == 1:
        return rng.sample(range(1, max(10, size + 3) + 1), size)
    return rng.sample([x for x in range(-12, 13) if x], size) if size <= 24 else list(range(-size, 0))


def mixed_groups(rng, n):
    groups, left, i = [], n, 0
    while left:
        s = min([1, 2, 3, 7, 17][i % 5], left)
        groups.append(index_set(rng, s, i % 3))
        left -= s
        i += 1
    return groups


@pytest.mark.parametrize("n", [1, 64, 65, 130])
def test_lambda_mixed_groups(ta, n):
    """groups of 1, 2, 3, 7, 17 in turn (prefixes, shuffled and signed index sets) up to n members: the
    digits are those of the exact lambda; t_u = 3 does not describe the layout, so nonuni is set (n > 1:
    a lone group of one does not match t_u = 3 either); t_u = 0 and a null pointer leave it alone"""
    rng = random.Random(500 + n)
    groups = mixed_groups(rng, n)
    assert sum(map(len, groups)) == n
    run_lambda(ta, groups, t_u=3, nonuni=0)
    run_lambda(ta, groups, t_u=0, nonuni=0)
    run_lambda(ta, groups, t_u=0, nonuni=1)
    run_lambda(ta, groups, t_u=3, nonuni=None)
    run_lambda(ta, groups, mode=1, t_u=0, nonuni=None)  # Aggregate: lambda = 1 everywhere


@pytest.mark.parametrize("n, t", [(1, 1), (64, 2), (65, 1), (130, 2), (66, 3), (63, 7), (51, 17)])
def test_lambda_uniform_groups(ta, n, t):
    """n / t groups of t: nonuni stays as it was for t_u = t (from 0 and from 1), and is set for another t_u,
    for groups of 2 and 4 alternating, and for the same layout behind an empty first group"""
    rng = random.Random(600 + n)
    groups = [index_set(rng, t, g % 3) for g in range(n // t)]
    run_lambda(ta, groups, t_u=t, nonuni=0)
    run_lambda(ta, groups, t_u=t, nonuni=1)
    assert ta.layout(VB._offsets([t] * (n // t)), t, 0) == 0
    run_lambda(ta, groups, t_u=t + 1, nonuni=0)
    run_lambda(ta, [[]] + groups, t_u=t, nonuni=0)
    if t == 2:
        alt = [index_set(rng, 2 if g % 2 == 0 else 4, g % 3) for g in range(n // 3)]
        assert len(alt) < 2 or nonuni_expect(VB._offsets([len(g) for g in alt]), 3, 0, True) == 1
        run_lambda(ta, alt, t_u=3, nonuni=0)


# the denominators' table ends at |d| = 64 (consts.h FR_SMALL_INV_N); every pair meets both signs of d
EDGE_SETS = [[1, 64], [1, 65], [1, 66], [1, 67], [-30, 33, 34], [-30, 35, 36], [70, 6, 5, 135], [100, 36, 165, 35],
             [2 ** 62 - 1, 1, 2], [-(2 ** 62 - 1), 2 ** 62 - 1, 3], [-(2 ** 62 - 1), -(2 ** 62 - 1) + 64, 9],
             [2 ** 62, 5, 6], [-2 ** 62, -2 ** 62 + 1, 2 ** 62 - 1], [INT64_MAX, INT64_MIN, 1], [INT64_MAX, 1],
             [INT64_MIN, -1, 2], [INT64_MAX, INT64_MAX - 1, INT64_MIN, INT64_MIN + 1], list(range(1, 11)),
             [9, 3, 10, 1, 7, 4, 2, 8, 6, 5], [-1, -2, -3, -4, -5, 6, 7], list(range(1, 18)),
             [INT64_MAX - 3 * k for k in range(17)]]


def test_lambda_index_edges(ta):
    """the 1/d table's last entries and the first denominators past it (|d| = 63 / 64 / 65 / 66, both
    signs), the 2^62 guard on either index (+-(2^62 - 1) is inside it, 2^62 outside), INT64_MAX and
    INT64_MIN (one Fermat inversion; the reference reduces the true integers mod r), 17 members; and for
    each of divmod_xabs's three divisions a lambda whose running remainder reaches 2^63"""
    ds = {abs(a - b) for ids in EDGE_SETS for a in ids for b in ids}
    assert {63, 64, 65, 66} <= ds and ta.INV_N == 64
    rng = random.Random(700)
    found, groups = [False] * 3, list(EDGE_SETS)
    for ids in EDGE_SETS + [rng.sample(range(1, 30), 4) for _ in range(50)]:
        if all(found):
            break
        c = [divmod_crossings(lam) for lam in R.ta_lambda(ids)]
        new = [any(x[i] for x in c) for i in range(3)]
        if any(n and not f for n, f in zip(new, found)):
            found = [f or n for f, n in zip(found, new)]
            if ids not in groups:
                groups.append(ids)
    assert all(found), "the search found no remainder above 2^63 for some division"
    dig = run_lambda(ta, groups, t_u=0, nonuni=None)
    assert all(int(x) < Z for row in dig[:sum(map(len, groups))] for x in row)


def test_lambda_flags_and_skips(ta):
    """index 0 and duplicates: M_BAD_IDX on the members the rule names, M_BAD_SIG stays, flagged members
    get (1, 0, 0, 0); a skipped group keeps its sentinel digits and its statuses, whatever its indices"""
    groups = [[0, 1, 2], [1, 1, 2], [4, 5, 4, 0], [3, 9], [0, 0], [7], [0], [2, 3, 5], [6, 6, 6], [1, 2, 3, 4, 5, 6, 7],
              [5, INT64_MAX, 5], [0, INT64_MIN]]
    n = sum(map(len, groups))
    ms = [ta.M_BAD_SIG if j % 4 == 1 else ta.M_OK for j in range(n)]
    want = lambda_expect(ta, groups, 0, ms, None)[1]
    assert ta.M_BAD_IDX in want and ta.M_BAD_SIG in want and want[0] == ta.M_OK and want[1] == ta.M_BAD_SIG and want[2] == ta.M_BAD_IDX
    run_lambda(ta, groups, mstat=ms, nonuni=None)
    run_lambda(ta, groups, mode=1, mstat=ms, nonuni=None)
    skip = [1, 0, 1, 0, 0, 1, 0, 1, 1, 0, 0, 1]
    run_lambda(ta, groups, mstat=ms, skip=skip, nonuni=None)
    run_lambda(ta, groups, mstat=ms, skip=skip, t_u=3, nonuni=0)  # nonuni is decided before the skip


def test_member_status(ta):
    for n in (1, 64, 65, 130):
        rng = random.Random(n)
        sig_st = [rng.choice([0, 0, 2, 3, 255]) for _ in range(40)]
        src = [rng.randrange(40) for _ in range(n)]
        got = ta.member_status(sig_st, src, n + 3)
        assert [int(x) for x in got[:n]] == [ta.M_BAD_SIG if sig_st[s] else ta.M_OK for s in src] and untouched(got[n:])


def test_harness_refuses_indices_outside_its_buffers(ta, vw):
    pts = hm_rows(vw, vw.k[:4])
    dig = [[1, 0, 0, 0]] * 4
    ta.lam([1, 2, 3, 4], [0, 3, 2, 4], rc=DB_E_ARG)          # offsets not monotone
    ta.lam([1, 2, 3, 4], [1, 2, 4], rc=DB_E_ARG)             # not from 0
    ta.layout([0, 3, 2], 2, rc=DB_E_ARG)
    ta.member_status([0, 0], [0, 2], 2, rc=DB_E_ARG)         # no such signature
    ta.straus(pts, [0, 1, 2, 4], dig, 2, rc=DB_E_ARG)        # no such point
    ta.straus(pts, None, dig + dig, 2, rc=DB_E_ARG)          # more members than points
    ta.joint(pts, [0, 1, 2, 9], dig, 2, 2, 2, rc=DB_E_ARG)
    ta.joint(pts, None, dig, 2, 2, 9, rc=DB_E_ARG)           # c beyond TA_JOINT_MAX
    ta.joint(pts, None, dig, 4, 2, 2, rc=DB_E_ARG)           # more members than digits' buffer holds points for
    ta.small(pts, [0, 1, 2, 4], [1, 2, 1, 2], 2, 2, 0, rc=DB_E_ARG)
    w, a = sel_arrays(ta, SelCase(1, 2, 0, 0))
    a["key"] = _u32([ta.KEYS])
    ta.sel_fill(w, a, rc=DB_E_ARG)                           # no such class
    a["key"], a["off"] = _u32([0]), _u32([1] * (ta.KEYS + 1))
    ta.sel_fill(w, a, rc=DB_E_ARG)                           # a place beyond the groups
    z8 = np.zeros(2, np.uint8)
    ta.sel_scatter(2, _u32([0, 2]), z8, np.zeros(192, np.uint8), z8, np.zeros((2, 52), np.uint32), None, 1, np.zeros(192, np.uint8),
                   z8.copy(), None, None, np.zeros(4, np.uint64), rc=DB_E_ARG)


# ---- k_ta_straus --------------------------------------------------------------------------------
SPECIAL = [(0, 0, 0, 0), (1, 0, 0, 0), (Z - 1, 0, 0, 0), (0, Z - 1, 0, 0), (0, 0, Z - 1, 0), (0, 0, 0, Z - 1), (Z - 1,) * 4,
           (7, 8, 9, 15), (15, 9, 8, 7), (0x5555555555555555, 0xAAAAAAAAAAAAAAAA, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA),
           (0xAAAAAAAAAAAAAAAA, 0x5555555555555555, 0, 1), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (8, 0, 0, 7),
           (0x8000000000000000, 1 << 63, 9, Z - 2)]
assert all(d < Z for s in SPECIAL for d in s)


def straus_want(vw, dig, ks):
    """per member: the scalar of its output (0: infinity, for a member at infinity too)"""
    return [0 if k is None else R.ta_digit_scalar(d) * k % B.R for d, k in zip(dig, ks)]


def straus_setup(vw, n, n_groups, plain, shape_no, permute):
    """digits per LANE by wave kind (0 uniform special, 1 every lane its own special, 2 uniform random with
    one lane off, 3 uniform random), a member at infinity in every wave, points through src or in place"""
    rng = random.Random(800 + 7 * n + n_groups + shape_no)
    dig, ks = [None] * n, [None] * n
    for L in range(n):
        w, lane = divmod(L, 64)
        kind = (w + shape_no) % 4
        wr = random.Random(9000 + 64 * shape_no + w)
        uni = tuple(wr.randrange(Z) for _ in range(4))
        if kind == 0:
            d = SPECIAL[(3 * shape_no + w) % len(SPECIAL)]
        elif kind == 1:
            d = SPECIAL[lane % len(SPECIAL)]
        elif kind == 2:
            d = (uni[0], uni[1] ^ 1, uni[2], uni[3]) if lane == min(5, n - 64 * w - 1) and n - 64 * w > 1 else uni
        else:
            d = uni
        m = lane_member(L, n, n_groups, plain)
        dig[m] = list(d)
        ks[m] = None if lane == 9 else vw.k[(3 * L + shape_no) % 8]  # few distinct points: few reference products
    pos = list(range(n))
    if permute:
        rng.shuffle(pos)
        assert n < 3 or pos != list(range(n))
    rows = [None] * n
    for m in range(n):
        rows[pos[m]] = ks[m]
    return dig, ks, hm_rows(vw, rows), (pos if permute else None)


STRAUS_SHAPES = [(1, 1, None), (63, 21, None), (63, 63, None), (64, 32, None), (64, 1, None), (65, 13, None), (130, 65, None),
                 (130, 26, None), (65, 4, None), (130, 7, None), (130, 65, 1), (63, 21, 1), (64, 64, 1), (1, 1, 1)]


@pytest.mark.parametrize("shape_no", range(len(STRAUS_SHAPES)), ids=["%d-%d-%s" % s for s in STRAUS_SHAPES])
def test_straus_branches(ta, vw, shape_no):
    """every member's output is [(sum a_i z^i) k] Q whichever lane and branch computed it: without a guard
    and n a multiple of n_groups the lanes are share-position-major (t = 1 and n_groups = 1 among the
    shapes), otherwise plain; src null (even shapes) or a permutation (odd)"""
    n, ng, guard = STRAUS_SHAPES[shape_no]
    dig, ks, pts, src = straus_setup(vw, n, ng, guard is not None, shape_no, shape_no % 2 == 1)
    out = ta.straus(pts, src, dig, ng, guard=guard)
    check_rows(vw, out, straus_want(vw, dig, ks) + [None, None])


def test_straus_special_digits_on_the_naf_branch(ta, vw):
    """one wave of 64 equal digit vectors per special vector: zero and one, a single digit in each position,
    z - 1 in all four (the NAF's carry into position 64: the top must be found), 7 / 8 / 9 / 15 and the
    alternating words; lane 9 at infinity gives infinity"""
    for i, d in enumerate(SPECIAL):
        ks = [None if L == 9 else vw.k[L % 2] for L in range(64)]
        dig = [list(d)] * 64
        out = ta.straus(hm_rows(vw, ks), None, dig, 32 if i % 2 else 64, guard=None if i % 3 else 1, pad=1)
        check_rows(vw, out, straus_want(vw, dig, ks) + [None])


def test_straus_skips_and_the_first_valid_lane(ta, vw):
    """65 groups of 2, share-position-major: wave 0 is share 0 of validators 0..63, wave 1 validator 64 and
    share 1 of 0..62, wave 2 share 1 of 63 and 64.  With validators 0, 1, 2, 63, 64 skipped the first lanes
    of waves 0 and 1 are invalid (their digits, never computed in the product, differ from the wave's): the
    schedule must come from the first VALID lane; wave 2 is skipped whole.  Skipped members keep the
    sentinel.  Then the same with one valid lane off (general), with guard 1 (skip ignored, plain order)
    and with guard 0 (nothing written)"""
    n, ng, t = 130, 65, 2
    skip = [1 if v in (0, 1, 2, 63, 64) else 0 for v in range(ng)]
    rng = random.Random(810)
    uni = [[rng.randrange(Z) for _ in range(4)] for _ in range(3)]
    ks = [vw.k[m % 6] for m in range(n)]
    pts = hm_rows(vw, ks)
    for variant in ("uniform", "one_off"):
        dig = [None] * n
        for L in range(n):
            m = lane_member(L, n, ng, False)
            dig[m] = list(uni[L // 64])
            if skip[m // t]:
                dig[m] = [SENT64 - 1 - L, 3, 5, L]
            elif variant == "one_off" and L % 64 == 40:
                dig[m] = [dig[m][0] ^ 2] + dig[m][1:]
        want = [None if skip[m // t] else s for m, s in enumerate(straus_want(vw, dig, ks))]
        assert want[0] is None and want[1] is None and want[2 * 3] is not None and want[2 * 64 + 1] is None
        check_rows(vw, ta.straus(pts, None, dig, ng, skip=skip), want + [None, None])
    dig = [[d if d < Z else 11 for d in row] for row in dig]
    check_rows(vw, ta.straus(pts, None, dig, ng, skip=skip, guard=1), straus_want(vw, dig, ks) + [None, None])
    assert untouched(ta.straus(pts, None, dig, ng, skip=skip, guard=0))
    assert untouched(ta.straus(pts, None, dig, ng, guard=0))


# ---- launch_ta_joint ----------------------------------------------------------------------------
JOINT_SHAPES = [(1, 2, 2), (64, 4, 2), (65, 4, 2), (33, 5, 2), (64, 5, 2), (64, 8, 8), (70, 7, 3), (64, 17, 8)]


def joint_sets(ng, t, mixed, seed):
    """one index set per validator: the same shuffled 1..t + 2 subset for all, or (mixed) every third
    validator on a set of its own"""
    rng = random.Random(seed)
    shared = rng.sample(range(1, t + 3), t)
    return [rng.sample(range(1, t + 9), t) if mixed and v % 3 == 1 else shared for v in range(ng)]


def joint_digits(sets):
    return [R.ta_digits(lam) for ids in sets for lam in R.ta_lambda(ids)]


def joint_want(sets, ks, t, c, skip=None):
    """per member slot: the chunk's sum [sum lambda_j k_j] Q at the chunk's first member, infinity at its
    others; None (the sentinel) for skipped groups"""
    want = []
    for v, ids in enumerate(sets):
        lam = R.ta_lambda(ids)
        for j0 in range(0, t, c):
            js = range(j0, min(t, j0 + c))
            s = sum(lam[j] * ks[v * t + j] for j in js if ks[v * t + j] is not None) % B.R
            want += [None] * len(js) if skip is not None and skip[v] else [s] + [0] * (len(js) - 1)
    return want


def group_sums(out, ng, t):
    """what k_group_sum adds: the t slots of each group"""
    sums = []
    for v in range(ng):
        acc = None
        for j in range(t):
            acc = B.g2_add(acc, elem(out[v * t + j]))
        sums.append(acc)
    return sums


def uniform_waves(sets, t, c, skip=None):
    """joint_lane's rule restated for the branch table: per wave, do the valid lanes agree in cnt and digits?"""
    ng = len(sets)
    n_chunks = (t + c - 1) // c
    out = []
    for w0 in range(0, ng * n_chunks, 64):
        keys = set()
        for L in range(w0, min(w0 + 64, ng * n_chunks)):
            q, v = divmod(L, ng)
            if skip is None or not skip[v]:
                lam = R.ta_lambda(sets[v])
                keys.add(tuple(lam[q * c:min(t, q * c + c)]))
        out.append(len(keys) == 1 if keys else None)
    return out


JOINT_UNIFORM = {(1, 2, 2): [True], (64, 4, 2): [True, True], (65, 4, 2): [True, False, True], (33, 5, 2): [False, False],
                 (64, 5, 2): [True] * 3, (64, 8, 8): [True], (70, 7, 3): [True, False, False, True], (64, 17, 8): [True] * 3}


@pytest.mark.parametrize("mixed", [False, True], ids=["shared", "own"])
@pytest.mark.parametrize("shape", JOINT_SHAPES, ids=["%d-%d-%d" % s for s in JOINT_SHAPES])
def test_joint_shapes(ta, vw, shape, mixed):
    """digits from ta_lambda of one shared index set (the waves of JOINT_UNIFORM run k_ta_jtab +
    k_ta_jladder, the others -- a wave over two chunk positions, cnt 2 and 1 side by side -- k_ta_jgeneral)
    and of per-validator sets (k_ta_jgeneral throughout); every validator has distinct points, through a
    src permutation for the shared sets.  Every chunk's sum at its first member and infinity at the others;
    the t slots of a group add up to [sum lambda_j k_j] Q"""
    ng, t, c = shape
    sets = joint_sets(ng, t, mixed, 900 + ng + t)
    uni = uniform_waves(sets, t, c)
    assert uni == (JOINT_UNIFORM[shape] if not mixed else [False] * len(uni)) or (mixed and ng == 1)
    ks = [vw.k[(v * t + j) % 48] for v in range(ng) for j in range(t)]
    n = ng * t
    pos = list(range(n))
    if not mixed and n > 2:
        random.Random(shape[0]).shuffle(pos)
    rows = [None] * n
    for m in range(n):
        rows[pos[m]] = ks[m]
    out = ta.joint(hm_rows(vw, rows), None if mixed or n <= 2 else pos, joint_digits(sets), ng, t, c)
    check_rows(vw, out, joint_want(sets, ks, t, c) + [None, None])
    if ng <= 33:
        for v, got in enumerate(group_sums(out, ng, t)):
            lam = R.ta_lambda(sets[v])
            assert got == vw.f2.mul(sum(lam[j] * ks[v * t + j] for j in range(t)))


@pytest.mark.parametrize("shape, skipped", [((64, 4, 2), [0, 5, 63]), ((65, 4, 2), [0, 3, 64]), ((64, 8, 8), [0, 1, 63]),
                                            ((128, 2, 2), [0, 5] + list(range(64, 128))), ((70, 7, 3), [0, 69, 33])],
                         ids=["64-4-2", "65-4-2", "64-8-8", "128-2-2", "70-7-3"])
def test_joint_skip(ta, vw, shape, skipped):
    """skipped groups (lane 0 of a wave among them; in 128-2-2 the whole second wave): their digits are
    never computed in the product -- here they hold another validator set's values, so a schedule taken from
    a skipped lane shows -- and nothing is written to their slots"""
    ng, t, c = shape
    skip = [1 if v in skipped else 0 for v in range(ng)]
    sets = joint_sets(ng, t, False, 950 + ng)
    other = random.Random(951).sample(range(20, 40), t)
    dig_sets = [other if skip[v] else sets[v] for v in range(ng)]
    ks = [vw.k[(v * t + j) % 48] for v in range(ng) for j in range(t)]
    assert True in uniform_waves(sets, t, c, skip)
    out = ta.joint(hm_rows(vw, ks), None, joint_digits(dig_sets), ng, t, c, skip=skip)
    want = joint_want(sets, ks, t, c, skip)
    assert want[0] is None and any(w is not None for w in want)
    check_rows(vw, out, want + [None, None])


def test_joint_nonuni_then_the_guarded_ladders(ta, vw):
    """nonuni = 1: launch_ta_joint writes nothing at all; the guarded launch_ta_straus the product issues
    behind it fills the same buffer, and the groups' sums are right.  nonuni = 0 behaves as no pointer"""
    ng, t, c = 20, 4, 2
    sets = joint_sets(ng, t, True, 960)
    ks = [vw.k[(v * t + j) % 48] for v in range(ng) for j in range(t)]
    pts, dig = hm_rows(vw, ks), joint_digits(sets)
    out = ta.joint(pts, None, dig, ng, t, c, nonuni=1)
    assert untouched(out)
    out = ta.straus(pts, None, dig, ng, guard=1, out=out)
    lam = [x for ids in sets for x in R.ta_lambda(ids)]
    check_rows(vw, out, [lam[m] * ks[m] % B.R for m in range(ng * t)] + [None, None])
    for v, got in enumerate(group_sums(out, ng, t)):
        assert got == vw.f2.mul(sum(lam[v * t + j] * ks[v * t + j] for j in range(t)))
    check_rows(vw, ta.joint(pts, None, dig, ng, t, c, nonuni=0), joint_want(sets, ks, t, c) + [None, None])


@pytest.mark.parametrize("c", [3, 2])
def test_joint_degenerate_members_in_a_uniform_chunk(ta, vw, c):
    """one uniform wave over the index set (1, 2, 3), lambda = (3, -3, 1): two members holding the same
    point (jac_add_aff meets R = T), sigma and -sigma, and (S, 2S, 3S), whose combination vanishes; c = 3
    one chunk, c = 2 chunks of 2 and 1 in two uniform waves"""
    ids = [1, 2, 3]
    assert R.ta_lambda(ids) == [3, B.R - 3, 1]
    a, b, s = vw.k[0], vw.k[1], vw.k[2]
    per = [[a, a, b], [a, B.R - a, b], [s, 2 * s % B.R, 3 * s % B.R], [b, b, b], [a, b, B.R - a], [a, 2 * a % B.R, b], [a, b, s]]
    ng = len(per) if c == 3 else 64  # 64 validators: each chunk position fills a wave of its own
    ks = [k for v in range(ng) for k in per[v % len(per)]]
    sets = [ids] * ng
    assert uniform_waves(sets, 3, c) == [True] * (1 if c == 3 else 2)
    out = ta.joint(hm_rows(vw, ks), None, joint_digits(sets), ng, 3, c)
    check_rows(vw, out, joint_want(sets, ks, 3, c) + [None, None])
    sums = group_sums(out, len(per), 3)
    assert sums[2] is None and sums[6] == vw.f2.mul(3 * a - 3 * b + s)


@pytest.mark.parametrize("t, c", [(3, 3), (5, 2)])
def test_joint_infinite_member(ta, vw, t, c):
    """a member at infinity inside a uniform chunk (t = c = 3: one wave; t = 5, c = 2: three uniform waves,
    the member in the middle one): that lane's sum is unspecified (see the module docstring) and is the one
    value not asserted -- the lane wrote its own cnt slots (no sentinel left, the slots behind the first hold
    infinity), every other lane of the wave is exact and nothing else is touched.  With one validator on
    another index set the waves take k_ta_jgeneral, where the same input is exact: the infinite member adds
    nothing"""
    ng = 64 if c < t else 6
    at = 2 * t + (1 if c == t else 3)  # validator 2; with c = 2 its chunk (2, 3), second slot
    ks = [vw.k[(v * t + j) % 48] for v in range(ng) for j in range(t)]
    ks[at] = None
    first = at - (at - 2 * t) % c
    sets = joint_sets(ng, t, False, 971)
    assert all(uniform_waves(sets, t, c))
    out = ta.joint(hm_rows(vw, ks), None, joint_digits(sets), ng, t, c)
    want = joint_want(sets, ks, t, c)
    for m in range(ng * t):
        if m == first:
            assert not untouched(out[m])
            elem(out[m])  # below 2p; the element itself is the unspecified one
        else:
            assert elem(out[m]) == vw.f2.mul(want[m]), m
    assert untouched(out[ng * t:])
    sets = [rs if v % 7 else [9, 4, 11, 2, 30][:t] for v, rs in enumerate(sets)]  # no wave uniform: k_ta_jgeneral, exact
    assert not any(uniform_waves(sets, t, c))
    out = ta.joint(hm_rows(vw, ks), None, joint_digits(sets), ng, t, c)
    check_rows(vw, out, joint_want(sets, ks, t, c) + [None, None])


# ---- k_ta_sprep and launch_ta_small -------------------------------------------------------------
def small_expect(sets, ks, t):
    """-> (csm rows, sdig rows, sok, done, out scalars) by ta_small.h's rule and k_ta_small's: a wave of 64
    validators runs when every split was taken and (c, s) agree; done = 2 where Q = sum c_j sigma_j vanishes"""
    sp = [R.ta_small_split(ids) if len(ids) == t else None for ids in sets]
    csm = [list(s[0]) if s else [0] * t for s in sp]
    sdig = [R.ta_digits(s[1]) if s else [0] * 4 for s in sp]
    sok = [1 if s else 0 for s in sp]
    done, out = [], []
    for w0 in range(0, len(sets), 64):
        vs = range(w0, min(w0 + 64, len(sets)))
        uniform = all(sp[v] is not None and sp[v] == sp[w0] for v in vs)
        for v in vs:
            if not uniform:
                done.append(0)
                out += [None] * t
                continue
            q = sum(cj * ks[v * t + j] for j, cj in enumerate(sp[v][0]) if ks[v * t + j] is not None) % B.R
            done.append(1 if q else 2)
            out += [sp[v][1] * q % B.R] + [0] * (t - 1)
    return csm, sdig, sok, done, out


def check_small(ta, vw, sets, ks, t, pair, src=None, pts=None):
    ng = len(sets)
    idx = [x for ids in sets for x in ids]
    got = ta.small(hm_rows(vw, ks) if pts is None else pts, src, idx, ng, t, pair)
    csm, sdig, sok, done, out = small_expect(sets, ks, t)
    assert got["csm"].tolist() == csm and got["sdig"].tolist() == sdig and got["sok"].tolist() == sok
    assert got["done"].tolist() == done
    check_rows(vw, got["out"], out + [None, None])
    return got


@pytest.mark.parametrize("pair", [0, 1])
@pytest.mark.parametrize("t", [2, 3, 7, 16])
@pytest.mark.parametrize("ng", [1, 32, 33, 64, 65, 100])
def test_small_uniform(ta, vw, ng, t, pair):
    """every validator on one index set: csm, sdig, sok equal ta_small_split, done = 1 everywhere, the
    sum [s sum c_j k_j] Q at the group's first member and infinity at the others; lane pairs at 33 and 65
    validators leave a half-filled wave"""
    ids = random.Random(1000 + t).sample(range(1, min(t + 3, 17)), t)  # 16 members: the cluster 1..16, shuffled
    assert R.ta_small_split(ids) is not None
    sets = [ids] * ng
    ks = [vw.k[((v % 4) * t + j) % 48] for v in range(ng) for j in range(t)]
    got = check_small(ta, vw, sets, ks, t, pair)
    assert got["done"].tolist() == [1] * ng
    csm, sdig, sok = ta.sprep([x for s in sets for x in s], ng, t)
    assert (csm == got["csm"]).all() and (sdig == got["sdig"]).all() and (sok == got["sok"]).all()


@pytest.mark.parametrize("pair", [0, 1])
def test_small_wave_patterns(ta, vw, pair):
    """100 validators of 3: wave 0 uniform and wave 1 with one validator on another index set; then wave 0
    holding one refused group (an index of 2^31) and wave 1 uniform; then a shuffled set (other c_j) in
    wave 0.  done = 0 for the whole of such a wave and out untouched there"""
    t, ng = 3, 100
    ks = [vw.k[((v % 5) * t + j) % 48] for v in range(ng) for j in range(t)]
    base = [2, 5, 3]
    for odd_at, odd in ((80, [2, 5, 4]), (17, [2, 5, 2 ** 31]), (0, [5, 2, 3]), (99, [0, 5, 3]), (63, [2, 2, 3])):
        sets = [odd if v == odd_at else base for v in range(ng)]
        got = check_small(ta, vw, sets, ks, t, pair)
        w = odd_at // 64
        assert got["done"].tolist() == [0 if v // 64 == w else 1 for v in range(ng)]


def test_sprep_refusals(ta):
    """the split per group, without the ladders: taken and refused sets side by side (index 0, duplicates,
    2^31 and -2^31, E_j = -2^63, a product beyond 63 bits): sok = 0 and csm = 0 for the refused ones.  t = 17
    and nonuni = 1: sok = 0 everywhere, sdig zero, csm untouched.  t = 1: sok = 0 everywhere; the kernel
    treats the group as any refused set and writes csm = 0 (t = 1 is within TA_SMALL_MAX, so the kernel
    looks at it; no later kernel reads csm when t < 2)"""
    edge = [-2 ** 30, 2 ** 30, -2 ** 30 + 1, -2 ** 30 + 4]
    sets4 = [[1, 2, 3, 4], [0, 1, 2, 3], [1, 2, 2, 4], [1, 2, 3, 2 ** 31], [1, -2 ** 31, 3, 4], edge, [2 ** 31 - 1, -2 ** 31 + 1, 5, 9],
             [4, 3, 2, 1], [-1, -2, -3, -4], [1, 2, 3, 2 ** 31 - 1], [10, 20, 30, 40]] * 7
    assert len(sets4) == 77
    exp = small_expect(sets4, [1] * (4 * 77), 4)
    assert exp[2][:11] == [1, 0, 0, 0, 0, 0, 0, 1, 1, 0, 1]  # 2^31 - 1 is an index the header looks at; its E_j overflows
    csm, sdig, sok = ta.sprep([x for s in sets4 for x in s], 77, 4)
    assert csm.tolist() == exp[0] and sdig.tolist() == exp[1] and sok.tolist() == exp[2]
    for ng in (1, 65):
        for t, nonuni in ((17, None), (17, 0), (3, 1), (16, 1)):
            csm, sdig, sok = ta.sprep(list(range(1, t + 1)) * ng, ng, t, nonuni=nonuni)
            assert (csm == SENTI).all() and (sdig == 0).all() and (sok == 0).all(), (ng, t, nonuni)
        csm, sdig, sok = ta.sprep([5] * ng, ng, 1)
        assert (csm == 0).all() and (sdig == 0).all() and (sok == 0).all()
        csm, sdig, sok = ta.sprep(list(range(1, 4)) * ng, ng, 3, nonuni=0)  # nonuni = 0 is no refusal
        assert sok.tolist() == [1] * ng


@pytest.mark.parametrize("pair", [0, 1])
def test_small_stands_down(ta, vw, pair):
    """t = 1, t = 17 and nonuni = 1 through the whole launcher: sok = 0 and done = 0 everywhere, out untouched"""
    for ng, t, nonuni in ((3, 1, None), (65, 17, None), (65, 3, 1)):
        ks = [vw.k[(v * t + j) % 48] for v in range(ng) for j in range(t)]
        got = ta.small(hm_rows(vw, ks), None, list(range(1, t + 1)) * ng, ng, t, pair, nonuni=nonuni)
        assert (got["sok"] == 0).all() and (got["done"] == 0).all() and untouched(got["out"]) and (got["sdig"] == 0).all()
        assert (got["csm"] == (0 if t == 1 else SENTI)).all()


@pytest.mark.parametrize("pair", [0, 1])
@pytest.mark.parametrize("ids", [[1, 2], [1, 2, 3]], ids=["1-2", "1-2-3"])
def test_small_degenerate_members(ta, vw, ids, pair):
    """one uniform wave (40 validators; with lane pairs two waves of the ladder): members at infinity are
    skipped exactly; (S, 2S) under (1, 2) and (S, 2S, 3S) under (1, 2, 3) give Q = infinity: done = 2 and
    infinity out on that lane, its neighbours exact; equal and opposite members (g2l_madd's doubling branch
    and its infinity), through a src permutation"""
    t, ng = len(ids), 40
    c = R.ta_small_split(ids)[0]
    assert c == ([2, -1] if t == 2 else [3, -3, 1])
    a, b, s = vw.k[0], vw.k[1], vw.k[2]
    ks = [vw.k[((v % 5) * t + j) % 48] for v in range(ng) for j in range(t)]
    vanish = [s * (j + 1) % B.R for j in range(t)]
    special = {0: vanish, 7: [a] * t, 8: [a, B.R - a, b][:t], 13: [None] + [b] * (t - 1), 14: [a] * (t - 1) + [None],
               21: [None] * t, 31: vanish, 32: [b, a, a][:t], 39: vanish}
    for v, row in special.items():
        ks[v * t:v * t + t] = row
    pos = list(range(ng * t))
    random.Random(1100 + t).shuffle(pos)
    rows = [None] * (ng * t)
    for m in range(ng * t):
        rows[pos[m]] = ks[m]
    got = check_small(ta, vw, [ids] * ng, ks, t, pair, src=pos, pts=hm_rows(vw, rows))
    done = got["done"].tolist()
    assert [v for v in range(ng) if done[v] == 2] == ([0, 14, 21, 31, 39] if t == 3 else [0, 21, 31, 39])  # 3a - 3a at 14
    assert all(d in (1, 2) for d in done)


@pytest.mark.parametrize("ng, t", [(33, 3), (65, 7), (100, 2)])
def test_small_pair_settings_agree(ta, vw, ng, t):
    """the two settings of g_ta_pair_max give identical group elements (and identical csm / sdig / done)"""
    ids = random.Random(1200 + t).sample(range(1, t + 3), t)
    sets = [ids if v != 70 else ids[::-1] for v in range(ng)]
    ks = [vw.k[((v % 4) * t + j) % 48] for v in range(ng) for j in range(t)]
    pts, idx = hm_rows(vw, ks), [x for s in sets for x in s]
    g0, g1 = ta.small(pts, None, idx, ng, t, 0), ta.small(pts, None, idx, ng, t, 1)
    for k in ("csm", "sdig", "sok", "done"):
        assert (g0[k] == g1[k]).all(), k
    for m in range(ng * t + 2):
        if untouched(g0["out"][m]):
            assert untouched(g1["out"][m]), m
        else:
            assert elem(g0["out"][m]) == elem(g1["out"][m]), m


# ---- the selection kernels ----------------------------------------------------------------------
class SelCase:
    """n_groups groups of candidates in eight kinds by g % 8: exactly t verified; more than t, the first
    failed (shifted); more than t, all good; fewer than t verified; mixed messages; no candidates; a repeated
    share index (and a candidate naming no partial); t good behind a failed one on another message.  The
    offsets of the last `cut` groups reach beyond n_cand.  Every candidate names a partial of its own
    (shuffled), plus some partials nobody names"""

    def __init__(self, ng, t, mode, cut, seed=0):
        rng = random.Random(1300 + 10 * ng + t + seed)
        self.ng, self.t, self.mode = ng, t, mode
        cands = []  # per group: [(ok, share index, message)]
        for g in range(ng):
            kind, m = g % 8, 1 + g % 3
            if kind == 0:
                c = [(1, k + 1, m) for k in range(t)]
            elif kind == 1:
                c = [(0, 1, m)] + [(1, k + 2, m) for k in range(t + 1)]
            elif kind == 2:
                c = [(1, k + 1, m) for k in range(t + 2)]
            elif kind == 3:
                c = [(1 if k < t - 1 else 0, k + 1, m) for k in range(t + 1)]
            elif kind == 4:
                c = [(1, k + 1, m + (k == 1)) for k in range(t + 1)] + [(1, t + 2 + k, m + 1) for k in range(t - 1)]
            elif kind == 5:
                c = []
            elif kind == 6:
                c = [(1, 1, m), (1, 1, m), (2, 9, m)] + [(1, k + 2, m) for k in range(t)]
            else:
                c = [(0, 1, m + 1)] + [(1, k + 2, m) for k in range(t)]
            cands.append(c)
        flat = [x for c in cands for x in c]
        n = len(flat) + 5
        order = list(range(n))
        rng.shuffle(order)
        self.vstatus, self.msg_idx = [3] * n, [rng.randrange(4) for _ in range(n)]
        self.src, self.idx = [], []
        for j, (ok, x, m) in enumerate(flat):
            p = order[j]
            self.src.append(n + 4 if ok == 2 else p)
            self.idx.append(x)
            self.vstatus[p], self.msg_idx[p] = (0 if ok else rng.choice([1, 2, 3])), m
        if not flat:
            self.src, self.idx = [0], [1]
        self.off = VB._offsets([len(c) for c in cands])
        self.n, self.n_cand = n, len(self.src)
        if cut:  # the offsets go on as if the last groups' candidates existed; the arrays end before them
            self.n_cand = max(1, self.off[ng - cut] + 1)
        self.model()

    def model(self):
        t, n = self.t, self.n
        self.exp = []
        for g in range(self.ng):
            b = min(self.off[g], self.n_cand)
            e = min(max(self.off[g + 1], b), self.n_cand)
            cand = [(self.src[j], self.idx[j]) for j in range(b, e)]
            msgs = [self.msg_idx[p] for p, _ in cand if p < n]
            if self.mode == HS.FIRST:
                mem, pos = TS.rule(self.vstatus, cand, t)
                state = TS.ST_MIXED if len(set(msgs)) > 1 else TS.ST_FEW if len(mem) < t else TS.ST_OK
                key = 0
                for k in pos:
                    key ^= 1 << (k & 15)
                r = dict(chosen=mem + [TS.NONE] * (t - len(mem)), cidx=[cand[k][1] for k in pos] + [0] * (t - len(mem)),
                         count=len(mem), key=key if state == TS.ST_OK else HS.KEY_NONE, state=state,
                         shifted=int(len(mem) == t and pos[-1] != t - 1), msg=msgs[0] if msgs else 0)
            else:
                r = HS.expect(self.vstatus, self.msg_idx, cand, t)
                r["msg"] = r["root"] if r["root"] is not None else (msgs[0] if msgs else 0)
            self.exp.append(r)


def sel_arrays(ta, sc, ctr0=(0, 0, 0, 0)):
    ng, t = sc.ng, sc.t
    w = dict(n=sc.n, n_cand=sc.n_cand, n_groups=ng, t=t, mode=sc.mode)
    a = dict(vstatus=_u8(sc.vstatus), msg_idx=_u32(sc.msg_idx), src=_u32(sc.src[:sc.n_cand]), idx=_i64(sc.idx[:sc.n_cand]),
             grp_off=_u32(sc.off), chosen=VB._sent32(ng * t), cidx=np.full(ng * t, SENTI, np.int64), ta_count=VB._sent32(ng),
             key=VB._sent32(ng), state=VB._sent8(ng), gmsg=VB._sent32(ng), hist=np.zeros(ta.KEYS, np.uint32),
             off=np.zeros(ta.KEYS + 1, np.uint32), cur=np.zeros(ta.KEYS, np.uint32), perm=VB._sent32(ng), pmem=VB._sent32(ng * t),
             pgoff=VB._sent32(ng + 1), pidx=np.full(ng * t, SENTI, np.int64), ctr=np.array(ctr0, dtype=np.uint64))
    return w, a


SEL_SHAPES = [(1, 2), (64, 2), (64, 4), (65, 4), (130, 2), (130, 4)]


@pytest.mark.parametrize("mode", [0, 1], ids=["first", "matching"])
@pytest.mark.parametrize("ng, t", SEL_SHAPES)
def test_select(ta, ng, t, mode):
    """chosen / cidx / ta_count / key / state / gmsg equal the rule's (tests/test_tasel_host.py rule() for
    the first-t mode, tests/test_hslot.py matching() for the matching mode); hist is the exact histogram of
    the keys; the three counters advance by the exact counts from a non-zero start and SEL_SMALL stays"""
    for cut in (0, 3):
        sc = SelCase(ng, t, mode, min(cut, ng - 1) if ng > 1 else 0)
        start = [5, 1 << 40, 77, 9]
        w, a = sel_arrays(ta, sc, start)
        ta.select(w, a)
        e = sc.exp
        assert a["chosen"].reshape(ng, t).tolist() == [r["chosen"] for r in e]
        assert a["cidx"].reshape(ng, t).tolist() == [r["cidx"] for r in e]
        assert a["ta_count"].tolist() == [r["count"] for r in e] and a["key"].tolist() == [r["key"] for r in e]
        assert a["state"].tolist() == [r["state"] for r in e] and a["gmsg"].tolist() == [r["msg"] for r in e]
        hist = np.bincount([r["key"] for r in e], minlength=ta.KEYS)
        assert (a["hist"] == hist).all()
        want = list(start)
        want[ta.SEL_SEEN] += ng
        want[ta.SEL_FEW] += sum(r["state"] == ta.FEW for r in e)
        want[ta.SEL_SHIFTED] += sum(r["shifted"] for r in e)
        assert a["ctr"].tolist() == want
        if ng >= 64 and not cut:
            states, n_keys = {r["state"] for r in e}, len({r["key"] for r in e})
            assert states == ({0, 1, 2} if mode == 0 else {0, 1}) and n_keys >= 4 and any(r["shifted"] for r in e)


@pytest.mark.parametrize("mode", [0, 1], ids=["first", "matching"])
@pytest.mark.parametrize("ng, t", SEL_SHAPES)
def test_sel_fill(ta, ng, t, mode):
    """class order from the rule's keys and the exclusive scan of their histogram.  The order inside a class
    is decided by atomics, so: perm is a permutation; the places [off[k], off[k + 1]) hold exactly the groups
    of key k; pgoff[p] = p t with the final entry; pmem / pidx of place p are group perm[p]'s members, or
    (0, 1..t) for a group without an aggregate; cur ends as the histogram"""
    sc = SelCase(ng, t, mode, 0, seed=1)
    e = sc.exp
    w, a = sel_arrays(ta, sc)
    a["chosen"] = _u32([x for r in e for x in r["chosen"]])
    a["cidx"] = _i64([x for r in e for x in r["cidx"]])
    a["key"], a["state"] = _u32([r["key"] for r in e]), _u8([r["state"] for r in e])
    hist = np.bincount([r["key"] for r in e], minlength=ta.KEYS)
    off = np.concatenate([[0], np.cumsum(hist)]).astype(np.uint32)
    a["off"] = off
    ta.sel_fill(w, a)
    perm = a["perm"].tolist()
    assert sorted(perm) == list(range(ng))
    for p, g in enumerate(perm):
        k = e[g]["key"]
        assert off[k] <= p < off[k + 1], (p, g)
        ok = e[g]["state"] == ta.OK
        assert a["pmem"][p * t:p * t + t].tolist() == (e[g]["chosen"] if ok else [0] * t)
        assert a["pidx"][p * t:p * t + t].tolist() == (e[g]["cidx"] if ok else list(range(1, t + 1)))
    assert a["pgoff"].tolist() == [p * t for p in range(ng + 1)]
    assert (a["cur"] == hist).all()


@pytest.mark.parametrize("rows16", [1, 0])
@pytest.mark.parametrize("ng", [1, 64, 65, 130])
def test_sel_scatter(ta, ng, rows16):
    """rows, statuses and points land in the caller's order; groups without an aggregate get zero rows and
    ST_UNCHECKED (too few) / ST_BAD_INPUT (mixed) and keep their agg_pt; SEL_SMALL counts the aggregated
    groups the small-scalar path took, the other counters stay; perm null: no group has an aggregate; the
    optional agg_pt / agg_st / sdone null and given"""
    rng = random.Random(1400 + ng)
    state = [rng.choice([ta.OK, ta.OK, ta.FEW, ta.MIXED]) for _ in range(ng)]
    perm = list(range(ng))
    rng.shuffle(perm)
    pout = np.frombuffer(rng.randbytes(96 * ng), dtype=np.uint8).copy()
    pstatus = [rng.choice([ta.ST_OK, ta.ST_OK, ta.ST_COMBINE, B.ST_BAD_SIGNATURE]) for _ in range(ng)]
    ppt = np.array([[rng.getrandbits(32) for _ in range(52)] for _ in range(ng)], dtype=np.uint32)
    sdone = [rng.choice([0, 1, 2]) for _ in range(ng)]
    for use_perm, opt in ((True, True), (True, False), (False, True)):
        ta_out, ta_status = VB._sent8(96 * ng), VB._sent8(ng)
        agg_pt, agg_st = (VB._sent32(ng, 52), VB._sent8(ng)) if opt else (None, None)
        ctr = np.array([11, 22, 33, 44], dtype=np.uint64)
        ta.sel_scatter(ng, _u32(perm) if use_perm else None, _u8(state), pout, _u8(pstatus), ppt, _u8(sdone) if opt else None,
                       rows16, ta_out, ta_status, agg_pt, agg_st, ctr)
        small = 0
        for p in range(ng):
            g = perm[p] if use_perm else p
            have = use_perm and state[g] == ta.OK
            st = pstatus[p] if have else ta.ST_BAD_INPUT if state[g] == ta.MIXED else ta.ST_UNCHECKED
            assert ta_status[g] == st
            assert (ta_out[96 * g:96 * g + 96] == (pout[96 * p:96 * p + 96] if have else 0)).all()
            if opt:
                assert agg_st[g] == (st != ta.ST_OK)
                assert (agg_pt[g] == ppt[p]).all() if have else untouched(agg_pt[g])
                small += have and sdone[p] != 0
        want = [11, 22, 33, 44]
        want[ta.SEL_SMALL] += small
        assert ctr.tolist() == want


def test_sel_verdicts(ta):
    for ng in (1, 64, 65, 130):
        rng = random.Random(1500 + ng)
        st = [rng.choice([ta.ST_OK, ta.ST_OK, ta.ST_UNCHECKED, ta.ST_BAD_INPUT, ta.ST_COMBINE]) for _ in range(ng)]
        agg = np.array([rng.choice([0, 3, SENT8]) for _ in range(ng)] + [SENT8] * 3, dtype=np.uint8)
        before = agg.copy()
        ta.sel_verdicts(st, agg)
        assert agg[:ng].tolist() == [int(before[g]) if st[g] == ta.ST_OK else st[g] for g in range(ng)] and untouched(agg[ng:])
