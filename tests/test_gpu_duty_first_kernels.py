"""The kernels of the segmented first-error verification on the GPU, one launcher at a time, through the
device harness tests/native/dutyfirstdev.hip (which compiles the product's charon_amd/csrc/dutyfirst.hip):
k_seg_first_batch + k_seg_batch_verdict, k_seg_first_group, k_seg_scatter and k_seg_first_item on explicit
bytes against the rule of charon_amd/csrc/dutyfirst.h restated in Python, exactly.  Every output array
carries sentinel entries behind it, and what a kernel must leave alone is preset and compared as well.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
PAD = 8
S8, S32 = 0xA5, 0xA5A5A5A5
KEEP = 0x5A  # preset of a verdict the kernel must not write (a listed group's, decided by its own check later)
READY = 0
PASS, FAILED, GV_UNCHECKED, NOT_READY = 0, 3, 0x80, 0x81
OK, BAD_PUBKEY, BAD_SIGNATURE, NOT_VERIFIED, UNCHECKED = 0, 1, 2, 3, 7


@pytest.fixture(scope="module")
def D(hipbls):
    from gpu_helpers import harness
    lib = harness.load("dutyfirstdev")
    I, V = ctypes.c_int, ctypes.c_void_p
    lib.dfd_batch_verdict.argtypes = [I, V, V, I, I, I, V, I, I, V, V, V, V]
    lib.dfd_first_group.argtypes = [I, V, V, I, I, V]
    lib.dfd_scatter.argtypes = [I, V, V, I, V, V, V, V, V, I, V, V, V, I, V, I, V, V, V]
    lib.dfd_first_item.argtypes = [I, V, V, V, I, I, V]
    return lib


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def u8(x):
    return np.ascontiguousarray(x, dtype=np.uint8)


def u32(x):
    return np.ascontiguousarray(x, dtype=np.uint32)


def segs(off):
    """contiguous segments over group (or item) positions: segment k is positions off[k] .. off[k + 1] - 1"""
    return np.repeat(np.arange(len(off) - 1), np.diff(off)).astype(np.uint32)


# ---------------------------------------------------------------------------------------------
# k_seg_first_batch + k_seg_batch_verdict
# ---------------------------------------------------------------------------------------------
def model_batch_verdict(gst, bver, guard, fb, g0, gseg, n_seg, sf0):
    ng, sf = len(gst), list(sf0)
    gver, lst = [KEEP] * ng, []
    if guard == 0:
        return gver, lst, sf
    key = lambda lg: g0 + lg // fb * fb  # noqa: E731
    seg = lambda lg: int(gseg[g0 + lg])  # noqa: E731
    head = lambda lg: int(gseg[key(lg)]) != seg(lg)  # noqa: E731 -- the batch begins with an earlier segment's group
    for lg in range(ng):
        if gst[lg] == READY and bver[lg // fb] and seg(lg) < n_seg and not head(lg):
            sf[2 * seg(lg)] = min(sf[2 * seg(lg)], key(lg))
    for lg in range(ng):
        if gst[lg] != READY:
            gver[lg] = NOT_READY
        elif not bver[lg // fb]:
            gver[lg] = PASS
        elif seg(lg) < n_seg and (head(lg) or sf[2 * seg(lg)] == key(lg)):
            lst.append(lg)
        else:
            gver[lg] = GV_UNCHECKED
    return gver, lst, sf


def run_batch_verdict(D, gst, bver, fb, gseg, n_seg, g0=0, guard=-1, sf0=None, what=""):
    gst, bver, gseg, ng = u8(gst), u8(bver), u32(gseg), len(gst)
    assert len(gseg) == g0 + ng and len(bver) == (ng + fb - 1) // fb
    sf0 = [NONE] * (2 * n_seg) if sf0 is None else list(sf0)
    gver = np.concatenate([np.full(ng, KEEP, np.uint8), np.full(PAD, S8, np.uint8)])
    lst, cnt = np.full(ng + PAD, S32, np.uint32), np.concatenate([np.zeros(1, np.uint32), np.full(PAD, S32, np.uint32)])
    sf = np.concatenate([u32(sf0), np.full(PAD, S32, np.uint32)])
    assert D.dfd_batch_verdict(ng, _p(gst), _p(bver), guard, fb, g0, _p(gseg), n_seg, PAD, _p(gver), _p(lst), _p(cnt), _p(sf)) == 0
    want = model_batch_verdict(gst, bver, guard, fb, g0, gseg, n_seg, sf0)
    assert (gver[ng:] == S8).all() and (cnt[1:] == S32).all() and (sf[2 * n_seg:] == S32).all(), (what, "sentinels")
    k = int(cnt[0])
    assert k == len(want[1]) and (lst[k:] == S32).all(), (what, "the list and nothing behind it")
    assert sorted(lst[:k].tolist()) == want[1], (what, "descended groups")
    assert gver[:ng].tolist() == want[0], (what, "verdicts; a listed group's is left to its own check")
    assert sf[:2 * n_seg].tolist() == want[2], (what, "first batch per segment; the group words untouched")
    return gver[:ng].tolist(), sorted(lst[:k].tolist()), sf[:2 * n_seg].tolist()


def bver_of(ready_fail, fb):
    ng = len(ready_fail)
    return [int(any(ready_fail[b * fb:(b + 1) * fb])) for b in range((ng + fb - 1) // fb)]


@pytest.mark.parametrize("fb", [4, 64])
def test_three_sets_with_straddling_batches(D, fb):
    ng, off = 264, [0, 100, 200, 264]  # at fb 64 batches 1 (64 .. 127) and 3 (192 .. 255) straddle
    gseg, ready = segs(off), np.zeros(ng, np.uint8)
    rng = np.random.default_rng(fb)
    for fails in ([], [5], [99], [100], [99, 100], [150, 199, 263], [70, 130, 131, 210], list(range(ng))):
        fail = np.zeros(ng, np.uint8)
        fail[fails] = 1
        run_batch_verdict(D, ready, bver_of(fail, fb), fb, gseg, 3, what=fails)
    for rnd in range(6):
        fail = (rng.random(ng) < [0.01, 0.05, 0.5][rnd % 3]).astype(np.uint8)
        gst = np.where(rng.random(ng) < 0.1, rng.integers(1, 3, size=ng), 0)
        run_batch_verdict(D, gst, bver_of(fail & (gst == 0), fb), fb, gseg, 3, what=rnd)


@pytest.mark.parametrize("fb", [4, 64])
def test_200_groups_every_cut(D, fb):
    ng = 200
    rng = np.random.default_rng(200 + fb)
    for off in ([0, 200], [0, 1, 200], [0, 0, 63, 63, 64, 65, 200, 200], [0, 199, 200], [0, 3, 5, 6, 70, 130, 200],
                sorted(rng.integers(0, 201, size=40).tolist() + [0, 200])):
        gseg, n_seg = segs(off), len(off) - 1
        for p in (0.0, 0.02, 0.3, 1.0):
            fail = (rng.random(ng) < p).astype(np.uint8)
            run_batch_verdict(D, np.zeros(ng), bver_of(fail, fb), fb, gseg, n_seg, what=(off, p))


def test_head_batch_failing_through_the_earlier_set_only(D):
    # fb 64: batch 64 .. 127 fails (through set 0's groups 96 .. 99, which a batch verdict does not name); set 1
    # begins at 100 and its own failure is in batch 192 .. 255, two batches later
    ng, fb, gseg = 320, 64, segs([0, 100, 320])
    gver, lst, sf = run_batch_verdict(D, np.zeros(ng), [0, 1, 0, 1, 0], fb, gseg, 2)
    assert sf == [64, NONE, 192, NONE], "set 1's head batch does not count as its first failing batch"
    assert lst == list(range(64, 128)) + list(range(192, 256)), "set 1 descends in its head batch and in batch 192"
    # a later failing batch of set 1 stays unchecked; set 0's second failing batch as well
    gver, lst, sf = run_batch_verdict(D, np.zeros(ng), [1, 1, 0, 1, 1], fb, gseg, 2)
    assert sf == [0, NONE, 192, NONE] and lst == list(range(0, 64)) + list(range(100, 128)) + list(range(192, 256))
    assert gver[64:100] == [GV_UNCHECKED] * 36 and gver[256:] == [GV_UNCHECKED] * 64


def test_none_failing_issues_no_atomic_and_guard_zero_writes_nothing(D):
    ng, gseg = 200, segs([0, 100, 200])
    for fb in (4, 64):
        gver, lst, sf = run_batch_verdict(D, np.zeros(ng), [0] * ((ng + fb - 1) // fb), fb, gseg, 2)
        assert sf == [NONE] * 4 and lst == [] and gver == [PASS] * ng, "the atomics' targets still hold 0xff"
        gver, lst, sf = run_batch_verdict(D, np.zeros(ng), [1] * ((ng + fb - 1) // fb), fb, gseg, 2, guard=0)
        assert sf == [NONE] * 4 and lst == [] and gver == [KEEP] * ng, "guard byte 0: nothing is written"
        gver, lst, sf = run_batch_verdict(D, np.zeros(ng), [1] * ((ng + fb - 1) // fb), fb, gseg, 2, guard=1)
        assert sf[0] == 0 and len(lst) > 0


def test_chunk_offset(D):
    # the second chunk of a call: groups 64 .. 199 (g0 = 64, ng = 136), batches counted from the chunk's start
    g0, ng, fb = 64, 136, 64
    gseg = segs([0, 30, 100, 150, 200])
    for bver in ([1, 0, 0], [0, 1, 1], [1, 1, 1]):
        # the first chunk left first[1] = 0: set 1's batches here are later ones, and stay unchecked
        for sf0 in (None, [NONE, NONE, 0, 7, NONE, NONE, NONE, NONE]):
            run_batch_verdict(D, np.zeros(ng), bver, fb, gseg, 4, g0=g0, sf0=sf0, what=(bver, sf0))
    gver, lst, sf = run_batch_verdict(D, np.zeros(ng), [1, 1, 1], fb, gseg, 4, g0=g0)
    assert sf == [NONE, NONE, 64, NONE, 128, NONE, 192, NONE], "keys are group indices of the call, g0 included"


def test_a_set_id_equal_to_n_sets_touches_nothing(D):
    ng, fb = 130, 4
    gseg = segs([0, 50, 100, 130])  # three segments, of which the call has two
    gver, lst, sf = run_batch_verdict(D, np.zeros(ng), [1] * 33, fb, gseg, 2)
    assert gver[100:] == [GV_UNCHECKED] * 30 and all(g < 100 for g in lst) and sf == [0, NONE, 52, NONE]
    gver, lst, sf = run_batch_verdict(D, np.zeros(ng), [1] * 33, fb, np.full(ng, 7, np.uint32), 0)
    assert gver == [GV_UNCHECKED] * ng and lst == [] and sf == []


# ---------------------------------------------------------------------------------------------
# k_seg_first_group
# ---------------------------------------------------------------------------------------------
def run_first_group(D, gver, gseg, n_seg, sf0=None, what=""):
    gver, gseg, n = u8(gver), u32(gseg), len(gver)
    sf0 = [NONE] * (2 * n_seg) if sf0 is None else list(sf0)
    sf = np.concatenate([u32(sf0), np.full(PAD, S32, np.uint32)])
    assert D.dfd_first_group(n, _p(gver), _p(gseg), n_seg, PAD, _p(sf)) == 0
    want = list(sf0)
    for g in range(n):
        if 0 < gver[g] < 0x80 and gseg[g] < n_seg:
            want[2 * gseg[g] + 1] = min(want[2 * gseg[g] + 1], g)
    assert (sf[2 * n_seg:] == S32).all() and sf[:2 * n_seg].tolist() == want, what
    return want


def test_first_group_per_set(D):
    rng = np.random.default_rng(5)
    for n in (1, 63, 64, 65, 200, 264):
        for off in ([0, n], sorted({0, n // 3, min(64, n), n}), [0, 0] + sorted(rng.integers(0, n + 1, size=9).tolist()) + [n, n]):
            gseg, n_seg = segs(off), len(off) - 1
            assert run_first_group(D, np.zeros(n), gseg, n_seg, what=(n, off)) == [NONE] * (2 * n_seg), "none failing: no atomic"
            run_first_group(D, np.full(n, 3), gseg, n_seg, what=(n, off))
            for p in (0.02, 0.4):
                gver = np.where(rng.random(n) < p, rng.choice([1, 3, 0x7F, 0x80, 0x81], size=n), 0)
                run_first_group(D, gver, gseg, n_seg, sf0=rng.integers(0, 5, size=2 * n_seg) * 64, what=(n, off, p))
    assert run_first_group(D, np.full(130, 3), segs([0, 50, 100, 130]), 2) == [NONE, 0, NONE, 50], "a set id >= n_sets"


# ---------------------------------------------------------------------------------------------
# k_seg_scatter
# ---------------------------------------------------------------------------------------------
def run_scatter(D, item_grp, msg_idx, hm_inf, pk_inf, pk_st, sig_inf, sig_st, gver, grp_off, gseg, n_seg, sf, what=""):
    n, ngr = len(item_grp), len(gver)
    a = [u32(item_grp), u32(msg_idx), u8(hm_inf), u8(pk_inf), u8(pk_st), u8(sig_inf), u8(sig_st), u8(gver),
         None if grp_off is None else u32(grp_off), u32(gseg), u32(sf if len(sf) else [S32, S32])]
    st = np.concatenate([np.full(n, KEEP, np.uint8), np.full(PAD, S8, np.uint8)])
    lst, cnt = np.full(n + PAD, S32, np.uint32), np.concatenate([np.zeros(1, np.uint32), np.full(PAD, S32, np.uint32)])
    rc = D.dfd_scatter(n, _p(a[0]), _p(a[1]), len(hm_inf), _p(a[2]), _p(a[3]), _p(a[4]), _p(a[5]), _p(a[6]), ngr, _p(a[7]),
                       _p(a[8]), _p(a[9]), n_seg, _p(a[10]), PAD, _p(st), _p(lst), _p(cnt))
    assert rc == 0
    want, wl = [KEEP] * n, []
    for i in range(n):
        g = int(item_grp[i])
        k, v = int(gseg[g]), int(gver[g])
        if pk_st[i]:
            want[i] = BAD_PUBKEY
        elif sig_st[i]:
            want[i] = BAD_SIGNATURE
        elif pk_inf[i] or sig_inf[i] or hm_inf[msg_idx[i]]:
            want[i] = NOT_VERIFIED
        elif v == PASS:
            want[i] = OK
        elif v == GV_UNCHECKED or (v < 0x80 and (k >= n_seg or sf[2 * k + 1] != g)):
            want[i] = UNCHECKED  # an unchecked group, or a failing one that is not its set's first
        elif grp_off is None or grp_off[g + 1] - grp_off[g] <= 1:
            want[i] = NOT_VERIFIED  # a failing group of one item: its verdict is the item's
        else:
            wl.append(i)  # the set's first failing group, or a group that was not READY: re-checked alone
    k = int(cnt[0])
    assert (st[n:] == S8).all() and (cnt[1:] == S32).all() and (lst[k:] == S32).all(), (what, "sentinels")
    assert sorted(lst[:k].tolist()) == wl and st[:n].tolist() == want, what
    return st[:n].tolist(), wl


@pytest.mark.parametrize("per_group", [1, 3])
def test_scatter(D, per_group):
    rng = np.random.default_rng(per_group)
    for ngr, off in ((1, [0, 1]), (70, [0, 10, 10, 64, 70]), (200, [0, 100, 200]), (130, [0, 50, 100, 130])):
        n_seg = len(off) - 1 if ngr != 130 else 2  # the last shape: groups of a set id the call does not have
        sizes = np.full(ngr, per_group) if per_group == 1 else rng.integers(1, per_group + 1, size=ngr)
        grp_off = np.concatenate([[0], np.cumsum(sizes)])
        n = int(grp_off[-1])
        item_grp = np.repeat(np.arange(ngr), sizes)
        gseg = segs(off)
        for rnd in range(4):
            gver = np.where(rng.random(ngr) < [0, 0.1, 0.5, 1][rnd], rng.choice([3, 3, 0x80, 0x81], size=ngr), 0)
            sf = [NONE] * (2 * n_seg)
            for g in range(ngr):  # what k_seg_first_group leaves
                if 0 < gver[g] < 0x80 and gseg[g] < n_seg:
                    sf[2 * gseg[g] + 1] = min(sf[2 * gseg[g] + 1], g)
            flags = [(rng.random(n) < 0.03).astype(np.uint8) for _ in range(4)]
            st, wl = run_scatter(D, item_grp, rng.integers(0, 2, size=n), [0, rnd == 3], flags[0], flags[1], flags[2], flags[3],
                                 gver, None if per_group == 1 else grp_off, gseg, n_seg, sf, what=(ngr, rnd))
            if rnd == 0:
                assert wl == [] and set(st) <= {OK, BAD_PUBKEY, BAD_SIGNATURE, NOT_VERIFIED}


# ---------------------------------------------------------------------------------------------
# k_seg_first_item
# ---------------------------------------------------------------------------------------------
def run_first_item(D, status, item_seg, arrival, n_seg, what=""):
    status, item_seg, arrival, n = u8(status), u32(item_seg), u32(arrival), len(status)
    sf = np.concatenate([np.full(n_seg, NONE, np.uint32), np.full(PAD, S32, np.uint32)])
    assert D.dfd_first_item(n, _p(status), _p(item_seg), _p(arrival), n_seg, PAD, _p(sf)) == 0
    want = [NONE] * n_seg
    for q in range(n):
        if status[q] not in (OK, UNCHECKED) and item_seg[q] < n_seg:  # decided and not OK
            want[item_seg[q]] = min(want[item_seg[q]], int(arrival[q]))
    assert (sf[n_seg:] == S32).all() and sf[:n_seg].tolist() == want, what
    return want


def test_first_item_skips_unchecked(D):
    rng = np.random.default_rng(9)
    for n in (1, 63, 64, 65, 130, 300):
        for off in ([0, n], [0, 0] + sorted({n // 3, min(64, n)}) + [n, n], list(range(n + 1))):
            sid, n_seg = segs(off), len(off) - 1
            arr = np.arange(n) + 1000
            assert run_first_item(D, np.zeros(n), sid, arr, n_seg) == [NONE] * n_seg, "a clean add issues no atomic"
            assert run_first_item(D, np.full(n, UNCHECKED), sid, arr, n_seg) == [NONE] * n_seg, "unchecked is not a failure"
            got = run_first_item(D, np.full(n, NOT_VERIFIED), sid, arr, n_seg)
            assert got == [1000 + off[k] if off[k + 1] > off[k] else NONE for k in range(n_seg)]
            for p in (0.05, 0.5):
                st = np.where(rng.random(n) < p, rng.choice([1, 2, 3, 7, 7], size=n), 0)
                run_first_item(D, st, sid, rng.permutation(n) + 3, n_seg, what=(n, p))
    # an unchecked item before the set's first decided failure (another shard's, after the merge) is skipped
    assert run_first_item(D, [0, 7, 3, 7, 0, 2], [0, 0, 0, 1, 1, 1], np.arange(6), 2) == [2, 5]
    assert run_first_item(D, [3, 3, 3], [0, 1, 2], np.arange(3), 2) == [0, 1], "a set id >= n_sets touches nothing"
