"""The host side of first-error duty set adds (hbls_duty_add_sets_first) on the CPU, through the g++
harness tests/native/dutyfirstcheck.cpp: the set-major plan of a shard (charon_amd/csrc/hduty.h
duty_plan_shard with set ids) against a Python restatement and against the message-sorted plan it must
agree with in everything the store reads, and the descent rule of the segmented first-error
verification (charon_amd/csrc/dutyfirst.h, what dutyfirst.hip's kernels run per lane) over seeded
streams of group verdicts: each set's first failure must be its first failing group in arrival order.
"""
import ctypes

import numpy as np
import pytest

NONE = 0xFFFFFFFF
PASS, FAILED, UNCHECKED, NOT_READY = 0, 3, 0x80, 0x81


@pytest.fixture(scope="module")
def H():
    from gpu_helpers import harness
    lib = harness.load("dutyfirstcheck")
    V, SZ, U32, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    lib.df_plan.argtypes = [V, V, V, SZ, V, SZ, I, SZ, SZ, SZ, U32, SZ] + [V] * 10
    lib.df_rule.argtypes = [SZ, SZ, U32, V, V, V, U32, V, V, V, V]
    return lib


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


# ---------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------
def plan(H, c, k, use_sets):
    n, S = len(c["msg"]), len(c["set_off"]) - 1
    o = dict(order=np.full(n + 1, NONE, np.uint32), midx=np.full(n + 1, NONE, np.uint32), serial=np.full(n + 1, NONE, np.uint32),
             vgoff=np.full(n + 2, NONE, np.uint32), vgset=np.full(n + 1, NONE, np.uint32), tgroup=np.full(n + 1, NONE, np.uint32),
             toff=np.full(n + 2, NONE, np.uint32), tpos=np.full(n + 1, NONE, np.uint32), tidx=np.full(n + 1, -1, np.int64))
    res = np.zeros(6, np.uint64)
    rc = H.df_plan(_p(c["msg"]), _p(c["group"]), _p(c["idx"]), n, _p(c["set_off"]), S, int(use_sets), c["G"], c["nd"], c["gmax"],
                   c["first"], k, _p(o["order"]), _p(o["midx"]), _p(o["serial"]), _p(o["vgoff"]), _p(o["vgset"]),
                   _p(o["tgroup"]), _p(o["toff"]), _p(o["tpos"]), _p(o["tidx"]), _p(res))
    assert rc == 0
    m, nvg, nt, npos = (int(x) for x in res[:4])
    assert o["order"][m] == NONE and o["vgoff"][nvg + 1] == NONE and o["tgroup"][nt] == NONE and o["tpos"][npos] == NONE
    return dict(order=o["order"][:m].tolist(), midx=o["midx"][:m].tolist(), serial=o["serial"][:m].tolist(),
                vgoff=o["vgoff"][:nvg + 1].tolist(), vgset=o["vgset"][:nvg].tolist() if use_sets else None,
                touched={int(o["tgroup"][u]): [(int(o["order"][o["tpos"][j]]), int(o["tidx"][j]))
                                               for j in range(o["toff"][u], o["toff"][u + 1])] for u in range(nt)},
                tgroup=o["tgroup"][:nt].tolist(), table=int(res[4]), resident=int(res[5]))


def shard_items(c, k):
    """hduty.h duty_route restated: a partial goes to its group's shard, a verify-only one by position"""
    n, G, nd = len(c["msg"]), c["G"], c["nd"]
    out = []
    for i in range(n):
        g = int(c["group"][i])
        s = next(j for j in range(nd) if G * j // nd <= g < G * (j + 1) // nd) if g < G else i * nd // n
        if s == k:
            out.append(i)
    return out


def model_groups(msg, sets, gmax):
    """runs of consecutive items over one message, at most gmax, broken at every set boundary"""
    off, gset = [], []
    for q in range(len(msg)):
        if q == 0 or sets[q] != sets[q - 1] or msg[q] != msg[q - 1] or q - off[-1] >= gmax:
            off.append(q)
            gset.append(sets[q])
    return off + [len(msg)], gset


def random_call(rng, nd):
    n = int(rng.integers(1, 90))
    G = int(rng.integers(nd, 12))
    S = int(rng.integers(1, 8))
    cuts = np.sort(rng.integers(0, n + 1, size=S - 1)).tolist()  # repeated cuts: empty sets anywhere
    if rng.random() < 0.3:
        cuts = ([0] + cuts)[:S - 1] if S > 1 else cuts
    set_off = np.array([0] + sorted(cuts) + [n], np.uint32)
    msg = np.repeat(rng.integers(1, 5, size=n), rng.integers(1, 6, size=n))[:n].astype(np.uint32)  # runs of one message
    group = np.where(rng.random(n) < 0.15, NONE, rng.integers(0, G, size=n)).astype(np.uint32)
    return dict(msg=msg, group=group, idx=rng.integers(1, 9, size=n).astype(np.int64), set_off=set_off, G=G, nd=nd,
                gmax=int(rng.choice([1, 3, 8, 100])), first=int(rng.integers(0, 1000)))


@pytest.mark.parametrize("nd", [1, 2, 3])
def test_set_major_plan(H, nd):
    rng = np.random.default_rng(100 + nd)
    seen_empty = seen_gmax = seen_boundary = 0
    for _ in range(150):
        c = random_call(rng, nd)
        n, so = len(c["msg"]), c["set_off"].tolist()
        set_of = np.repeat(np.arange(len(so) - 1), np.diff(so)).tolist()
        seen_empty += any(so[j] == so[j + 1] for j in range(len(so) - 1))
        covered = []
        for k in range(nd):
            items = shard_items(c, k)
            covered += items
            p, q = plan(H, c, k, True), plan(H, c, k, False)
            assert p["order"] == items, "set-major and arrival order within the set: the shard's items as they came"
            assert p["serial"] == [c["first"] + i for i in items]
            ids = {}
            for i in items:  # message ids in order of first appearance
                ids.setdefault(int(c["msg"][i]), len(ids))
            assert p["midx"] == [ids[int(c["msg"][i])] for i in items]
            off, gset = model_groups([int(c["msg"][i]) for i in items], [set_of[i] for i in items], c["gmax"])
            assert p["vgoff"] == off and p["vgset"] == gset
            assert all(b - a <= c["gmax"] for a, b in zip(off, off[1:]))
            seen_gmax += any(b - a == c["gmax"] and b < len(items) and set_of[items[b]] == set_of[items[b - 1]] and
                             c["msg"][items[b]] == c["msg"][items[b - 1]] for a, b in zip(off, off[1:]))
            seen_boundary += any(0 < b < len(items) and set_of[items[b]] != set_of[items[b - 1]] and
                                 c["msg"][items[b]] == c["msg"][items[b - 1]] for b in off)
            # what k_duty_store reads is the message-sorted plan's, item for item
            assert p["tgroup"] == q["tgroup"] and p["touched"] == q["touched"]
            assert sorted(zip(q["order"], q["midx"], q["serial"])) == sorted(zip(p["order"], p["midx"], p["serial"]))
            assert (p["table"], p["resident"]) == (q["table"], q["resident"])
        assert sorted(covered) == list(range(n))
    assert seen_empty > 20 and seen_gmax > 20 and seen_boundary > 20, (seen_empty, seen_gmax, seen_boundary)


def test_plan_of_a_single_set_and_of_singleton_sets(H):
    n = 20
    msg = np.array([7] * 9 + [8] * 11, np.uint32)
    base = dict(msg=msg, group=np.arange(n, dtype=np.uint32) % 4, idx=np.ones(n, np.int64), G=4, nd=1, gmax=8, first=5)
    one = plan(H, dict(base, set_off=np.array([0, n], np.uint32)), 0, True)
    assert one["vgoff"] == [0, 8, 9, 17, 20] and one["vgset"] == [0, 0, 0, 0]
    each = plan(H, dict(base, set_off=np.arange(n + 1, dtype=np.uint32)), 0, True)
    assert each["vgoff"] == list(range(n + 1)) and each["vgset"] == list(range(n))
    empties = plan(H, dict(base, set_off=np.array([0, 0, 0, 9, 9, 20, 20], np.uint32)), 0, True)
    assert empties["vgoff"] == [0, 8, 9, 17, 20] and empties["vgset"] == [2, 2, 4, 4]


# ---------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------
def c_rule(H, ready, fail, gseg, n_seg, gcap, fb):
    n = len(ready)
    gver, unch, desc = np.full(n + 1, 0x5A, np.uint8), np.full(n + 1, 0x5A, np.uint8), np.full(n + 1, 0x5A, np.uint8)
    sf = np.full(2 * n_seg + 1, 0x5A5A5A5A, np.uint32)
    H.df_rule(n, gcap, fb, _p(ready), _p(fail), _p(gseg), n_seg, _p(gver), _p(sf), _p(unch), _p(desc))
    assert gver[n] == 0x5A and unch[n] == 0x5A and desc[n] == 0x5A and sf[2 * n_seg] == 0x5A5A5A5A
    return gver[:n].tolist(), sf[:2 * n_seg].tolist(), unch[:n].tolist(), desc[:n].tolist()


def py_rule(ready, fail, gseg, n_seg, gcap, fb):
    """include/hipbls.h's and DESIGN.md's wording restated: per chunk the batches' verdicts, per set the
    smallest failing batch that is not its head batch, and which groups of a failing batch descend"""
    n = len(ready)
    gver, desc, first_batch = [None] * n, [0] * n, [NONE] * n_seg
    for g0 in range(0, n, gcap):
        ng = min(gcap, n - g0)
        batch_of = lambda g: g0 + (g - g0) // fb * fb  # noqa: E731
        failing = {batch_of(g) for g in range(g0, g0 + ng) if ready[g] and fail[g]}
        head = lambda g: gseg[batch_of(g)] != gseg[g]  # noqa: E731 -- the batch begins with an earlier set's group
        for g in range(g0, g0 + ng):
            if ready[g] and batch_of(g) in failing and gseg[g] < n_seg and not head(g):
                first_batch[gseg[g]] = min(first_batch[gseg[g]], batch_of(g))
        for g in range(g0, g0 + ng):
            if not ready[g]:
                gver[g] = NOT_READY
            elif batch_of(g) not in failing:
                gver[g] = PASS
            elif gseg[g] < n_seg and (head(g) or first_batch[gseg[g]] == batch_of(g)):
                gver[g], desc[g] = (FAILED if fail[g] else PASS), 1
            else:
                gver[g] = UNCHECKED
    first_group = [NONE] * n_seg
    for g in range(n):
        if gver[g] == FAILED and gseg[g] < n_seg:
            first_group[gseg[g]] = min(first_group[gseg[g]], g)
    unch = [int(gver[g] == UNCHECKED or (gver[g] == FAILED and (gseg[g] >= n_seg or first_group[gseg[g]] != g)))
            for g in range(n)]
    sf = [x for k in range(n_seg) for x in (first_batch[k], first_group[k])]
    return gver, sf, unch, desc


def random_stream(rng):
    n = int(rng.integers(1, 330))
    fb = int(rng.choice([1, 2, 3, 4, 5, 16, 64]))
    gcap = int(rng.choice([n, n, 64, 100, 136, 7 * fb]))
    S = int(rng.integers(1, 12))
    kind = rng.integers(0, 3)
    if kind == 0:  # short sets: several inside one batch
        lens = rng.integers(0, max(2, fb // 2 + 1), size=S)
    elif kind == 1:
        lens = rng.integers(0, 3 * fb + 2, size=S)
    else:
        lens = rng.integers(0, n + 1, size=S)
    off = np.minimum(np.concatenate([[0], np.cumsum(lens)]), n)
    off[-1] = n
    gseg = np.repeat(np.arange(S), np.diff(off)).astype(np.uint32)
    fail = np.zeros(n, np.uint8)
    for k in range(S):
        a, b = int(off[k]), int(off[k + 1])
        if a == b:
            continue
        mode = rng.integers(0, 6)
        if mode == 1:  # one failure, anywhere
            fail[rng.integers(a, b)] = 1
        elif mode == 2:  # the set's last groups: the next set's head batch fails through this one
            fail[max(a, b - int(rng.integers(1, 4))):b] = 1
        elif mode == 3:  # a late failure only
            fail[a + (b - a) * 3 // 4:b] = rng.random(b - a - (b - a) * 3 // 4) < 0.3
        elif mode == 4:  # many
            fail[a:b] = rng.random(b - a) < rng.choice([0.1, 0.5, 1.0])
    ready = (rng.random(n) >= rng.choice([0, 0, 0.05, 0.3])).astype(np.uint8)
    return ready, fail, gseg, S, gcap, fb, off


def test_rule_over_seeded_streams(H):
    rng = np.random.default_rng(20261021)
    seen = dict(inside_one_batch=0, three_sets_in_a_batch=0, head_fails_through_previous=0, two_failing_batches=0,
                chunk_offset=0, unchecked=0, not_ready=0)
    for _ in range(2000):
        ready, fail, gseg, S, gcap, fb, off = random_stream(rng)
        n = len(ready)
        got = c_rule(H, ready, fail, gseg, S, gcap, fb)
        want = py_rule(ready.tolist(), fail.tolist(), gseg.tolist(), S, gcap, fb)
        assert got == want, (n, S, gcap, fb)
        gver, sf, unch, desc = got
        batch_of = lambda g: g // gcap * gcap + (g % gcap) // fb * fb  # noqa: E731
        failing = {batch_of(g) for g in range(n) if ready[g] and fail[g]}
        seen["chunk_offset"] += gcap < n
        seen["not_ready"] += int((ready == 0).any())
        by_batch = {}
        for g in range(n):
            by_batch.setdefault(batch_of(g), set()).add(int(gseg[g]))
        seen["three_sets_in_a_batch"] += any(len(v) >= 3 for v in by_batch.values())
        for k in range(S):
            a, b = int(off[k]), int(off[k + 1])
            bad = [g for g in range(a, b) if ready[g] and fail[g]]
            # the property: the set's first failure is its first failing group in arrival order
            assert sf[2 * k + 1] == (bad[0] if bad else NONE), (k, n, S, gcap, fb)
            if a == b:
                continue
            first = bad[0] if bad else b
            assert all(gver[g] in (PASS, NOT_READY) for g in range(a, first)), "every group before it passed or is exact"
            assert all(gver[g] == NOT_READY for g in range(a, b) if not ready[g]), "NOT_READY groups keep the exact fallback"
            assert not any(unch[g] for g in range(a, first + 1 if bad else b)), "nothing up to the first failure is left unchecked"
            assert all(unch[g] for g in range(first + 1, b) if ready[g] and gver[g] != PASS), "behind it nothing is re-checked"
            assert len({batch_of(g) for g in range(a, b) if desc[g]}) <= 2, "at most two batches per set descend"
            mine = {batch_of(g) for g in range(a, b)}
            seen["inside_one_batch"] += len(mine) == 1 and len(by_batch[batch_of(a)]) > 1
            seen["two_failing_batches"] += len({batch_of(g) for g in bad}) >= 2
            seen["unchecked"] += any(gver[g] == UNCHECKED for g in range(a, b))
            head = batch_of(a)
            if gseg[head] != k and head in failing and bad and batch_of(bad[0]) != head:
                seen["head_fails_through_previous"] += 1
    assert all(v >= 50 for v in seen.values()), seen


def test_rule_head_batch_failing_through_the_previous_set_only():
    """the pitfall, by hand: fb 4, set 1 begins at group 6 (batch 4..7, which fails through group 5 of
    set 0 alone); set 1's own failure is group 13, two batches later"""
    ready, fail = [1] * 16, [0] * 16
    fail[5] = fail[13] = 1
    gseg = [0] * 6 + [1] * 10
    gver, sf, unch, desc = py_rule(ready, fail, gseg, 2, 16, 4)
    assert sf == [4, 5, 12, 13]
    assert [g for g in range(16) if desc[g]] == [4, 5, 6, 7, 12, 13, 14, 15]
    assert not any(unch)


def test_rule_by_hand_through_the_harness(H):
    ready, fail = np.ones(16, np.uint8), np.zeros(16, np.uint8)
    fail[[5, 13]] = 1
    gseg = np.array([0] * 6 + [1] * 10, np.uint32)
    gver, sf, unch, desc = c_rule(H, ready, fail, gseg, 2, 16, 4)
    assert sf == [4, 5, 12, 13] and not any(unch)
    assert [g for g in range(16) if desc[g]] == [4, 5, 6, 7, 12, 13, 14, 15]
    # a set id outside the call's sets indexes nothing: left unchecked, sfirst untouched
    gver, sf, unch, desc = c_rule(H, ready, fail, np.full(16, 2, np.uint32), 2, 16, 4)
    assert sf == [NONE] * 4 and not any(desc) and [gver[g] for g in (5, 13, 0)] == [UNCHECKED, UNCHECKED, PASS]
