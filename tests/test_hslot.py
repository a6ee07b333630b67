"""The host side of hbls_slot_select_batch on the CPU, through the g++ harness
tests/native/slothostcheck.cpp: the matching rule (charon_amd/csrc/tasel.h ta_select_matching, what
threshold.hip's k_ta_select runs per lane in that mode) and the plan that cuts one duty into one
shard per device (charon_amd/csrc/hslot.h).

The rule's expected values come from matching() below, the rule as include/hipbls.h states it (the
reference's parsigdb/memory.go:149-160 and 197-225), or are hand-written rows; the plan's from the
caller's own arrays: whatever the order a shard uploads, every group's candidates must name the
same partials and every partial must be verified somewhere.  All comparisons are exact.
"""
import ctypes
import hashlib

import numpy as np
import pytest

OK, BAD_PUBKEY, BAD_SIGNATURE, NOT_VERIFIED = 0, 1, 2, 3
NONE = 0xFFFFFFFF
ST_OK, ST_FEW, ST_MIXED = 0, 1, 2
FIRST, MATCHING = 0, 1
KEY_NONE = 0x10000


@pytest.fixture(scope="module")
def hs():
    from gpu_helpers import harness
    lib = harness.load("slothostcheck")
    P, U, SZ = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t
    lib.hs_select.argtypes, lib.hs_select.restype = [U, P, P, U, P, P, U, U, U, P, P, P], None
    lib.hs_plan_new.argtypes, lib.hs_plan_new.restype = [P, P, P, SZ, P, P, SZ, SZ, SZ], P
    lib.hs_plan_free.argtypes, lib.hs_plan_free.restype = [P], None
    lib.hs_plan_shards.argtypes, lib.hs_plan_shards.restype = [P], SZ
    lib.hs_shard_info.argtypes, lib.hs_shard_info.restype = [P, SZ, P], None
    lib.hs_shard_msg_bytes.argtypes, lib.hs_shard_msg_bytes.restype = [P, SZ], SZ
    lib.hs_shard_copy.argtypes, lib.hs_shard_copy.restype = [P, SZ, P, P, P, P, P, P, P, P], None
    lib.hs_chosen_to_caller.argtypes, lib.hs_chosen_to_caller.restype = [P, SZ, P, SZ], None
    return lib


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


# ---------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------
def select(hs, mode, vstatus, cand, t, msg_idx=None):
    """cand: [(partial, share index)] of one group.  -> dict(chosen, cidx, count, key, msg, state, shifted)"""
    vst = np.asarray(vstatus, dtype=np.uint8)
    n = len(vst)
    mid = np.asarray(msg_idx if msg_idx is not None else [0] * n, dtype=np.uint32)
    src = np.asarray([c[0] for c in cand] or [0], dtype=np.uint32)
    idx = np.asarray([c[1] for c in cand] or [0], dtype=np.int64)
    chosen, cidx, res = np.full(t, 12345, np.uint32), np.full(t, 12345, np.int64), np.zeros(5, np.uint32)
    hs.hs_select(mode, _p(vst if n else np.zeros(1, np.uint8)), _p(mid if n else np.zeros(1, np.uint32)), n, _p(src),
                 _p(idx), 0, len(cand), t, _p(chosen), _p(cidx), _p(res))
    return dict(chosen=[int(x) for x in chosen], cidx=[int(x) for x in cidx], count=int(res[0]), key=int(res[1]),
                msg=int(res[2]), state=int(res[3]), shifted=int(res[4]))


def matching(vstatus, msg_idx, cand, t):
    """The matching rule restated.  -> (member candidate positions, winning message or None).
    Candidate j is stored iff it is verified and no earlier verified candidate has its share index;
    the first message to hold t stored candidates wins.  Without a winner: candidates over one message
    report their stored ones (what the first-t rule reports below t), several messages report none."""
    n = len(vstatus)
    seen, by_root = set(), {}
    for k, (p, x) in enumerate(cand):
        if p >= n or vstatus[p] != OK or x in seen:
            continue
        seen.add(x)
        pos = by_root.setdefault(msg_idx[p], [])
        pos.append(k)
        if len(pos) == t:
            return pos, msg_idx[p]
    roots = {msg_idx[p] for p, _ in cand if p < n}
    return (next(iter(by_root.values()), []) if len(roots) <= 1 else []), None


def expect(vstatus, msg_idx, cand, t):
    pos, root = matching(vstatus, msg_idx, cand, t)
    key = 0
    for k in pos:
        key ^= 1 << (k & 15)
    return dict(chosen=[cand[k][0] for k in pos] + [NONE] * (t - len(pos)),
                cidx=[cand[k][1] for k in pos] + [0] * (t - len(pos)), count=len(pos),
                key=key if root is not None else KEY_NONE, state=ST_OK if root is not None else ST_FEW,
                shifted=int(root is not None and pos != list(range(t))), root=root)


def check(hs, vstatus, msg_idx, cand, t):
    r, e = select(hs, MATCHING, vstatus, cand, t, msg_idx), expect(vstatus, msg_idx, cand, t)
    for k in ("chosen", "cidx", "count", "key", "state", "shifted"):
        assert r[k] == e[k], (k, r, e)
    if e["root"] is not None:
        assert r["msg"] == e["root"]
    return r


def shares(n, first=0):
    return [(first + k, k + 1) for k in range(n)]


def test_single_root_groups_equal_the_first_t_rule(hs):
    """Candidates over one message: chosen, count, key (and the rest) of ta_select, for every status
    pattern of 7 candidates at t = 5 -- below t too -- and random rows with repeated share indices."""
    rows = [([OK if (m >> k) & 1 else NOT_VERIFIED for k in range(7)], shares(7), 5) for m in range(128)]
    rng = np.random.default_rng(7)
    for _ in range(300):
        n, t = int(rng.integers(1, 12)), int(rng.integers(1, 8))
        vst = [int(x) for x in rng.choice([OK, OK, OK, NOT_VERIFIED, BAD_SIGNATURE], size=n)]
        rows.append((vst, [(int(rng.integers(0, n + 2)), int(rng.integers(1, 6))) for _ in range(int(rng.integers(0, 12)))], t))
    for vst, cand, t in rows:
        mid = [3] * len(vst)
        a, b = select(hs, FIRST, vst, cand, t, mid), select(hs, MATCHING, vst, cand, t, mid)
        assert a == b and a["state"] != ST_MIXED, (vst, cand, t)
        check(hs, vst, mid, cand, t)


def test_interleaved_roots(hs):
    """Roots A A B A B B at t = 3: A completes at candidate 3, before B does at candidate 5."""
    A, B = 4, 9
    r = check(hs, [OK] * 6, [A, A, B, A, B, B], shares(6), 3)
    assert r["chosen"] == [0, 1, 3] and r["cidx"] == [1, 2, 4] and r["msg"] == A
    assert (r["count"], r["state"], r["shifted"], r["key"]) == (3, ST_OK, 1, 0b1011)
    # the first-t rule refuses the same group
    assert select(hs, FIRST, [OK] * 6, shares(6), 3, [A, A, B, A, B, B])["state"] == ST_MIXED


def test_earlier_completion_wins(hs):
    """Both roots are one partial short; B's t-th arrives before A's."""
    A, B = 0, 1
    mid = [A, A, B, B, B, A]
    r = check(hs, [OK] * 6, mid, shares(6), 3)
    assert r["chosen"] == [2, 3, 4] and r["msg"] == B and r["shifted"] == 1
    # with B's third partial unverified A completes instead, at the last candidate
    r = check(hs, [OK, OK, OK, OK, NOT_VERIFIED, OK], mid, shares(6), 3)
    assert r["chosen"] == [0, 1, 5] and r["msg"] == A


def test_duplicate_share_index_across_roots(hs):
    """A second partial under a stored share index is dropped whatever its root: share 2 over A is
    stored first, so share 2 over B never counts and B stays below t."""
    A, B = 0, 1
    cand = [(0, 1), (1, 2), (2, 2), (3, 3), (4, 4)]
    mid = [A, A, B, B, B]
    r = check(hs, [OK] * 5, mid, cand, 3)
    assert r["state"] == ST_FEW and r["count"] == 0 and r["chosen"] == [NONE] * 3 and r["key"] == KEY_NONE
    # an unverified partial does not reserve its share index: now share 2 over B is stored
    r = check(hs, [OK, NOT_VERIFIED, OK, OK, OK], mid, cand, 3)
    assert r["chosen"] == [2, 3, 4] and r["cidx"] == [2, 3, 4] and r["msg"] == B
    # the dropped duplicate is skipped, the root still completes with a later share
    r = check(hs, [OK] * 6, [A, B, A, A, B, A], [(0, 1), (1, 1), (2, 2), (3, 2), (4, 3), (5, 3)], 3)
    assert r["state"] == ST_FEW
    r = check(hs, [OK] * 6, [A, B, A, A, B, A], [(0, 1), (1, 1), (2, 2), (3, 2), (4, 3), (5, 4)], 3)
    assert r["chosen"] == [0, 2, 5] and r["msg"] == A


def test_enough_verified_but_no_root_reaches_t(hs):
    r = check(hs, [OK] * 6, [0, 1, 2, 0, 1, 2], shares(6), 3)
    assert (r["state"], r["count"], r["key"]) == (ST_FEW, 0, KEY_NONE) and r["chosen"] == [NONE] * 3


def test_no_candidates_and_forty(hs):
    r = check(hs, [OK] * 4, [0, 1, 0, 1], [], 3)
    assert (r["state"], r["count"], r["msg"]) == (ST_FEW, 0, 0) and r["chosen"] == [NONE] * 3
    r = select(hs, MATCHING, [], [], 2)  # a call without partials
    assert (r["state"], r["count"]) == (ST_FEW, 0) and r["chosen"] == [NONE] * 2
    # 40 candidates over 5 roots, share indices 1 .. 40, every third unverified: no bound on the count
    vst = [NOT_VERIFIED if k % 3 == 0 else OK for k in range(40)]
    mid = [k % 5 for k in range(40)]
    r = check(hs, vst, mid, shares(40), 6)
    assert r["state"] == ST_OK and r["count"] == 6 and r["shifted"] == 1
    assert check(hs, vst, mid, shares(40), 16)["state"] == ST_FEW
    # ... and random ones, with repeated share indices and candidates naming no partial
    rng = np.random.default_rng(11)
    for _ in range(400):
        n, t = int(rng.integers(1, 30)), int(rng.integers(1, 9))
        vst = [int(x) for x in rng.choice([OK, OK, OK, NOT_VERIFIED, BAD_SIGNATURE], size=n)]
        mid = [int(x) for x in rng.integers(0, int(rng.integers(1, 4)), size=n)]
        cand = [(int(rng.integers(0, n + 2)), int(rng.integers(1, 12))) for _ in range(int(rng.integers(0, 41)))]
        r = check(hs, vst, mid, cand, t)
        assert r["state"] != ST_MIXED


def test_candidate_naming_no_partial_counts_as_not_verified(hs):
    r = check(hs, [OK] * 4, [0, 1, 0, 0], [(0, 1), (7, 2), (NONE, 3), (1, 4), (2, 5), (4, 6), (3, 7)], 3)
    assert r["chosen"] == [0, 2, 3] and r["cidx"] == [1, 5, 7] and r["msg"] == 0


# ---------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------
def duty(layout, V=23, nsh=4, M=5, orphans=0):
    """V validators x nsh partials, validator v over message v % M (32 bytes each, of distinct
    lengths for two of them), in validator-major (item = v nsh + share) or peer-major (item =
    share V + v) order, then `orphans` partials no validator lists.  -> dict of the caller's arrays;
    group v lists its nsh partials in share order."""
    n = V * nsh + orphans
    item = (lambda v, s: v * nsh + s) if layout == "validator" else (lambda v, s: s * V + v)
    roots = [hashlib.sha256(bytes([m])).digest()[:32 - (m % 3)] for m in range(M + 1)]
    owner = np.zeros(n, dtype=np.int64)
    for v in range(V):
        for s in range(nsh):
            owner[item(v, s)] = v % M
    owner[V * nsh:] = M  # the orphans' message, which no listed partial has
    msgs, off = [], []
    for i in range(n):
        off.append(sum(len(x) for x in msgs))
        msgs.append(roots[owner[i]])
    d = dict(n=n, V=V, nsh=nsh, roots=roots, owner=owner, msgs=np.frombuffer(b"".join(msgs), dtype=np.uint8).copy(),
             off=np.asarray(off, dtype=np.uint64), len=np.asarray([len(x) for x in msgs], dtype=np.uint32))
    d["groups"] = [[item(v, s) for s in range(nsh)] for v in range(V)]
    return d


def flat(groups):
    cand = np.asarray([c for g in groups for c in g] or [0], dtype=np.uint32)
    goff = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.uint32)
    return cand, goff


def plan(hs, d, groups, nd, gmax=3):
    """-> [dict per shard]"""
    cand, goff = flat(groups)
    h = hs.hs_plan_new(_p(d["msgs"]), _p(d["off"]), _p(d["len"]), d["n"], _p(cand), _p(goff), len(groups), nd, gmax)
    try:
        out = []
        for k in range(hs.hs_plan_shards(h)):
            info = np.zeros(7, dtype=np.uint64)
            hs.hs_shard_info(h, k, _p(info))
            gb, ge, whole, m, nvg, nm, nc = (int(x) for x in info)
            a = dict(order=np.zeros(max(m, 1), np.uint32), midx=np.zeros(max(m, 1), np.uint32),
                     vgoff=np.zeros(nvg + 1, np.uint32), cand=np.zeros(max(nc, 1), np.uint32),
                     goff=np.zeros(ge - gb + 1, np.uint32), moff=np.zeros(max(nm, 1), np.uint64),
                     mlen=np.zeros(max(nm, 1), np.uint32),
                     mbytes=np.zeros(max(hs.hs_shard_msg_bytes(h, k), 1), np.uint8))
            hs.hs_shard_copy(h, k, *(_p(a[x]) for x in ("order", "midx", "vgoff", "cand", "goff", "moff", "mlen", "mbytes")))
            a.update(gb=gb, ge=ge, whole=bool(whole), m=m, nvg=nvg, nm=nm, nc=nc)
            # chosen back to the caller: every position, one past the last, and the sentinel
            ch = np.asarray(list(range(m)) + [m, NONE], dtype=np.uint32)
            hs.hs_chosen_to_caller(h, k, _p(ch), len(ch))
            assert np.array_equal(ch[:m], a["order"][:m]) and ch[m] == NONE and ch[m + 1] == NONE
            out.append(a)
        return out
    finally:
        hs.hs_plan_free(h)


def check_plan(d, groups, shards, nd, gmax=3):
    n, G = d["n"], len(groups)
    want = min(nd, max(G, 1))
    assert len(shards) == want
    listed = {c for g in groups for c in g if c < n}
    covered = set()
    for k, s in enumerate(shards):
        assert (s["gb"], s["ge"]) == (G * k // want, G * (k + 1) // want)
        assert s["whole"] == (want == 1)
        m, order = s["m"], [int(x) for x in s["order"][:s["m"]]]
        # the items: what the shard's groups list, each once, plus its share of the orphans
        mine = {c for g in groups[s["gb"]:s["ge"]] for c in g if c < n}
        mine |= {i for i in range(n) if i not in listed and i * want // n == k}
        assert sorted(order) == sorted(mine) and len(order) == len(mine)
        covered |= mine
        # verification order: by message, the table's bytes are the items', groups of <= gmax over one message
        midx = [int(x) for x in s["midx"][:m]]
        assert midx == sorted(midx) and (not midx or set(midx) == set(range(s["nm"])))
        for q in range(m):
            o, l = int(s["moff"][midx[q]]), int(s["mlen"][midx[q]])
            assert bytes(s["mbytes"][o:o + l]) == d["roots"][d["owner"][order[q]]]
        vg = [int(x) for x in s["vgoff"]]
        assert vg[0] == 0 and vg[-1] == m and len(vg) == s["nvg"] + 1
        for a, b in zip(vg, vg[1:]):
            assert 0 < b - a <= gmax and len(set(midx[a:b])) == 1
        # two neighbouring groups over one message: the first is full
        for g in range(1, s["nvg"]):
            if midx[vg[g]] == midx[vg[g] - 1]:
                assert vg[g] - vg[g - 1] == gmax
        # the candidates name the same partials
        goff = [int(x) for x in s["goff"]]
        base = sum(len(g) for g in groups[:s["gb"]])
        assert goff == [sum(len(g) for g in groups[:s["gb"] + j]) - base for j in range(s["ge"] - s["gb"] + 1)]
        assert s["nc"] == goff[-1]
        for j, g in enumerate(groups[s["gb"]:s["ge"]]):
            got = [int(x) for x in s["cand"][goff[j]:goff[j + 1]]]
            assert [order[q] if q < m else None for q in got] == [c if c < n else None for c in g]
    assert covered == set(range(n))  # every partial lands in at least one shard


@pytest.mark.parametrize("layout", ["validator", "peer"])
@pytest.mark.parametrize("nd", [1, 2, 3])
def test_plan(hs, layout, nd):
    d = duty(layout, orphans=7)
    V, n = d["V"], d["n"]
    groups = [list(g) for g in d["groups"]]
    check_plan(d, groups, plan(hs, d, groups, nd), nd)                 # orphans at the end of the call
    # a partial listed by the first and the last validator (two shards when there are several), an
    # empty group at each shard boundary, a candidate naming no partial, a partial listed twice
    groups[V - 1] = groups[V - 1] + [groups[0][1]]
    for k in range(1, nd):
        groups[V * k // nd] = []
    groups[2] = [groups[2][0], n + 5, NONE] + groups[2][1:] + [groups[2][0]]
    shards = plan(hs, d, groups, nd)
    check_plan(d, groups, shards, nd)
    if nd > 1:
        assert sum(int(groups[0][1]) in s["order"][:s["m"]] for s in shards) == 2
        assert all(s["goff"][0] == s["goff"][1] for s in shards[1:])  # the boundary groups are empty
    # gmax 1 (the small calls: every item its own group) and one above every message's item count
    for gmax in (1, 64):
        check_plan(d, groups, plan(hs, d, groups, nd, gmax), nd, gmax)


@pytest.mark.parametrize("layout", ["validator", "peer"])
def test_plan_more_shards_than_groups(hs, layout):
    d = duty(layout, V=2, orphans=3)
    for nd in (1, 2, 3):
        shards = plan(hs, d, d["groups"], nd)
        assert len(shards) == min(nd, 2)
        check_plan(d, d["groups"], shards, nd)
    # no groups at all: one shard, the whole call, every partial an orphan
    shards = plan(hs, d, [], 3)
    assert len(shards) == 1 and shards[0]["whole"] and shards[0]["m"] == d["n"] and shards[0]["nc"] == 0
    check_plan(d, [], shards, 3)
    # only empty groups
    check_plan(d, [[], [], []], plan(hs, d, [[], [], []], 2), 2)


def test_plan_without_partials(hs):
    d = dict(n=0, msgs=np.zeros(1, np.uint8), off=np.zeros(1, np.uint64), len=np.zeros(1, np.uint32), roots=[], owner=[])
    for nd in (1, 2):
        shards = plan(hs, d, [[], [0, NONE]], nd)
        check_plan(d, [[], [0, NONE]], shards, nd)
        assert all(s["m"] == 0 and s["nvg"] == 0 for s in shards)
