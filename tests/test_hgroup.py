"""The host-buffer Verify calls' grouping (charon_amd/csrc/hgroup.h) on the CPU, through the g++
harness (tests/native/hostcheck.cpp hc_group_by_message, hc_group_runs, hc_split_chunks, ...).

Expected values never come from the header.  They come from two restatements and hand-written rows:

* rule_*: the rules as the header's callers state them -- a stable order by message id; a group
  starts at item 0, at a message change and when the current group holds gmax items; chunk
  boundary c is the first group starting at or after item n c / K, kept only beyond the previous
  boundary and below n_groups; offsets rebased to their first entry.
* parent_*: the loops that verify_large, verify_host and verify_first_host held inline before the
  header existed, transliterated statement by statement from charon_amd/csrc/hipbls.hip of commit
  87285e4 (line numbers at each), so the header is held to the rule the old code computed.  The
  one deliberate difference is named at parent_large_groups: verify_large read the limit unclamped
  on every iteration, where 0 made every item its own group exactly as 1 does.
"""
import bisect
import ctypes
import random

import numpy as np
import pytest

U32, U64 = np.uint32, np.uint64


@pytest.fixture(scope="module")
def hc():
    from gpu_helpers import harness
    lib = harness.load("hostcheck")
    P, Q = ctypes.c_void_p, ctypes.c_uint64
    for name, args, res in (("hc_call_gmax", [Q, Q, Q, Q], Q), ("hc_defer_lines", [Q, Q, Q], ctypes.c_int),
                            ("hc_group_by_message", [P, Q, Q, Q, P, P, P], Q), ("hc_group_runs", [P, Q, Q, P], Q),
                            ("hc_split_chunks", [P, Q, Q, P, P, P, P], Q), ("hc_rebase_offsets", [P, Q, Q, P], None)):
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, res
    return lib


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


# ---- the header, through the harness ----

def group_by_message(hc, idx, gmax):
    n, nm = len(idx), max(idx) + 1
    a = np.asarray(idx, dtype=U32)
    order, midx, gstart = np.zeros(n, U32), np.zeros(n, U32), np.zeros(n + 1, U64)
    ng = hc.hc_group_by_message(_p(a), n, nm, gmax, _p(order), _p(midx), _p(gstart))
    assert ng <= n
    return [int(x) for x in order], [int(x) for x in midx], [int(x) for x in gstart[:ng + 1]]


def group_runs(hc, idx, gmax):
    a = np.asarray(idx, dtype=U32)
    goff = np.zeros(len(idx) + 1, U32)
    ng = hc.hc_group_runs(_p(a), len(idx), gmax, _p(goff))
    assert ng <= len(idx)
    return [int(x) for x in goff[:ng + 1]]


def split_chunks(hc, gstart, K):
    ng = len(gstart) - 1
    gs = np.asarray(gstart, dtype=U64)
    cg, base, goffs, ngo = np.zeros(K + 1, U64), np.zeros(K, U64), np.zeros(ng + K, U32), ctypes.c_uint64(0)
    nc = hc.hc_split_chunks(_p(gs), ng, K, _p(cg), _p(base), _p(goffs), ctypes.byref(ngo))
    assert 1 <= nc <= K and ngo.value <= ng + K
    return [int(x) for x in cg[:nc + 1]], [int(x) for x in goffs[:ngo.value]], [int(x) for x in base[:nc]]


def call_gmax(hc, n, gmax, single_max=0, fe_min=0):
    return int(hc.hc_call_gmax(n, single_max, fe_min, gmax))


# ---- the rules ----

def rule_split(mids, gmax):
    """Group starts over a sequence of message ids, then its length."""
    start = []
    for k, m in enumerate(mids):
        if k == 0 or m != mids[k - 1] or k - start[-1] == gmax:
            start.append(k)
    return start + [len(mids)]


def rule_by_message(idx, gmax):
    order = sorted(range(len(idx)), key=lambda k: (idx[k], k))
    midx = [idx[k] for k in order]
    return order, midx, rule_split(midx, gmax)


def rule_chunks(gstart, K):
    ng, n = len(gstart) - 1, gstart[-1]
    cg = [0]
    for c in range(1, K):
        g = bisect.bisect_left(gstart, n * c // K, 0, ng)
        if cg[-1] < g < ng:
            cg.append(g)
    cg.append(ng)
    goffs, base = [], []
    for a, b in zip(cg, cg[1:]):
        base.append(len(goffs))
        goffs += [gstart[g] - gstart[a] for g in range(a, b + 1)]
    return cg, goffs, base


# ---- the parent's loops (hipbls.hip of 87285e4) ----

def parent_large_groups(idx, nm, g_gmax):
    """verify_large, lines 2111-2122.  g_gmax is what g_gmax.load() returned, read on every
    iteration and unclamped there: the header's callers clamp it once (0 groups as 1 does)."""
    n = len(idx)
    order32, mstart = [0] * n, [0] * (nm + 1)                                        # 2111
    for k in range(n):                                                               # 2112
        mstart[idx[k] + 1] += 1
    for j in range(nm):                                                              # 2113
        mstart[j + 1] += mstart[j]
    for k in range(n):                                                               # 2114
        order32[mstart[idx[k]]] = k
        mstart[idx[k]] += 1
    gstart, midx = [], [0] * n                                                       # 2115-2116
    for k in range(n):                                                               # 2117
        midx[k] = idx[order32[k]]                                                    # 2118
        if k == 0 or midx[k] != midx[k - 1] or k - gstart[-1] >= g_gmax:             # 2119
            gstart.append(k)
    n_groups = len(gstart)                                                           # 2121
    gstart.append(n)                                                                 # 2122
    return order32, midx, gstart, n_groups


def parent_large_chunks(gstart, n_groups, n, K):
    """verify_large, lines 2140-2152."""
    cg = [0]                                                                         # 2140
    for c in range(1, K):                                                            # 2141
        g = bisect.bisect_left(gstart, n * c // K, 0, n_groups)                      # 2142 (std::lower_bound)
        if g > cg[-1] and g < n_groups:                                              # 2143
            cg.append(g)
    cg.append(n_groups)                                                              # 2145
    goffs, goff_base = [], []                                                        # 2147-2148
    for c in range(len(cg) - 1):                                                     # 2149
        goff_base.append(len(goffs))                                                 # 2150
        for g in range(cg[c], cg[c + 1] + 1):                                        # 2151
            goffs.append(gstart[g] - gstart[cg[c]])
    return cg, goffs, goff_base


def parent_host_groups(idx, nm, n, g_single_max, g_fe_batch_min, g_gmax):
    """verify_host, lines 2258-2261 (the order) and 2268-2275 (the limit and the group starts);
    SINGLE_MAX_DEFAULT is ~size_t(0) (line 298)."""
    order, mstart = [0] * n, [0] * (nm + 1)                                          # 2258
    for k in range(n):                                                               # 2259
        mstart[idx[k] + 1] += 1
    for j in range(nm):                                                              # 2260
        mstart[j + 1] += mstart[j]
    for k in range(n):                                                               # 2261
        order[mstart[idx[k]]] = k
        mstart[idx[k]] += 1
    sm = g_single_max                                                                # 2268
    single_max = g_fe_batch_min if sm == 2**64 - 1 else sm                           # 2269
    gmax = 1 if n < single_max else max(1, g_gmax)                                   # 2270
    gstart = []                                                                      # 2271
    for k in range(n):                                                               # 2272
        if k == 0 or idx[order[k]] != idx[order[k - 1]] or k - gstart[-1] >= gmax:   # 2273
            gstart.append(k)
    n_groups = len(gstart)                                                           # 2274
    gstart.append(n)                                                                 # 2275
    return order, gstart, n_groups, gmax


def parent_host_shard_offsets(gstart, gb, ge):
    """verify_host's lambda, lines 2280 and 2306-2307."""
    ib = gstart[gb]                                                                  # 2280
    goff = [0] * (ge - gb + 1)                                                       # 2306
    for g in range(gb, ge + 1):                                                      # 2307
        goff[g - gb] = gstart[g] - ib
    return goff


def parent_first_groups(idx, n, g_gmax):
    """verify_first_host, lines 2397-2402."""
    goff = []                                                                        # 2397
    for k in range(n):                                                               # 2398
        if k == 0 or idx[k] != idx[k - 1] or k - goff[-1] >= max(1, g_gmax):         # 2399
            goff.append(k)                                                           # 2400
    n_groups = len(goff)                                                             # 2401
    goff.append(n)                                                                   # 2402
    return goff, n_groups


def parent_defer_lines(n_groups, n_msgs, fe_min):
    """defer_lines, lines 1765-1768."""
    return bool(fe_min and n_groups >= fe_min and n_groups <= n_msgs)                # 1767


# ---- the cases ----

def _dense(idx):
    """The same partition with ids numbered in first-occurrence order (as dedup_messages assigns them)."""
    ids = {}
    return [ids.setdefault(m, len(ids)) for m in idx]


def _random_vectors():
    rng = random.Random(20240611)
    out = []
    for _ in range(300):
        n, nm = rng.randint(1, 300), rng.randint(1, 40)
        if rng.random() < 0.5:  # runs of one message, as a validator's partials arrive
            idx = []
            while len(idx) < n:
                idx += [rng.randrange(nm)] * rng.randint(1, 12)
            idx = idx[:n]
        else:
            idx = [rng.randrange(nm) for _ in range(n)]
        out.append((_dense(idx), rng.choice([1, 2, 3, 5, 16, 64, n, n + 1])))
    return out


RANDOM = _random_vectors()
N1 = 7
NAMED = [
    ("one item", [0], 16),
    ("one message, gmax 1", [0] * N1, 1),
    ("one message, gmax 2", [0] * N1, 2),
    ("one message, gmax n - 1", [0] * N1, N1 - 1),
    ("one message, gmax n", [0] * N1, N1),
    ("one message, gmax n + 1", [0] * N1, N1 + 1),
    ("n = gmax + 1", [0] * 17, 16),
    ("alternating", [0, 1] * 6, 4),
    ("sorted", [0, 0, 0, 1, 1, 2, 2, 2, 2, 3], 3),
    ("descending", [4, 4, 3, 3, 3, 2, 1, 1, 0, 0, 0], 2),
]
# by hand: (idx, gmax) -> (order, gstart)
HAND_BY_MESSAGE = [
    ([0], 16, [0], [0, 1]),
    ([0] * 5, 2, [0, 1, 2, 3, 4], [0, 2, 4, 5]),
    ([0, 1, 0, 1, 0], 16, [0, 2, 4, 1, 3], [0, 3, 5]),
    ([2, 1, 0], 16, [2, 1, 0], [0, 1, 2, 3]),
    ([1, 0, 1, 1, 0, 1], 2, [1, 4, 0, 2, 3, 5], [0, 2, 4, 6]),
]
# by hand: (idx, gmax) -> offsets
HAND_RUNS = [
    ([0, 1, 0], 16, [0, 1, 2, 3]),  # A B A: three groups, no sort
    ([0, 0, 0], 2, [0, 2, 3]),
    ([0], 16, [0, 1]),
    ([0, 0, 1, 1, 1, 1, 1, 0], 3, [0, 2, 5, 7, 8]),
]


def _check_by_message(hc, idx, gmax):
    n = len(idx)
    order, midx, gstart = group_by_message(hc, idx, gmax)
    assert sorted(order) == list(range(n))  # a permutation
    for a, b in zip(order, order[1:]):  # by message, stable: caller indices ascend within one
        assert (idx[a], a) < (idx[b], b)
    assert midx == [idx[k] for k in order]
    assert gstart[0] == 0 and gstart[-1] == n
    for a, b in zip(gstart, gstart[1:]):  # every group: one message, 1 .. gmax items
        assert 1 <= b - a <= gmax and len(set(midx[a:b])) == 1
    assert (order, midx, gstart) == rule_by_message(idx, gmax)
    nm = max(idx) + 1
    p_order, p_midx, p_gstart, p_ng = parent_large_groups(idx, nm, gmax)
    assert (order, midx, gstart, len(gstart) - 1) == (p_order, p_midx, p_gstart, p_ng)
    h_order, h_gstart, h_ng, _ = parent_host_groups(idx, nm, n, 0, 0, gmax)
    assert (order, gstart, len(gstart) - 1) == (h_order, h_gstart, h_ng)
    return gstart


@pytest.mark.parametrize("name,idx,gmax", NAMED, ids=[c[0] for c in NAMED])
def test_by_message_named(hc, name, idx, gmax):
    _check_by_message(hc, idx, gmax)


def test_by_message_by_hand(hc):
    for idx, gmax, order, gstart in HAND_BY_MESSAGE:
        assert group_by_message(hc, idx, gmax) == (order, [idx[k] for k in order], gstart), (idx, gmax)


def test_by_message_random(hc):
    for idx, gmax in RANDOM:
        _check_by_message(hc, idx, gmax)


def test_group_limit_is_clamped_once_by_the_caller(hc):
    """gmax 0 through the caller's clamp groups as 1 does -- what the parent's unclamped loop gave."""
    assert call_gmax(hc, 100, 0) == 1 and call_gmax(hc, 100, 1) == 1 and call_gmax(hc, 100, 16) == 16
    for idx in ([0] * 6, [0, 0, 1, 1, 1, 0]):
        idx = _dense(idx)
        got = group_by_message(hc, idx, call_gmax(hc, len(idx), 0))
        assert got == rule_by_message(idx, 1) and got[2] == list(range(len(idx) + 1))
        assert got[:3] == parent_large_groups(idx, max(idx) + 1, 0)[:3]  # the unclamped 0 of the old loop
        assert group_runs(hc, idx, call_gmax(hc, len(idx), 0)) == parent_first_groups(idx, len(idx), 0)[0]


def test_call_gmax_and_defer_lines(hc):
    """single_max -> gmax (n < single_max: every item alone; the default is the batched final
    exponentiation's threshold) and defer_lines, against the parent's expressions."""
    dflt = 2**64 - 1
    assert call_gmax(hc, 127, 16, dflt, 128) == 1 and call_gmax(hc, 128, 16, dflt, 128) == 16  # by hand
    assert call_gmax(hc, 5, 16, 0, 128) == 16 and call_gmax(hc, 5, 16, 6, 128) == 1
    for n in (1, 2, 127, 128, 129, 4096):
        for sm in (dflt, 0, 1, 128, 5000):
            for fe in (0, 1, 128, 40_000):
                for gm in (0, 1, 16):
                    assert call_gmax(hc, n, gm, sm, fe) == parent_host_groups([0] * n, 1, n, sm, fe, gm)[3]
    assert hc.hc_defer_lines(128, 128, 128) == 1 and hc.hc_defer_lines(127, 128, 128) == 0  # by hand
    assert hc.hc_defer_lines(129, 128, 128) == 0 and hc.hc_defer_lines(500, 500, 0) == 0
    for ng in (0, 1, 127, 128, 129, 53_000):
        for nm in (1, 128, 129, 53_000):
            for fe in (0, 1, 128, 40_000):
                assert bool(hc.hc_defer_lines(ng, nm, fe)) == parent_defer_lines(ng, nm, fe), (ng, nm, fe)


def test_runs(hc):
    for idx, gmax, goff in HAND_RUNS:
        assert group_runs(hc, idx, gmax) == goff, (idx, gmax)
    for idx, gmax in RANDOM + [(c[1], c[2]) for c in NAMED]:
        goff = group_runs(hc, idx, gmax)
        assert goff == rule_split(idx, gmax)
        assert (goff, len(goff) - 1) == parent_first_groups(idx, len(idx), gmax)
        for a, b in zip(goff, goff[1:]):
            assert 1 <= b - a <= gmax and len(set(idx[a:b])) == 1


def _check_chunks(hc, gstart, K):
    ng, n = len(gstart) - 1, gstart[-1]
    cg, goffs, base = split_chunks(hc, gstart, K)
    gs = np.asarray(gstart, dtype=U64)
    assert cg[0] == 0 and cg[-1] == ng and all(a < b for a, b in zip(cg, cg[1:]))  # strictly increasing
    assert len(base) == len(cg) - 1 and len(goffs) == ng + len(base)
    for c, (a, b) in enumerate(zip(cg, cg[1:])):
        mine = goffs[base[c]:base[c] + (b - a) + 1]  # goff_base indexes the chunk's offsets
        assert mine[0] == 0 and mine[-1] == gstart[b] - gstart[a]  # from 0 to the chunk's item count
        assert mine == [gstart[g] - gstart[a] for g in range(a, b + 1)]
        assert mine == parent_host_shard_offsets(gstart, a, b)
        out = np.zeros(b - a + 1, U32)
        hc.hc_rebase_offsets(_p(gs), a, b, _p(out))  # the shard helper, the same rule
        assert [int(x) for x in out] == mine
    assert (cg, goffs, base) == rule_chunks(gstart, K)
    assert (cg, goffs, base) == parent_large_chunks(gstart, ng, n, K)
    return cg


def test_chunk_split_named(hc):
    even = list(range(0, 41, 4))  # 10 groups of 4 items
    assert _check_chunks(hc, even, 1) == [0, 10]  # K = 1
    assert _check_chunks(hc, even, 2) == [0, 5, 10]
    assert _check_chunks(hc, [0, 3, 6], 8) == [0, 1, 2]  # K larger than n_groups: one group per chunk at most
    assert _check_chunks(hc, [0, 5], 4) == [0, 1]
    # a target inside a group (item 10 of 20, in group [8, 14)): the boundary is the next group start
    assert _check_chunks(hc, [0, 4, 8, 14, 20], 2) == [0, 3, 4]
    # two targets (items 10 and 20 of 30) in the one group [2, 28): one boundary
    assert _check_chunks(hc, [0, 2, 28, 30], 3) == [0, 2, 3]
    # one huge group, then small ones: every target lands in it, one boundary behind it
    assert _check_chunks(hc, [0, 90, 92, 94, 96, 98, 100], 4) == [0, 1, 6]
    # a target in the last group: no boundary at n_groups
    assert _check_chunks(hc, [0, 1, 2, 30], 2) == [0, 3]


def test_chunk_split_random(hc):
    rng = random.Random(7)
    for _ in range(400):
        ng = rng.randint(1, 60)
        sizes = [rng.choice([1, 1, 2, 3, 16, rng.randint(1, 200)]) for _ in range(ng)]
        gstart = [0]
        for s in sizes:
            gstart.append(gstart[-1] + s)
        for K in range(1, 9):
            _check_chunks(hc, gstart, K)
    for idx, gmax in RANDOM[:100]:  # and over real groupings
        gstart = group_by_message(hc, idx, gmax)[2]
        for K in (1, 2, 3, 8):
            _check_chunks(hc, gstart, K)
