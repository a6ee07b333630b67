"""hbls_slot_select_device: one slot whose aggregation members are chosen from the verified partials
(parsigex.go:93-98 -> parsigdb/memory.go:198-225 -> sigagg.go:84-117), -m gpu.

Inputs are bench.setup_inputs clusters of 256 validators (four waves; 5 of 7 and 3 of 4, four
messages, one verification group per validator), every validator's n partials as its candidates in
share order.  The shares of a validator come from one polynomial, so every correct aggregate,
whatever its member set, equals root_sigs[v] byte for byte: the main oracle, with no tolerance.  The
expected members come from the rule restated in numpy (tests/gpu_helpers/slot_select.py rule), the
expected statuses from the construction.  All comparisons are exact.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from charon_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPERS = os.path.join(ROOT, "tests", "gpu_helpers")
for p in (ROOT, HELPERS):
    if p not in sys.path:
        sys.path.insert(0, p)

OK, BAD_PUBKEY, BAD_SIGNATURE, NOT_VERIFIED, COMBINE_FAILED, BAD_INPUT, UNCHECKED = 0, 1, 2, 3, 4, 6, 7
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def L(hipbls):
    return _lib.load_library()


@pytest.fixture(scope="module")
def ss():
    import slot_select
    return slot_select


@pytest.fixture(scope="module")
def clusters(L, ss):
    return {(7, 5): ss.inputs(L, 7, 5), (4, 3): ss.inputs(L, 4, 3)}


@pytest.fixture(scope="module")
def skipped(L, ss, clusters):
    """The second test's input and result per cluster, shared with the tests that reuse it."""
    out = {}
    for key, d in clusters.items():
        sigs, exp_v = ss.skip_case(L, d)
        out[key] = (sigs, exp_v, ss.run(L, d, sigs=sigs))
    return out


def first_t(d, V=None):
    n, t, V = d["n"], d["t"], d["V"] if V is None else V
    src = (np.arange(V)[:, None] * n + np.arange(t)[None, :]).reshape(-1).astype(np.uint32)
    return src, np.tile(np.arange(1, t + 1, dtype=np.int64), V), np.arange(V + 1, dtype=np.uint32) * t


def roots(d, V=None):
    return d["root_sigs"].reshape(d["V"], 96)[:d["V"] if V is None else V]


@pytest.mark.parametrize("key", [(7, 5), (4, 3)])
def test_select_clean(L, ss, clusters, key):
    d = clusters[key]
    V, t = d["V"], d["t"]
    r = ss.run(L, d)
    src, _, _ = first_t(d)
    assert np.array_equal(r["chosen"], src.reshape(V, t)) and np.array_equal(r["count"], np.full(V, t))
    assert np.array_equal(r["out"], roots(d))
    assert not r["vst"].any() and not r["tst"].any() and not r["ast"].any()
    f = ss.run(L, d, cand=first_t(d), select=False)
    for k in ("vst", "tst", "ast", "out"):
        assert np.array_equal(r[k], f[k]), k


@pytest.mark.parametrize("key", [(7, 5), (4, 3)])
def test_select_skips_bad_members(L, ss, clusters, skipped, key):
    from oracle import bls12381 as B
    d = clusters[key]
    V, n, t, NP = d["V"], d["n"], d["t"], d["NP"]
    sigs, exp_v, r = skipped[key]
    assert sorted(set(int(x) for x in exp_v)) == [OK, BAD_SIGNATURE, NOT_VERIFIED]
    src, idx, goff = ss.all_candidates(d)
    chosen, count, state = ss.rule(exp_v, d["midx"], src, idx, goff, t)
    assert not state.any() and np.array_equal(count, np.full(V, t))
    assert np.array_equal(r["vst"], exp_v)
    assert np.array_equal(r["chosen"], chosen) and np.array_equal(r["count"], count)
    assert np.array_equal(r["out"], roots(d))
    assert not r["tst"].any() and not r["ast"].any()
    if key == (7, 5):  # the oracle on one validator of each of the four member sets
        for v in (4, 5, 6, 7):
            members = {int(c) % n + 1: bytes(sigs[int(c)]) for c in r["chosen"][v]}
            st, agg = B.threshold_aggregate(members)
            assert st == OK and agg == bytes(r["out"][v]), v
            msg = bytes(d["msgs"].reshape(-1, 32)[d["midx"][v * n]])
            assert B.verify(bytes(d["dv_pks"][48 * v:48 * v + 48]), msg, agg) == OK, v
    # the gap: the fixed first-t members on the same bytes lose every validator with a corrupted member
    f = ss.run(L, d, sigs=sigs, cand=first_t(d), select=False)
    assert np.array_equal(f["vst"], exp_v)
    hit = np.arange(V) % 4 < 3
    assert (f["ast"][hit] != OK).all() and (f["ast"][~hit] == OK).all()


def test_select_threshold_edges(L, ss, clusters):
    d = clusters[(7, 5)]
    V, n, t, NP = d["V"], d["n"], d["t"], d["NP"]
    sigs = d["sigs"].reshape(NP, 96).copy()
    pks = d["pks"].copy()
    midx = d["midx"].copy()
    items = [(1 * n + 0, 2), (1 * n + 1, 0)]                               # v1: exactly t good, the last t
    items += [(2 * n + 0, 1), (2 * n + 2, 3), (2 * n + 4, 4)]              # v2: t - 1 good
    items += [(3 * n + k, k % 5) for k in range(n)]                        # v3: none good
    exp_v = ss.corrupt_at(L, d, sigs, items)
    pks[48 * (5 * n + 1):48 * (5 * n + 1) + 48] = 0xFF                     # v5: an undecodable key
    exp_v[5 * n + 1] = BAD_PUBKEY
    midx[7 * n + 3] = (midx[7 * n + 3] + 1) % d["M"]                       # v7: candidates over two messages
    exp_v[7 * n + 3] = NOT_VERIFIED
    src, idx, goff = [], [], [0]
    for v in range(V):
        c = list(range(v * n, v * n + n))
        x = list(range(1, n + 1))
        if v == 4:                                                         # v4: no candidates
            c, x = [], []
        if v == 6:                                                         # v6: a candidate listed twice
            c, x = [c[0], c[0]] + c[1:], [x[0], x[0]] + x[1:]
        if v == 8:                                                         # v8: share index 0 among the good
            x[1] = 0
        src += c
        idx += x
        goff.append(len(src))
    src, idx, goff = np.asarray(src, np.uint32), np.asarray(idx, np.int64), np.asarray(goff, np.uint32)
    r = ss.run(L, d, sigs=sigs, cand=(src, idx, goff), pks=pks, midx=midx)
    chosen, count, state = ss.rule(exp_v, midx, src, idx, goff, t)
    assert np.array_equal(r["vst"], exp_v)
    assert np.array_equal(r["chosen"], chosen) and np.array_equal(r["count"], count)
    assert list(r["chosen"][1]) == [n + 2, n + 3, n + 4, n + 5, n + 6]
    assert list(r["chosen"][2]) == [2 * n + 1, 2 * n + 3, 2 * n + 5, 2 * n + 6, NONE] and r["count"][2] == t - 1
    assert list(r["chosen"][3]) == [NONE] * t and r["count"][3] == 0
    assert list(r["chosen"][4]) == [NONE] * t and r["count"][4] == 0
    assert list(r["chosen"][5]) == [5 * n + 0, 5 * n + 2, 5 * n + 3, 5 * n + 4, 5 * n + 5]
    assert list(r["chosen"][6]) == [6 * n + k for k in range(t)]
    # v8: the status of the host ThresholdAggregate over the same members, not a constant
    m8 = np.ascontiguousarray(sigs[chosen[8]].reshape(-1))
    i8 = np.asarray([0 if k == 1 else k + 1 for k in range(t)], dtype=np.int64)
    o8, s8, g8 = np.zeros(96, np.uint8), np.zeros(1, np.uint8), np.asarray([0, t], np.uint32)
    ss.chk(L, L.hbls_threshold_aggregate_batch(ss._p(m8), ss._p(i8), ss._p(g8), 1, ss._p(o8), ss._p(s8)))
    assert s8[0] != OK
    exp_t = state.copy()
    exp_t[8] = s8[0]
    assert [int(exp_t[v]) for v in range(9)] == [OK, OK, UNCHECKED, UNCHECKED, UNCHECKED, OK, OK, BAD_INPUT, int(s8[0])]
    assert np.array_equal(r["tst"], exp_t) and np.array_equal(r["ast"], exp_t)
    exp_out = roots(d).copy()
    exp_out[exp_t != OK] = 0
    exp_out[8] = o8
    assert np.array_equal(r["out"], exp_out)


def test_select_orders_classes(L, ss, clusters):
    d = clusters[(7, 5)]
    V, n, t, NP = d["V"], d["n"], d["t"], d["NP"]
    sigs = d["sigs"].reshape(NP, 96).copy()
    items = [(v * n + (0 if v % 4 == 1 else 2), v % 5) for v in range(V) if v % 4 in (1, 3)]
    exp_v = ss.corrupt_at(L, d, sigs, items)
    _lib.slot_select_stats(L)  # reset
    r = ss.run(L, d, sigs=sigs)
    st = _lib.slot_select_stats(L)
    assert np.array_equal(r["vst"], exp_v) and np.array_equal(r["out"], roots(d))
    assert not r["tst"].any() and not r["ast"].any()
    # derived, not measured: three classes of 128, 64 and 64 validators, whole waves each once the
    # groups are in class order (in input order no wave of 64 is uniform), and share indices 1..7
    # pass ta_small_split
    assert st == dict(groups=256, too_few=0, shifted=128, small_path=256)
    assert _lib.slot_select_stats(L) == dict(groups=0, too_few=0, shifted=0, small_path=0)  # reset by reading
    # classes that are no multiples of the wave: results only
    r = ss.run(L, d, sigs=sigs, V=V - 1)
    st = _lib.slot_select_stats(L)
    assert np.array_equal(r["vst"], exp_v[:(V - 1) * n]) and np.array_equal(r["out"], roots(d, V - 1))
    assert not r["tst"].any() and not r["ast"].any()
    assert st["groups"] == V - 1 and 0 <= st["small_path"] <= V - 1
    print("small-path groups with classes of 128, 64 and 63:", st["small_path"])


def test_select_vgroups_independent(L, ss, clusters, skipped):
    d = clusters[(7, 5)]
    V, n = d["V"], d["n"]
    sigs, _, one = skipped[(7, 5)]
    two = np.sort(np.concatenate([np.arange(V + 1) * n, np.arange(V) * n + 3])).astype(np.uint32)
    for vgrp in (two, None):
        r = ss.run(L, d, sigs=sigs, vgrp=vgrp)
        for k in one:
            assert np.array_equal(r[k], one[k]), (k, None if vgrp is None else len(vgrp))


def _child(settings):
    """tests/gpu_helpers/slot_select.py in a process of its own under the given HBLS_* settings."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("HBLS_")}
    env.update(settings)
    p = subprocess.run([sys.executable, "-u", os.path.join(HELPERS, "slot_select.py")], env=env, capture_output=True,
                       text=True, timeout=240)
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert p.returncode == 0 and lines, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    res = json.loads(lines[-1])
    assert res["env"] == settings
    return res


def test_select_learned_keys_off_and_on(L, ss, clusters, skipped):
    d = clusters[(7, 5)]
    sigs, _, one = skipped[(7, 5)]
    want = ss.digest(one)
    res = _child({"HBLS_KEY_LEARN": "0"})
    assert res["key_learn"]["capacity"] == 0
    assert {k: res[k] for k in want} == want
    # warm: two calls back to back, the second finds every key learned
    before = _lib.key_learn_stats(L)[0]
    r = ss.run(L, d, sigs=sigs, calls=2)
    after = _lib.key_learn_stats(L)[0]
    assert ss.digest(r) == want
    assert after["hits"] - before["hits"] >= d["NP"] + d["V"]  # the second call's pubshares and DV keys


def test_select_one_workspace_set(ss, skipped):
    """HBLS_WS_SETS=1: the aggregates' verification takes the workspace set the partials' used."""
    want = ss.digest(skipped[(7, 5)][2])
    res = _child({"HBLS_WS_SETS": "1"})
    assert {k: res[k] for k in want} == want


def test_select_deferred_lines(L, ss):
    """Distinct messages per validator: the partials' pass defers the messages' Miller lines (128 or
    more verification groups, a message each), and the aggregates' pass either defers them too (256
    aggregates) or computes them first (100 aggregates: below the batched sizes).  The slot-wide
    check, whose chains are evaluated without stored lines, is lowered to these sizes; with corrupted
    partials it fails and the lines are computed behind it (then the adaptive history skips it)."""
    import bench
    d = bench.setup_inputs(L, dict(n=4, t=3, distinct=True, n_msgs=0), 256, 0)
    V, n, t = d["V"], d["n"], d["t"]
    assert d["M"] == V
    sigs, exp_v = ss.skip_case(L, d)
    prev = L.hbls_slot_msm(256)
    try:
        for G in (V, 100):
            src, idx, goff = ss.all_candidates(d, G)
            chosen, count, state = ss.rule(exp_v, d["midx"], src, idx, goff, t)
            for s in (d["sigs"].reshape(-1, 96), sigs):
                r = ss.run(L, d, sigs=s, cand=(src, idx, goff))
                assert np.array_equal(r["vst"], exp_v if s is sigs else np.zeros(V * n, np.uint8))
                assert np.array_equal(r["out"], roots(d, G)) and not r["tst"].any() and not r["ast"].any()
                if s is sigs:
                    assert not state.any() and np.array_equal(r["chosen"], chosen) and np.array_equal(r["count"], count)
    finally:
        L.hbls_slot_msm(prev)


def test_callers_sigagg_slot(L, ss, clusters, skipped, hipbls):
    from charon_amd import callers
    d = clusters[(7, 5)]
    V, n, t = 24, d["n"], d["t"]
    sigs, exp_v, one = skipped[(7, 5)]
    msgs = d["msgs"].reshape(-1, 32)
    dv = [bytes(d["dv_pks"][48 * v:48 * v + 48]) for v in range(V + 1)]
    shares = {dv[v]: {k + 1: bytes(d["pks"][48 * (v * n + k):48 * (v * n + k) + 48]) for k in range(n)}
              for v in range(V + 1)}
    sets = {dv[v]: [callers.ParSig(k + 1, bytes(msgs[d["midx"][v * n + k]]), bytes(sigs[v * n + k])) for k in range(n)]
            for v in range(V)}
    statuses, aggs, used = callers.sigagg_slot(hipbls, t, dict(zip(dv, dv)), shares, sets)
    for v in range(V):
        assert statuses[dv[v]] == [int(x) for x in exp_v[v * n:v * n + n]]
        assert used[dv[v]] == [int(c) - v * n for c in one["chosen"][v]]
        assert aggs[dv[v]] == bytes(roots(d)[v])
    # a validator below threshold (three of its partials replaced by another share's): the duty fails
    # with sigagg.go:86's text through the reference's wrap
    sets[dv[V]] = [callers.ParSig(k + 1, bytes(msgs[d["midx"][V * n + k]]),
                                  bytes(sigs[V * n + (k + 1 if k < 3 else k)]))
                   for k in range(n)]
    with pytest.raises(callers.CallerError, match="^threshold aggregate: require threshold signatures$"):
        callers.sigagg_slot(L, t, dict(zip(dv, dv)), shares, sets)
