"""Set-atomic duty adds through the ABI (hbls_duty_add_sets / hbls_duty_set_stats), -m gpu: a peer's
set is stored whole or not at all.

Inputs are the clusters and streams of tests/test_gpu_duty.py (256 validators, 5 of 7 and 3 of 4).
The reference is the defining property of include/hipbls.h: the call equals hbls_duty_add on a twin
duty fed the same partials in the same calls with group 0xffffffff for every partial of a rejected
set (tests/gpu_helpers/duty_sets.py run_pair), plus the construction (root_sigs) and set_first
restated from vstatus.  Every comparison is exact.
"""
import ctypes
import os
import sys
import threading

import numpy as np
import pytest

from charon_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPERS = os.path.join(ROOT, "tests", "gpu_helpers")
for p in (ROOT, HELPERS, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

OK, NOT_VERIFIED, UNCHECKED = 0, 3, 7
NONE = 0xFFFFFFFF

from test_gpu_duty import L, clusters, dh, sh, ss, streams  # noqa: E402,F401 -- its fixtures: the same clusters and streams


@pytest.fixture(scope="module")
def ds():
    import duty_sets
    return duty_sets


def corrupted(s, at, by):
    """the stream with partial `at` carrying partial `by`'s signature: a point of G2 that verifies nothing here"""
    sigs = s["sigs"].copy()
    sigs[at] = s["sigs"][by]
    return dict(s, sigs=sigs)


# 1
def test_peer_major_clean_one_set_per_call(L, ds, clusters, streams):
    for key, d in clusters.items():
        s, _ = streams["clean", key]
        V, n, t = d["V"], d["n"], d["t"]
        bounds = [k * V for k in range(n + 1)]
        r = ds.run_pair(L, s, bounds, [[0, V]] * n)
        assert all(sf.tolist() == [NONE] for sf in r["set_first"])
        assert r["set_stats"] == [n, 0, 0]
        assert [len(c["fired"]) for c in r["calls"]] == [0] * (t - 1) + [V] + [0] * (n - t)
        assert np.array_equal(r["calls"][t - 1]["out"], d["root_sigs"].reshape(V, 96))
        assert r["stats"][:2] == [n * V, t * V]


# 2
def test_one_corrupted_partial_rejects_its_peers_set(L, ds, clusters, streams):
    d = clusters[(7, 5)]
    s0, _ = streams["clean", (7, 5)]
    V, n, t = d["V"], d["n"], d["t"]
    bad = 2 * V + 77
    s = corrupted(s0, bad, bad + 1)
    bounds = [k * V for k in range(n + 1)]
    r = ds.run_pair(L, s, bounds, [[0, V]] * n)
    assert [sf.tolist() for sf in r["set_first"]] == [[NONE]] * 2 + [[77]] + [[NONE]] * 4, "set_first names it"
    c2 = r["calls"][2]
    assert c2["vst"][77] == NOT_VERIFIED and (np.delete(c2["vst"], 77) == OK).all()
    assert not c2["stored"].any(), "nothing of peer 2 is stored"
    assert [len(c["fired"]) for c in r["calls"]] == [0, 0, 0, 0, 0, V, 0], "every validator fires through peer 5's set"
    c5 = r["calls"][5]
    assert np.array_equal(c5["out"], d["root_sigs"].reshape(V, 96)) and not c5["tst"].any() and not c5["ast"].any()
    members = np.asarray([0, 1, 3, 4, 5])[None, :] * V + np.arange(V)[:, None]
    assert np.array_equal(c5["chosen"], members), "peers 0, 1, 3, 4 and 5"
    assert (r["count"] == 5).all() and r["flag"].all()
    assert r["set_stats"] == [7, 1, 255]
    assert r["stats"][:2] == [n * V, 5 * V] and r["stats"][4:] == [V, 0]


def set_cuts(bounds, S, seed, small_until=3 * 256):
    """Sets cut independently of the calls: global boundaries (runs of singletons, spans of a few hundred
    partials, repeated boundaries for empty sets), clipped to each call -> per call, offsets relative to it.
    The corrupted stream's first three peers carry a bad partial every fourth validator, its last four
    almost none: short sets over the former and long ones over the latter leave sets of both kinds admitted
    and rejected, and validators that still reach the threshold."""
    rng = np.random.default_rng(seed)
    cuts, x = [], 0
    while x < S:
        x += int(rng.choice([1, 2, 2, 3, 3, 3, 3, 10] if x < small_until else [1, 2, 30, 70, 150, 300]))
        cuts += [min(x, S)] * int(rng.choice([1, 1, 1, 2, 3]))
    out = []
    for k in range(len(bounds) - 1):
        lo, hi = bounds[k], bounds[k + 1]
        inner = [c - lo for c in cuts if lo < c < hi]
        lead = [0] * int(rng.integers(0, 3))  # empty sets first and last, too
        out.append([0] + lead + inner + [hi - lo] * (1 + int(rng.integers(0, 3))))
    return out


# 3
@pytest.mark.parametrize("n_calls", [1, 2, 5, 37])
def test_defining_property_against_a_twin(L, dh, ds, streams, n_calls):
    s, _ = streams["corrupt", (7, 5)]
    S = len(s["pks"])
    bounds = dh.random_cuts(S, n_calls, seed=2000 + n_calls)
    sets = set_cuts(bounds, S, seed=3000 + n_calls)
    sizes = np.concatenate([np.diff(o) for o in sets])
    spans = [(bounds[k] + o[j], bounds[k] + o[j + 1]) for k, o in enumerate(sets) for j in range(len(o) - 1)]
    assert (sizes == 0).any() and (sizes == 1).any(), "empty sets and sets of one partial"
    assert any(e > b and (b - bounds[k]) // 64 != (e - 1 - bounds[k]) // 64
               for k, o in enumerate(sets) for b, e in [(bounds[k] + o[j], bounds[k] + o[j + 1]) for j in range(len(o) - 1)]), \
        "sets that span 64-item boundaries of their call"
    r = ds.run_pair(L, s, bounds, sets)
    n_rej = sum(int((sf != NONE).sum()) for sf in r["set_first"])
    assert r["set_stats"][0] == len(spans) and 0 < n_rej == r["set_stats"][1] < (sizes > 0).sum(), "some sets rejected, some admitted"
    assert r["set_stats"][2] > 0 and r["flag"].any() and not r["flag"].all()


# 4
def test_singleton_sets_equal_plain_adds(L, dh, ds, streams):
    s, _ = streams["corrupt", (7, 5)]
    S = len(s["pks"])
    bounds = dh.random_cuts(S, 3, seed=44)
    a, b = ds.SetsDuty(L, s["dv"], s["t"], 16), ds.SetsDuty(L, s["dv"], s["t"], 16)
    try:
        bad = 0
        for k in range(3):
            lo, hi = bounds[k], bounds[k + 1]
            r = a.add_sets(s, lo, hi, list(range(hi - lo + 1)))
            ds.same_call(r, b.add(s, lo, hi), k)  # the stream as it is: a singleton's rejection is its own verdict
            assert np.array_equal(r["set_first"] != NONE, r["vst"] != OK)
            assert np.array_equal(r["set_first"][r["vst"] != OK], np.flatnonzero(r["vst"] != OK))
            bad += int((r["vst"] != OK).sum())
        assert all(np.array_equal(x, y) for x, y in zip(a.state(), b.state())) and a.stats() == b.stats()
        assert a.set_stats() == [S, bad, 0] and bad > 0
    finally:
        a.close()
        b.close()


# 5
def test_several_peers_sets_in_one_call_the_middle_one_rejected(L, ds, clusters, streams):
    d = clusters[(4, 3)]
    s0, _ = streams["clean", (4, 3)]
    V, n, t = d["V"], d["n"], d["t"]
    s = corrupted(s0, V + 200, V + 5)
    r = ds.run_pair(L, s, [0, n * V], [[k * V for k in range(n + 1)]])
    c = r["calls"][0]
    assert c["set_first"].tolist() == [NONE, V + 200, NONE, NONE]
    assert c["stored"][:V].all() and not c["stored"][V:2 * V].any() and c["stored"][2 * V:].all(), "the sets after it are stored"
    assert c["fired"].tolist() == list(range(V)), "and fire: through peer 3's set"
    assert np.array_equal(c["chosen"], np.asarray([0, 2, 3])[None, :] * V + np.arange(V)[:, None])
    assert np.array_equal(c["out"], d["root_sigs"].reshape(V, 96)) and not c["tst"].any() and not c["ast"].any()
    assert r["set_stats"] == [4, 1, V - 1] and (r["count"] == 3).all()


# 6
def test_add_and_add_sets_interleaved(L, ds, clusters, streams):
    d = clusters[(7, 5)]
    s0, _ = streams["clean", (7, 5)]
    V, n, t = d["V"], d["n"], d["t"]
    s = corrupted(s0, 3 * V, 3 * V + 1)  # the first partial of peer 3's set
    bounds = [k * V for k in range(n + 1)]
    modes = ["add", "sets", "add", "sets", "add", "sets", "add"]
    r = ds.run_pair(L, s, bounds, [[0, 100, V]] * n, modes=modes)
    assert r["set_first"][3].tolist() == [0, NONE], "peer 3 in two sets: the first is rejected, the second stored"
    assert r["calls"][3]["stored"].tolist() == [0] * 100 + [1] * (V - 100)
    fired = [c["fired"].tolist() for c in r["calls"]]
    assert fired[4] == list(range(100, V)) and fired[5] == list(range(100)) and not any(fired[k] for k in (0, 1, 2, 3, 6))
    assert np.array_equal(np.concatenate([r["calls"][5]["out"], r["calls"][4]["out"]]), d["root_sigs"].reshape(V, 96))
    assert r["set_stats"] == [6, 1, 99] and r["stats"][0] == n * V


# 7
@pytest.mark.parametrize("copies", [2, 3])
def test_device_split(L, dh, ds, clusters, streams, copies):
    d = clusters[(7, 5)]
    V, n = d["V"], d["n"]
    s0, _ = streams["clean", (7, 5)]
    # the failing partial is validator 3's (the first shard's); what would have been stored lies on every shard
    sa, ba, seta = corrupted(s0, 2 * V + 3, 2 * V + 4), [k * V for k in range(n + 1)], [[0, V]] * n
    sb, _ = streams["corrupt", (7, 5)]
    bb = dh.random_cuts(len(sb["pks"]), 5, seed=71)
    setb = set_cuts(bb, len(sb["pks"]), seed=72)
    devices = L.hbls_device_count()
    want = [ds.run_pair(L, sa, ba, seta), ds.run_pair(L, sb, bb, setb)]
    assert want[0]["set_first"][2].tolist() == [3] and want[0]["set_stats"] == [7, 1, 255]
    try:
        assert L.hbls_debug_split(copies) == 0 and L.hbls_device_count() == copies * devices
        got = [ds.run_pair(L, sa, ba, seta), ds.run_pair(L, sb, bb, setb)]
    finally:
        assert L.hbls_debug_split(1) == 0
    for w, g in zip(want, got):
        for x, y in zip(w["calls"], g["calls"]):
            ds.same_call(x, y)
        assert all(np.array_equal(x, y) for x, y in zip(w["set_first"], g["set_first"]))
        assert np.array_equal(w["count"], g["count"]) and np.array_equal(w["flag"], g["flag"])
        assert w["set_stats"] == g["set_stats"] and w["stats"][:2] + w["stats"][4:] == g["stats"][:2] + g["stats"][4:]
    assert not got[0]["calls"][2]["stored"].any() and (got[0]["count"] == 5).all()


# 7b: concurrent calls on duties of several shards: every call takes one host-call context per shard from a
# pool of a few per device, the two-phase path across its join; they must not wait for each other in a circle
def test_concurrent_duties_on_several_shards(L, dh, ds, clusters, streams):
    d = clusters[(7, 5)]
    V, n = d["V"], d["n"]
    s0, _ = streams["clean", (7, 5)]
    sb, _ = streams["corrupt", (7, 5)]
    jobs = []
    for k in range(6):
        if k % 2:
            b = dh.random_cuts(len(sb["pks"]), 4 + k, seed=80 + k)
            jobs.append((sb, b, set_cuts(b, len(sb["pks"]), seed=90 + k)))
        else:
            jobs.append((corrupted(s0, k * V + 3, k * V + 4), [j * V for j in range(n + 1)], [[0, V]] * n))
    res, errs = [None] * len(jobs), []

    def drive(k):
        try:
            res[k] = ds.run_pair(L, *jobs[k])
        except BaseException as e:  # noqa: BLE001
            errs.append((k, e))

    try:
        assert L.hbls_debug_split(2) == 0
        want = [ds.run_pair(L, *j) for j in jobs]
        th = [threading.Thread(target=drive, args=(k,), daemon=True) for k in range(len(jobs))]
        for x in th:
            x.start()
        for x in th:
            x.join(timeout=120)
        assert not any(x.is_alive() for x in th), "the calls wait for each other"
    finally:
        assert L.hbls_debug_split(1) == 0
    assert not errs, errs
    for w, g in zip(want, res):
        for x, y in zip(w["calls"], g["calls"]):
            ds.same_call(x, y)
        assert np.array_equal(w["count"], g["count"]) and np.array_equal(w["flag"], g["flag"]) and w["set_stats"] == g["set_stats"]


# 8
def test_call_errors(L, ds, streams):
    s, _ = streams["clean", (4, 3)]
    V = 256
    du = ds.SetsDuty(L, s["dv"], s["t"], 8)

    def err(rc):
        return rc, L.hbls_last_error().decode()

    pre = "hbls_duty_add_sets: "
    try:
        du.add_sets(s, 0, V, [0, 10, V])
        before = (du.state()[0].tolist(), du.state()[1].tolist(), du.stats(), du.set_stats())
        assert before[2][:2] == [V, V] and before[3] == [2, 0, 0]
        n = 5
        for off, msg in (([1, 2, n], "set_off[0] must be 0"), ([0, 4, 3, n], "set_off must not decrease"),
                         ([0, 2, 4], "set_off[n_sets] must be n"), ([0, 2, n + 1], "set_off[n_sets] must be n"),
                         ([0], "n_sets is 0 with partials in the call")):
            assert err(du.add_sets(s, V, V + n, off, raw=True)) == (-1, pre + msg), off
        assert err(du.add_sets(s, V, V + n, None, raw=True, n_sets=2)) == (-1, pre + "set_off is required")
        assert err(du.add_sets(s, V, V + n, None, raw=True, n_sets=0)) == (-1, pre + "n_sets is 0 with partials in the call")
        assert err(du.add_sets(s, V, V + n, [0, 2, n], raw=True, no_set_first=True)) == (-1, pre + "set_first is required")
        none = "no such duty (never opened, or closed)"
        out = np.zeros(4, np.uint64)
        p = ctypes.c_void_p(out.ctypes.data)
        for bad in (0, du.h + 1000):
            assert err(du.add_sets(s, V, V + n, [0, 2, n], raw=True, handle=bad)) == (-1, pre + none)
            assert err(L.hbls_duty_set_stats(bad, p, 1)) == (-1, "hbls_duty_set_stats: " + none)
        assert err(L.hbls_duty_set_stats(du.h, p, 4)) == (-1, "hbls_duty_set_stats: out is null or n above 3")
        assert err(L.hbls_duty_set_stats(du.h, None, 1)) == (-1, "hbls_duty_set_stats: out is null or n above 3")
        assert not out.any()
        # nothing was verified, stored or numbered
        assert (du.state()[0].tolist(), du.state()[1].tolist(), du.stats(), du.set_stats()) == before
        r = du.add_sets(s, V, V + n, [0, 0, 2, n, n])  # the next serial is unchanged; empty sets count as seen
        assert r["first"] == V and r["set_first"].tolist() == [NONE] * 4 and du.set_stats() == [6, 0, 0]
        r = du.add_sets(s, V + n, V + n, [0, 0])  # no partials: one empty set
        assert r["first"] == V + n and r["set_first"].tolist() == [NONE] and du.set_stats() == [7, 0, 0]
        assert du.add_sets(s, V + n, V + n, [0])["first"] == V + n and du.set_stats() == [7, 0, 0]
    finally:
        closed = du.h
        du.close()
    assert err(du.add_sets(s, V, V + 5, [0, 2, 5], raw=True, handle=closed)) == (-1, pre + "no such duty (never opened, or closed)")
    out = np.zeros(3, np.uint64)
    assert err(L.hbls_duty_set_stats(closed, ctypes.c_void_p(out.ctypes.data), 3)) == \
        (-1, "hbls_duty_set_stats: no such duty (never opened, or closed)")


# 9: the Python layers
def test_parsig_duty_reject_sets(hipbls, ss, sh, clusters):
    from charon_amd import callers
    d = clusters[(4, 3)]
    V, n, t = 16, d["n"], d["t"]
    c = sh.case(ss, d)
    keys = [bytes(c["dv"][v]) for v in range(V)]
    shares = {keys[v]: {s + 1: bytes(c["pks"][v * n + s]) for s in range(n)} for v in range(V)}
    root_sigs = d["root_sigs"].reshape(-1, 96)
    not_verified = "^invalid partial signature: invalid signature: signature not verified$"

    def peer_set(s, vs=range(V)):
        return {keys[v]: callers.ParSig(s + 1, bytes(c["msgs"][v * n + s]), bytes(c["sigs"][v * n + s])) for v in vs}

    def spoiled(s, v):
        bad = peer_set(s)
        bad[keys[v]] = callers.ParSig(s + 1, bad[keys[v]].signing_root, bad[keys[(v + 1) % V]].signature)
        return bad

    with callers.ParSigDuty(hipbls, t, {k: k for k in keys}, shares, reject_sets=True) as du:
        for s in range(t - 1):
            assert du.store_external(peer_set(s)) == {}
        before = du.state()
        # the reference's rule: the set with a failing entry stores nothing, fires nothing, changes nothing
        with pytest.raises(callers.CallerError, match=not_verified) as ei:
            du.store_external(spoiled(t - 1, 2))
        assert ei.value.fired == {} and du.state() == before == {k: (t - 1, False) for k in keys}
        with pytest.raises(callers.CallerError, match="^invalid partial signature: unknown pubkey, not part of cluster lock$"):
            du.store_external({bytes(48): peer_set(0)[keys[0]]})
        with pytest.raises(callers.CallerError, match="^invalid partial signature: invalid shareIdx$"):
            du.store_external({keys[0]: callers.ParSig(n + 1, bytes(32), bytes(c["sigs"][0]))})
        assert du.state() == before
        assert du._duty.set_stats() == dict(sets=t + 2, rejected=1, verified_not_stored=V - 1)
        assert du.store_external(peer_set(t - 1)) == {keys[v]: bytes(root_sigs[v]) for v in range(V)}
    # several peers' sets in one call: a rejected one, one with a failing pre-check behind a bad entry, good ones
    with callers.ParSigDuty(hipbls, t, {k: k for k in keys}, shares) as du:
        unknown = dict(list(spoiled(1, 0).items())[:3] + [(bytes(48), peer_set(1)[keys[0]])])
        bad_idx = dict(list(peer_set(1).items())[:2] + [(keys[5], callers.ParSig(n + 1, bytes(32), bytes(c["sigs"][0])))])
        res = du.store_external_many([peer_set(0), spoiled(1, 4), unknown, bad_idx, {}, peer_set(2), peer_set(3, range(8))])
        assert res[0] == {} and res[4] == {}
        for k, text in ((1, "invalid signature: signature not verified"), (2, "invalid signature: signature not verified"),
                        (3, "invalid shareIdx")):
            assert isinstance(res[k], callers.CallerError) and str(res[k]) == "invalid partial signature: " + text, (k, res[k])
            assert res[k].fired == {}
        # peers 0, 2 and 3 were stored: validators 0..7 fire through peer 3's set, the others hold two partials
        assert res[5] == {} and res[6] == {keys[v]: bytes(root_sigs[v]) for v in range(8)}
        st = du.state()
        assert [st[keys[v]] for v in range(V)] == [(3, True)] * 8 + [(2, False)] * 8
        assert du._duty.set_stats() == dict(sets=7, rejected=2, verified_not_stored=V - 1 + 2)
        # the default keeps admitting one by one, and the two calls mix on one duty
        with pytest.raises(callers.CallerError, match=not_verified) as ei:
            du.store_external(spoiled(1, 9))
        assert ei.value.fired == {keys[v]: bytes(root_sigs[v]) for v in range(8, V) if v != 9}
