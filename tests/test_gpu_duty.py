"""Duty sessions (hbls_duty_open / _add / _state / _stats / _close): a duty's partials verified as
each peer's set arrives, its validators aggregated when they reach the threshold, -m gpu.

Inputs are the tests/gpu_helpers/slot_select.py clusters of tests/test_gpu_slot_host.py: 256
validators (four waves), 5 of 7 and 3 of 4, four messages.  The reference is the defining property
of include/hipbls.h: for any way of cutting one candidate stream into adds, the union of what the
adds return equals what hbls_slot_select_batch returns for the concatenation (tests/gpu_helpers/
duty.py check_union), plus the construction (root_sigs), the matching rule restated in Python and,
for one validator, the bigint oracle.  Every comparison is exact.
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
def dh():
    import duty
    return duty


@pytest.fixture(scope="module")
def sh():
    import test_gpu_slot_host
    return test_gpu_slot_host


@pytest.fixture(scope="module")
def clusters(L, ss):
    return {(7, 5): ss.inputs(L, 7, 5), (4, 3): ss.inputs(L, 4, 3)}


@pytest.fixture(scope="module")
def streams(L, ss, dh, sh, clusters):
    """name -> (stream, its one-shot result): the clean clusters, and the 5-of-7 one with the skip_case
    and edge_case corruptions together (exactly t good, t - 1 good, none good, an undecodable key, no
    candidates, the same partial twice, share index 0)."""
    out = {}
    for key, d in clusters.items():
        out["clean", key] = dh.stream_of(sh.case(ss, d))
    d = clusters[(7, 5)]
    sigs, pks, cand, exp_v = sh.edge_case(L, ss, d)
    skip, _ = ss.skip_case(L, d)
    n, NP = d["n"], d["NP"]
    skip = skip.reshape(NP, 96)
    sigs[16 * n:] = skip[16 * n:]  # the edge validators are the first nine; the skip pattern from validator 16 on
    out["corrupt", (7, 5)] = dh.stream_of(sh.case(ss, d, sigs=sigs, cand=cand, pks=pks))
    return {k: (s, sh.host(L, dh.case_of(s))) for k, s in out.items()}


# 1: peer-major clean
def test_peer_major_clean(L, dh, clusters, streams):
    for key, d in clusters.items():
        s, one = streams["clean", key]
        V, n, t = d["V"], d["n"], d["t"]
        assert len(s["pks"]) == V * n and (s["group"][:V] == np.arange(V)).all()
        bounds = [k * V for k in range(n + 1)]
        r = dh.run(L, s, bounds)
        assert r["per_add"] == [0] * (t - 1) + [V] + [0] * (n - t), "all fire in add t, none before or after"
        assert np.array_equal(r["out"], d["root_sigs"].reshape(V, 96)) and not r["tst"].any() and not r["ast"].any()
        assert r["stored"][:t * V].all() and not r["stored"][t * V:].any()
        dh.check_union(r, one, s, bounds, key)


# 2: corruptions, random cuts, one partial per add
def test_corrupted_stream_random_cuts(L, dh, clusters, streams):
    s, one = streams["corrupt", (7, 5)]
    S = len(s["pks"])
    fired_adds = set()
    for n_adds in (1, 2, 5, 37):
        bounds = dh.random_cuts(S, n_adds, seed=1000 + n_adds)
        assert n_adds == 1 or any((bounds[k + 1] - bounds[k]) % 64 for k in range(n_adds))
        r = dh.run(L, s, bounds)
        dh.check_union(r, one, s, bounds, n_adds)
        fired_adds |= {(n_adds, int(k)) for k in r["fired_in"] if k >= 0}
    assert len({k for a, k in fired_adds if a == 37}) > 1, "groups fire in different adds"
    assert (one["tst"] == UNCHECKED).sum() >= 3 and (one["tst"] == OK).sum() > 200


def test_one_partial_per_add(L, dh, sh, streams):
    s, _ = streams["corrupt", (7, 5)]
    s16 = dh.sub_stream(s, np.flatnonzero(s["group"] < 16))
    s16["dv"] = s["dv"][:16]
    one = sh.host(L, dh.case_of(s16))
    bounds = list(range(len(s16["pks"]) + 1))
    r = dh.run(L, s16, bounds)
    dh.check_union(r, one, s16, bounds)
    assert max(r["per_add"]) == 1 and sum(r["per_add"]) == (one["tst"] != UNCHECKED).sum() >= 10


# 3: several roots per validator
def test_several_roots(L, ss, dh, sh, clusters):
    from oracle import bls12381 as Bo
    d = clusters[(7, 5)]
    c, exp, _ = _two_roots(L, ss, sh, clusters)
    s = dh.stream_of(c)
    one = sh.host(L, dh.case_of(s))
    V, t = d["V"], d["t"]
    root_of = [bytes(m) for m in s["msgs"]]
    for g in range(V):  # the restated rule on the stream itself
        mine = np.flatnonzero(s["group"] == g)
        mem, root = sh.matching(one["vst"], root_of, [(int(i), int(s["idx"][i])) for i in mine], t)
        assert (root is None) == (one["tst"][g] == UNCHECKED) == (g % 6 in (3, 5))
        if root is not None:
            assert list(one["chosen"][g]) == mem
    assert np.array_equal(one["out"], exp["out"]) and np.array_equal(one["tst"], exp["tst"])
    bounds = dh.random_cuts(len(s["pks"]), 9, seed=3)
    r = dh.run(L, s, bounds)
    dh.check_union(r, one, s, bounds)
    # validator 2: the later-started root B reaches t first; validator 4: share 1 over A dropped
    assert all(root_of[int(i)] == ss.OTHER_ROOT for i in r["chosen"][2])
    dropped = [i for i in np.flatnonzero(s["group"] == 4) if s["idx"][i] == 1]
    assert len(dropped) == 2 and r["stored"][dropped[0]] == 1 and r["stored"][dropped[1]] == 0 and r["vst"][dropped[1]] == OK
    assert r["count"][3] == 7 and r["count"][5] == 7 and not r["flag"][3]  # a second root holding fewer than t
    members = {int(s["idx"][int(i)]): bytes(s["sigs"][int(i)]) for i in r["chosen"][2]}
    st, agg = Bo.threshold_aggregate(members)
    assert st == OK and agg == bytes(r["out"][2])
    assert Bo.verify(bytes(s["dv"][2]), ss.OTHER_ROOT, agg) == OK


def _two_roots(L, ss, sh, clusters):
    """tests/test_gpu_slot_host.py's two_roots fixture, called as a plain function."""
    fn = sh.two_roots
    if hasattr(fn, "_get_wrapped_function"):
        fn = fn._get_wrapped_function()
    elif hasattr(fn, "__pytest_wrapped__"):
        fn = fn.__pytest_wrapped__.obj
    return fn(L, ss, clusters)


# 4: all t members of a group in one add
def test_group_fires_in_its_first_add(L, dh, sh, ss, clusters):
    d = clusters[(4, 3)]
    V, n, t = d["V"], d["n"], d["t"]
    c = sh.case(ss, d)  # validator-major: a validator's n partials side by side
    s = dh.stream_of(c)
    order = np.argsort(s["group"], kind="stable")  # back to validator-major arrival
    s = dh.sub_stream(s, order)
    s["sigs"][5 * n + 3] = s["sigs"][5 * n + 2]  # validator 5's last partial, behind its firing: not a signature of its key
    one = sh.host(L, dh.case_of(s))
    bounds = [0, 10 * n + 1, 64 * n, V * n]  # the first cut splits validator 10 after its first partial
    r = dh.run(L, s, bounds)
    dh.check_union(r, one, s, bounds)
    assert (r["fired_in"][:10] == 0).all() and r["fired_in"][10] == 1
    assert [int(x) for x in r["stored"][:n]] == [1] * t + [0] * (n - t)
    assert r["vst"][5 * n + 3] == NOT_VERIFIED and not r["vst"][:5 * n + 3].any() and r["stored"][5 * n + 3] == 0


# 5: max_stored below a group's distinct verified share indices
def test_max_stored(L, dh, sh, ss, clusters):
    d = clusters[(7, 5)]
    V, n, t = d["V"], d["n"], d["t"]
    c, _, _ = _two_roots(L, ss, sh, clusters)
    s = dh.stream_of(c)
    bounds = dh.random_cuts(len(s["pks"]), 4, seed=5)
    r = dh.run(L, s, bounds, max_stored=6)
    big = dh.run(L, s, bounds, max_stored=16)
    assert np.array_equal(r["vst"], big["vst"]) and not r["vst"].any()
    # pattern 3 (shares 1..3 over B, 4..7 over A) and 5 (copies of 1..3 over B first, then 4..7 over A):
    # seven distinct share indices, no root reaches t: six are stored, the seventh finds the group full
    for g in (3, 5, 9, 11):
        assert r["count"][g] == 6 and big["count"][g] == 7 and not r["flag"][g] and not big["flag"][g]
    # pattern 1 (shares 1, 2 over B, then 3..7 over A): A's fifth is the seventh store, so the group never fires
    for g in (1, 7):
        assert r["count"][g] == 6 and not r["flag"][g] and r["tst"][g] == UNCHECKED and big["flag"][g] and big["count"][g] == 7
    assert r["stats"][5] == sum(1 for g in range(V) if g % 6 in (1, 3, 5)) and big["stats"][5] == 0
    assert r["stats"][1] == r["stored"].sum() == big["stats"][1] - r["stats"][5]
    # groups that fire within six stored partials are as with room to spare
    same = np.asarray([g % 6 in (0, 2, 4) for g in range(V)])
    for k in ("out", "tst", "ast", "chosen", "fired_in"):
        assert np.array_equal(r[k][same], big[k][same]), k
    assert (r["count"] <= 6).all()


# 6: verify-only partials
def test_verify_only(L, dh, sh, ss, clusters, streams):
    s0, one = streams["corrupt", (7, 5)]
    G = len(s0["dv"])
    s = dict(s0, group=s0["group"].copy())
    every3 = np.arange(len(s["pks"])) % 3 == 0
    s["group"][every3] = np.where(np.arange(every3.sum()) % 2 == 0, NONE, G)  # 0xffffffff and n_groups
    bounds = dh.random_cuts(len(s["pks"]), 3, seed=6)
    r = dh.run(L, s, bounds)
    assert np.array_equal(r["vst"], one["vst"])
    dh.check_union(r, sh.host(L, dh.case_of(s)), s, bounds)
    assert not r["stored"][every3].any() and r["stored"].sum() == r["count"].sum() + 0 == r["stats"][1]
    # only verify-only partials: nothing is stored, nothing fires
    s["group"][:] = NONE
    r = dh.run(L, s, [0, 100, len(s["pks"])])
    assert np.array_equal(r["vst"], one["vst"]) and not r["stored"].any() and not r["count"].any() and r["per_add"] == [0, 0]


# 7: stats
def test_stats(L, dh, clusters, streams):
    d = clusters[(7, 5)]
    s, _ = streams["clean", (7, 5)]
    V, n, t = d["V"], d["n"], d["t"]
    nd = L.hbls_device_count()  # each shard hashes the messages its own partials carry
    a = dh.Duty(L, s["dv"], t, 16)
    try:
        for k in range(n):
            a.add(s, k * V, (k + 1) * V)
        st = a.stats()
        assert st[:2] == [n * V, t * V] and st[4:] == [V, 0]
        assert 4 <= st[2] <= 4 * nd and (nd > 1 or st[2] == 4) and st[2] + st[3] == st[0]
        b = dh.Duty(L, s["dv"], t, 16)
        try:
            b.add(s, 0, V)
            assert b.stats() == [V, V, st[2], V - st[2], 0, 0]
        finally:
            b.close()
        assert a.stats() == st
        assert a.add(s, 0, 0)["first"] == n * V and a.stats() == st  # an empty add
    finally:
        a.close()


# 8: two contexts per device
def test_device_split(L, dh, clusters, streams):
    runs = [("clean", [k * 256 for k in range(8)]), ("corrupt", None)]
    devices = L.hbls_device_count()
    want = {}
    for name, bounds in runs:
        s, one = streams[name, (7, 5)]
        bounds = bounds or dh.random_cuts(len(s["pks"]), 5, seed=8)
        want[name] = (bounds, dh.run(L, s, bounds))
    try:
        assert L.hbls_debug_split(2) == 0 and L.hbls_device_count() == 2 * devices
        for name, _ in runs:
            s, one = streams[name, (7, 5)]
            bounds, w = want[name]
            r = dh.run(L, s, bounds)
            dh.check_union(r, one, s, bounds, name)
            for k in ("vst", "stored", "chosen", "out", "tst", "ast", "fired_in", "count", "flag"):
                assert np.array_equal(r[k], w[k]), (name, k)
            assert r["per_add"] == w["per_add"] and r["stats"][:2] == w["stats"][:2] and r["stats"][4:] == w["stats"][4:]
    finally:
        assert L.hbls_debug_split(1) == 0


# 9: two duties from two threads beside a verify loop
def test_two_duties_two_threads(L, dh, sh, clusters, streams):
    jobs = [streams["corrupt", (7, 5)], streams["clean", (4, 3)]]
    res, errs, stop = [None, None], [], threading.Event()

    def drive(k):
        try:
            s, _ = jobs[k]
            bounds = dh.random_cuts(len(s["pks"]), 6, seed=90 + k)
            res[k] = (bounds, dh.run(L, s, bounds))
        except BaseException as e:  # noqa: BLE001
            errs.append(e)

    def verify_loop():
        s, one = jobs[1]
        n = 300
        pks, sigs, msgs = (np.ascontiguousarray(s[k][:n]).reshape(-1) for k in ("pks", "sigs", "msgs"))
        off, ln = np.arange(n, dtype=np.uint64) * 32, np.full(n, 32, np.uint32)
        try:
            while not stop.is_set():
                st = np.full(n, 0xA5, np.uint8)
                p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
                assert L.hbls_verify_batch(p(pks), p(sigs), p(msgs), p(off), p(ln), n, p(st)) == 0
                assert np.array_equal(st, one["vst"][:n])
        except BaseException as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=drive, args=(k,)) for k in (0, 1)]
    vt = threading.Thread(target=verify_loop)
    vt.start()
    for x in th:
        x.start()
    for x in th:
        x.join()
    stop.set()
    vt.join()
    assert not errs, errs
    for k in (0, 1):
        s, one = jobs[k]
        dh.check_union(res[k][1], one, s, res[k][0], k)


# 10: call errors
def test_call_errors(L, dh, clusters, streams):
    s, one = streams["clean", (4, 3)]
    V, t = 256, s["t"]
    dv = np.ascontiguousarray(s["dv"]).reshape(-1)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    h = ctypes.c_uint64(0)

    def err(rc):
        return rc, L.hbls_last_error().decode()

    for bad_t in (0, 17):
        assert err(L.hbls_duty_open(p(dv), V, bad_t, 8, ctypes.byref(h))) == (-1, "hbls_duty_open: threshold must be in 1..16")
    for bad_m in (0, 65):
        assert err(L.hbls_duty_open(p(dv), V, t, bad_m, ctypes.byref(h))) == (-1, "hbls_duty_open: max_stored must be in 1..64")
    assert err(L.hbls_duty_open(None, V, t, 8, ctypes.byref(h))) == (-1, "hbls_duty_open: dv_pks is required")
    assert err(L.hbls_duty_open(p(dv), V, t, 8, None)) == (-1, "hbls_duty_open: duty is required")
    assert h.value == 0
    du = dh.Duty(L, s["dv"], t, 8)
    du.add(s, 0, V)
    # a null required pointer with a non-zero count
    n = 4
    a = [np.ascontiguousarray(s[k][V:V + n]).reshape(-1) for k in ("pks", "sigs", "msgs")]
    a += [np.arange(n, dtype=np.uint64) * 32, np.full(n, 32, np.uint32), np.ascontiguousarray(s["group"][V:V + n]),
          np.ascontiguousarray(s["idx"][V:V + n])]
    outs = [np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(1, np.uint32), np.zeros(n, np.uint32), np.zeros(1, np.uint64),
            np.zeros(n * t, np.uint32), np.zeros(96 * n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)]

    def add(handle, drop=None):
        args = [None if k == drop else p(x) for k, x in enumerate(a)] + [n] + \
               [None if 8 + k == drop else p(x) for k, x in enumerate(outs)]
        return err(L.hbls_duty_add(handle, *args))

    want = (-1, "hbls_duty_add: pks, sigs, msg_off, msg_len, group, share_idx, vstatus and stored are required")
    for drop in (0, 1, 3, 4, 5, 6, 8, 9):
        assert add(du.h, drop) == want, drop
    assert add(du.h, 2) == (-1, "hbls_duty_add: msgs is required")
    for drop in (10, 12):
        assert add(du.h, drop) == (-1, "hbls_duty_add: first_serial and n_fired are required"), drop
    for drop in (11, 13, 14, 15, 16):
        assert add(du.h, drop) == (-1, "hbls_duty_add: fired, chosen, ta_out, ta_status and agg_vstatus are required"), drop
    # a handle never issued
    none = "no such duty (never opened, or closed)"
    for bad in (0, du.h + 1000):
        assert add(bad) == (-1, "hbls_duty_add: " + none)
        assert err(L.hbls_duty_state(bad, p(outs[3]), p(outs[0]))) == (-1, "hbls_duty_state: " + none)
        assert err(L.hbls_duty_stats(bad, p(outs[4]), 1)) == (-1, "hbls_duty_stats: " + none)
        assert err(L.hbls_duty_close(bad)) == (-1, "hbls_duty_close: " + none)
    assert err(L.hbls_duty_stats(du.h, p(outs[4]), 7)) == (-1, "hbls_duty_stats: out is null or n above 6")
    # the valid duty is unaffected: the rest of the stream gives the one-shot result
    assert du.stats()[:2] == [V, V]
    fired = []
    for k in range(1, 4):
        r = du.add(s, k * V, (k + 1) * V)
        assert r["first"] == k * V
        fired.append(len(r["fired"]))
        if k == t - 1:
            assert np.array_equal(r["out"], one["out"]) and not r["tst"].any() and not r["ast"].any()
    assert fired == [0, V, 0]
    # a closed handle
    closed = du.h
    du.close()
    assert add(closed) == (-1, "hbls_duty_add: " + none)
    assert err(L.hbls_duty_state(closed, p(outs[3]), p(outs[0]))) == (-1, "hbls_duty_state: " + none)
    assert err(L.hbls_duty_stats(closed, p(outs[4]), 1)) == (-1, "hbls_duty_stats: " + none)
    assert err(L.hbls_duty_close(closed)) == (-1, "hbls_duty_close: " + none)


# the Python layers: tbls.Duty and the ParSigEx -> MemDB -> Aggregator mirror
def test_parsig_duty_mirror(hipbls, ss, sh, clusters):
    from charon_amd import callers
    d = clusters[(4, 3)]
    V, n, t = 16, d["n"], d["t"]
    c = sh.case(ss, d)
    keys = [bytes(c["dv"][v]) for v in range(V)]
    shares = {keys[v]: {s + 1: bytes(c["pks"][v * n + s]) for s in range(n)} for v in range(V)}
    root_sigs = d["root_sigs"].reshape(-1, 96)

    def peer_set(s, vs=range(V)):
        return {keys[v]: callers.ParSig(s + 1, bytes(c["msgs"][v * n + s]), bytes(c["sigs"][v * n + s])) for v in vs}

    with callers.ParSigDuty(hipbls, t, {k: k for k in keys}, shares) as du:
        for s in range(t - 1):
            assert du.store_external(peer_set(s)) == {}
        assert du.state()[keys[3]] == (t - 1, False)
        # a set with an entry that does not verify, one with an unknown validator, one with a bad share index
        bad = peer_set(t - 1, range(4))
        bad[keys[2]] = callers.ParSig(t, bad[keys[2]].signing_root, bad[keys[1]].signature)
        with pytest.raises(callers.CallerError, match="^invalid partial signature: invalid signature: signature not verified$") as ei:
            du.store_external(bad)
        assert ei.value.fired == {keys[v]: bytes(root_sigs[v]) for v in (0, 1, 3)}
        with pytest.raises(callers.CallerError, match="^invalid partial signature: unknown pubkey, not part of cluster lock$"):
            du.store_external({bytes(48): peer_set(0)[keys[0]]})
        with pytest.raises(callers.CallerError, match="^invalid partial signature: invalid shareIdx$"):
            du.store_external({keys[0]: callers.ParSig(n + 1, bytes(32), bytes(c["sigs"][0]))})
        # validators 0, 1 and 3 fired in the failing set (their entries verified); the rest fire now
        st = du.state()
        assert [st[keys[v]][1] for v in range(5)] == [True, True, False, True, False]
        got = du.store_external(peer_set(t - 1))
        assert got == {keys[v]: bytes(root_sigs[v]) for v in range(V) if v not in (0, 1, 3)}
        assert du.store_external(peer_set(t)) == {} and all(f for _, f in du.state().values())
    with hipbls.duty_open(keys, t, max_stored=4) as du2:
        r = du2.add([shares[keys[0]][1]], [bytes(c["msgs"][0])], [bytes(c["sigs"][0])], [0], [1])
        assert (r.vstatus, r.stored, r.first_serial, r.fired) == ([OK], [1], 0, [])
        assert du2.stats() == dict(seen=1, stored=1, hashed=1, resident_lookups=0, fired=0, full=0)
    with pytest.raises(Exception, match="closed"):
        du2.state()
