"""The cases of tests/test_gpu_cluster.py: cluster handles through the ABI (hbls_cluster_open / _close /
_stats, hbls_duty_open_cluster, and the three add entry points on a cluster duty), -m gpu.  Not collected
with the suite (the name): that file runs this one once, in a process of its own, and says why.

Inputs are the clusters and clean streams of tests/test_gpu_duty.py (256 validators, 5 of 7 and 3 of 4,
peer-major: partial i of a stream is peer i // 256's partial of validator i % 256 under share index
i // 256 + 1).  The lock is rebuilt from each cluster's pubshares and DV keys.  The reference is the
defining property of include/hipbls.h, the twin (tests/gpu_helpers/cluster.py run_twin), plus the
construction (root_sigs).  Every comparison is exact.
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

from charon_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HELPERS = os.path.join(ROOT, "tests", "gpu_helpers")
for p in (ROOT, HELPERS, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

OK, BAD_PUBKEY, UNCHECKED = 0, 1, 7
NONE = 0xFFFFFFFF
MODES = ("add", "sets", "first")

from test_gpu_duty import L, clusters, dh, sh, ss, streams  # noqa: E402,F401 -- its fixtures: the same clusters and streams


@pytest.fixture(scope="module")
def ch():
    import cluster
    return cluster


@pytest.fixture(scope="module")
def locks(ch, clusters):
    return {key: ch.Lock(d["dv_pks"], d["pks"], d["n"]) for key, d in clusters.items()}


def layouts(V, n):
    """peer-major with one set per call; all sets in one call"""
    return (([k * V for k in range(n + 1)], [[0, V]] * n), ([0, n * V], [[k * V for k in range(n + 1)]]))


# 1
@pytest.mark.parametrize("mode", MODES)
def test_clean_streams_equal_the_twin_and_the_construction(L, ch, clusters, streams, locks, mode):
    for key, d in clusters.items():
        s, _ = streams["clean", key]
        V, n, t = d["V"], d["n"], d["t"]
        tw, nokey = ch.twin_stream(s, locks[key])
        assert np.array_equal(tw["pks"], s["pks"]) and not nokey.any(), "the twin's pks are the stream's own"
        assert np.array_equal(tw["dv"], s["dv"])
        for tables in (1, 0):
            cl = ch.Cluster(L, locks[key], tables)
            try:
                assert not cl.key_status.any()
                assert cl.stats() == [V * (1 + n), 0, V * (1 + n) * tables, 0, 0, 0]
                for bounds, sets in layouts(V, n) if tables else layouts(V, n)[:1]:
                    r = ch.run_twin(L, cl, s, bounds, sets, mode, t)
                    assert r["rejected_by_twin"] == 0
                    out = np.concatenate([c["out"] for c in r["calls"]])
                    fired = np.concatenate([c["fired"] for c in r["calls"]])
                    assert fired.tolist() == list(range(V)) and np.array_equal(out, d["root_sigs"].reshape(V, 96))
                    assert all(not c["tst"].any() and not c["ast"].any() and not c["vst"].any() for c in r["calls"])
                    assert r["flag"].all() and (r["count"] == t).all() and r["stats"][:2] == [n * V, t * V]
                runs = 2 if tables else 1
                assert cl.stats()[3:] == [runs * n * V, 0, runs * V], "partials resolved, none without a key, a DV key per aggregate"
            finally:
                cl.close()


def planted(ch, d, s, lock):
    """The 5-of-7 stream with share index 0, n + 1 and 2^32 + 1 and a group equal to n_validators planted in
    peers 1 and 4, over a lock whose pubshare (validator 50, share 2) and DV key of validator 60 are
    undecodable.  -> (stream, lock, the planted partials' positions)"""
    V, n = d["V"], d["n"]
    idx, group = s["idx"].copy(), s["group"].copy()
    at = dict(zero=1 * V + 10, over=1 * V + 20, wide=4 * V + 30, group=4 * V + 40, badshare=1 * V + 50)
    idx[at["zero"]], idx[at["over"]], idx[at["wide"]] = 0, n + 1, (1 << 32) + 1
    group[at["group"]] = V
    bad = ch.Lock(lock.dv, lock.shares, n)
    bad.shares[50, 1] = 0xFF
    bad.dv[60] = 0xFF
    return dict(s, idx=idx, group=group), bad, at


# 2
@pytest.mark.parametrize("mode", MODES)
def test_planted_errors(L, ch, clusters, streams, locks, mode):
    d = clusters[(7, 5)]
    s0, _ = streams["clean", (7, 5)]
    V, n, t = d["V"], d["n"], d["t"]
    s, lock, at = planted(ch, d, s0, locks[(7, 5)])
    tw, nokey = ch.twin_stream(s, lock)
    assert sorted(np.flatnonzero(nokey).tolist()) == sorted(at[k] for k in ("zero", "over", "wide", "group"))
    assert not tw["pks"][nokey].any() and (tw["pks"][at["badshare"]] == 0xFF).all()
    cl = ch.Cluster(L, lock)
    try:
        want = np.zeros((V, 1 + n), np.uint8)
        want[50, 2] = want[60, 0] = BAD_PUBKEY
        assert np.array_equal(cl.key_status, want), "key_status names exactly the two bad keys"
        keys = V * (1 + n)
        assert cl.stats() == [keys, 2, keys - 2, 0, 0, 0]
        bad = sorted(at.values())
        for bounds, sets in layouts(V, n):
            r = ch.run_twin(L, cl, s, bounds, sets, mode, t)
            # the twin rejects exactly the planted items and nothing else: a wrong fixture cannot hide a wrong kernel
            exact = np.concatenate([w["vst"] for w in r["twin"]])
            assert r["rejected_by_twin"] == 5 and np.flatnonzero(exact != OK).tolist() == bad
            assert (exact[bad] == BAD_PUBKEY).all(), "no key, or the lock's bad pubshare: HBLS_BAD_PUBKEY, as 48 zero bytes get"
            vst = np.concatenate([c["vst"] for c in r["calls"]])
            stored = np.concatenate([c["stored"] for c in r["calls"]])
            assert vst[at["badshare"]] == BAD_PUBKEY and not stored[bad].any()
            fired = np.concatenate([c["fired"] for c in r["calls"]])
            ast = np.concatenate([c["ast"] for c in r["calls"]])
            tst = np.concatenate([c["tst"] for c in r["calls"]])
            assert sorted(fired.tolist()) == list(range(V)) and not tst.any(), "every validator still fires"
            assert ast[fired == 60].tolist() == [BAD_PUBKEY] and not ast[fired != 60].any(), "the bad DV key: agg_vstatus 1"
            if mode == "add":
                assert (vst[bad] == BAD_PUBKEY).all() and np.flatnonzero(vst != OK).tolist() == bad
            else:  # peers 1 and 4 are rejected whole, with set_first at their first planted partial
                sf = [NONE if x == NONE else int(x) + lo for c, lo in zip(r["calls"], bounds) for x in c["set_first"]]
                assert sf == [NONE if k not in (1, 4) else (at["zero"] if k == 1 else at["wide"]) for k in range(n)]
                assert not stored[1 * V:2 * V].any() and not stored[4 * V:5 * V].any() and r["set_stats"][:2] == [n, 2]
                assert vst[at["zero"]] == BAD_PUBKEY and vst[at["wide"]] == BAD_PUBKEY
        resolved = 2 * (n * V - 4)
        assert cl.stats() == [keys, 2, keys - 2, resolved, 2 * 4, 2 * V]
    finally:
        cl.close()


def _raw_open(L, lock_args, n_shares, tables=1):
    dv, sh, V = lock_args
    st = np.full(64, 0xA5, np.uint8)
    h = ctypes.c_uint64(0)
    rc = L.hbls_cluster_open(ctypes.c_void_p(dv.ctypes.data), ctypes.c_void_p(sh.ctypes.data), V, n_shares, tables,
                             ctypes.c_void_p(st.ctypes.data), ctypes.byref(h))
    assert (st == 0xA5).all() and h.value == 0, "a failed open wrote"
    return rc, L.hbls_last_error().decode()


# 3
def test_call_errors_write_nothing(L, ch, clusters, streams, locks):
    d = clusters[(4, 3)]
    s, _ = streams["clean", (4, 3)]
    V, n, t = d["V"], d["n"], d["t"]
    lock = locks[(4, 3)]

    def err(rc):
        return rc, L.hbls_last_error().decode()

    cl = ch.Cluster(L, lock)
    a, b = ch.ClusterDuty(L, cl, t, 8), ch.FirstDuty(L, lock.dv, t, 8)
    try:
        a.add_sets(s, 0, V, [0, 10, V])
        b.add_sets(s, 0, V, [0, 10, V])
        before = [(x.state()[0].tolist(), x.state()[1].tolist(), x.stats(), x.set_stats(), x.first_stats()) for x in (a, b)]
        cstats = cl.stats()
        # pks on a cluster duty: a shim that mixes the two kinds of duty
        msg = ": pks must be NULL on a cluster duty (the keys are the cluster's)"
        assert err(a.add_sets(s, V, V + 5, [0, 2, 5], raw=True, keys=True)) == (-1, "hbls_duty_add_sets" + msg)
        assert err(a.add_sets_first(s, V, V + 5, [0, 2, 5], raw=True, keys=True)) == (-1, "hbls_duty_add_sets_first" + msg)
        assert err(a.add(s, V, V + 5, raw=True, keys=True)) == (-1, "hbls_duty_add" + msg)
        # NULL pks on a plain duty: the call error it always was
        add, add_sets, add_first = ch.no_keys(b)
        req = ": pks, sigs, msg_off, msg_len, group, share_idx, vstatus and stored are required"
        assert err(add_sets(s, V, V + 5, [0, 2, 5], raw=True)) == (-1, "hbls_duty_add_sets" + req)
        assert err(add_first(s, V, V + 5, [0, 2, 5], raw=True)) == (-1, "hbls_duty_add_sets_first" + req)
        assert err(add(s, V, V + 5, raw=True)) == (-1, "hbls_duty_add" + req)
        # nothing was verified, stored, numbered or counted
        assert [(x.state()[0].tolist(), x.state()[1].tolist(), x.stats(), x.set_stats(), x.first_stats()) for x in (a, b)] == before
        assert cl.stats() == cstats
        # a closed or unknown cluster
        none = "no such cluster (never opened, or closed)"
        out = np.full(8, 0xA5A5A5A5A5A5A5A5, np.uint64)
        po = ctypes.c_void_p(out.ctypes.data)
        for bad in (0, cl.h + 1000):
            h = ctypes.c_uint64(77)
            assert err(L.hbls_duty_open_cluster(bad, t, 8, ctypes.byref(h))) == (-1, "hbls_duty_open_cluster: " + none)
            assert h.value == 77
            assert err(L.hbls_cluster_stats(bad, po, 6)) == (-1, "hbls_cluster_stats: " + none)
            assert err(L.hbls_cluster_close(bad)) == (-1, "hbls_cluster_close: " + none)
        assert err(L.hbls_cluster_stats(cl.h, po, 7)) == (-1, "hbls_cluster_stats: out is null or n above 6")
        assert err(L.hbls_cluster_stats(cl.h, None, 1)) == (-1, "hbls_cluster_stats: out is null or n above 6")
        assert (out == 0xA5A5A5A5A5A5A5A5).all()
        h = ctypes.c_uint64(77)
        assert err(L.hbls_duty_open_cluster(cl.h, 0, 8, ctypes.byref(h)))[0] == -1 and h.value == 77
        assert err(L.hbls_duty_open_cluster(cl.h, t, 65, ctypes.byref(h)))[0] == -1 and h.value == 77
        # n_shares 0 and 65
        args = (lock.dv.reshape(-1), lock.shares.reshape(-1), 3)
        for ns in (0, 65):
            assert _raw_open(L, args, ns) == (-1, "hbls_cluster_open: n_shares must be in 1..64")
        assert _raw_open(L, args, 1, tables=2) == (-1, "hbls_cluster_open: ladder_tables must be 0 or 1")
    finally:
        a.close()
        b.close()
        closed = cl.h
        cl.close()
    h = ctypes.c_uint64(77)
    assert err(L.hbls_duty_open_cluster(closed, t, 8, ctypes.byref(h))) == \
        (-1, "hbls_duty_open_cluster: no such cluster (never opened, or closed)") and h.value == 77
    assert err(L.hbls_cluster_close(closed)) == (-1, "hbls_cluster_close: no such cluster (never opened, or closed)")


# 4
def test_a_duty_outlives_its_closed_cluster(L, ch, clusters, streams, locks):
    d = clusters[(4, 3)]
    s, _ = streams["clean", (4, 3)]
    V, n, t = d["V"], d["n"], d["t"]
    cl = ch.Cluster(L, locks[(4, 3)])
    duties = (ch.ClusterDuty(L, cl, t, 16), ch.FirstDuty(L, cl.lock.dv, t, 16), None)
    cl.close()
    assert ch.ClusterDuty(L, cl, t, 16, raw=True).rc == -1, "no new duty on a closed cluster"
    bounds, sets = layouts(V, n)[0]
    r = ch.run_twin(L, cl, s, bounds, sets, "sets", t, duties=duties)
    assert np.concatenate([c["fired"] for c in r["calls"]]).tolist() == list(range(V))
    assert np.array_equal(np.concatenate([c["out"] for c in r["calls"]]), d["root_sigs"].reshape(V, 96))


# 5
def test_the_learned_key_cache_is_left_alone(L, ch, clusters, streams, locks):
    d = clusters[(4, 3)]
    s, _ = streams["clean", (4, 3)]
    V, n, t = d["V"], d["n"], d["t"]
    before = (_lib.key_learn_stats(L), _lib.key_wide_stats(L))
    cl = ch.Cluster(L, locks[(4, 3)])
    du = ch.ClusterDuty(L, cl, t, 16)
    try:
        fired = 0
        for k, call in enumerate((du.add, du.add_sets, du.add_sets_first, du.add)):
            r = call(s, k * V, (k + 1) * V) if call == du.add else call(s, k * V, (k + 1) * V, [0, V])
            assert not r["vst"].any()
            fired += len(r["fired"])
        assert fired == V
    finally:
        du.close()
        cl.close()
    assert (_lib.key_learn_stats(L), _lib.key_wide_stats(L)) == before, "neither read nor written: no hit, no miss, no entry"


# 6
@pytest.mark.parametrize("copies", [2])
def test_two_contexts(L, ch, clusters, streams, locks, copies):
    d = clusters[(7, 5)]
    s0, _ = streams["clean", (7, 5)]
    V, n, t = d["V"], d["n"], d["t"]
    s, lock, at = planted(ch, d, s0, locks[(7, 5)])
    bounds, sets = layouts(V, n)[0]
    devices = L.hbls_device_count()
    one = ch.Cluster(L, lock)
    try:
        want = {m: ch.run_twin(L, one, s, bounds, sets, m, t) for m in MODES}
    finally:
        one.close()
    try:
        assert L.hbls_debug_split(copies) == 0 and L.hbls_device_count() == copies * devices
        cl = ch.Cluster(L, lock)
        try:
            assert np.array_equal(cl.key_status, one.key_status) and cl.stats()[:3] == [V * (1 + n), 2, V * (1 + n) - 2]
            got = {m: ch.run_twin(L, cl, s, bounds, sets, m, t) for m in MODES}
        finally:
            cl.close()
    finally:
        assert L.hbls_debug_split(1) == 0
    for m in MODES:
        assert got[m]["rejected_by_twin"] == 5
        for x, y in zip(want[m]["calls"], got[m]["calls"]):
            for k in ("first", "stored", "fired", "chosen", "out", "tst", "ast") + (("vst",) if m != "first" else ()):
                assert np.array_equal(x[k], y[k]), (m, k)
        assert np.array_equal(want[m]["count"], got[m]["count"]) and np.array_equal(want[m]["flag"], got[m]["flag"])


# 7
def test_a_cluster_keeps_the_shard_layout_it_was_opened_under(L, ch, clusters, streams, locks):
    """the cluster and the twin are opened under two contexts; the cluster duty after the split is set back to one"""
    d = clusters[(7, 5)]
    s0, _ = streams["clean", (7, 5)]
    V, n, t = d["V"], d["n"], d["t"]
    s, lock, at = planted(ch, d, s0, locks[(7, 5)])
    bounds, sets = layouts(V, n)[0]
    try:
        assert L.hbls_debug_split(2) == 0
        cl = ch.Cluster(L, lock)
        twins = (ch.FirstDuty(L, lock.dv, t, 16), ch.FirstDuty(L, lock.dv, t, 16))
    finally:
        assert L.hbls_debug_split(1) == 0
    try:
        duties = (ch.ClusterDuty(L, cl, t, 16),) + twins
        r = ch.run_twin(L, cl, s, bounds, sets, "first", t, duties=duties)
        assert r["rejected_by_twin"] == 5 and r["set_stats"][:2] == [n, 2]
        assert sorted(np.concatenate([c["fired"] for c in r["calls"]]).tolist()) == list(range(V))
        # both shards served: the bad pubshare is validator 50's (the first shard), the bad DV key validator 60's,
        # and the planted group V goes to the shard its arrival index picks
        assert cl.stats()[3:] == [n * V - 4, 4, V]
    finally:
        cl.close()


# 8
def test_a_real_lock(L, ch):
    with open(os.path.join(ROOT, "tests", "golden", "kat_reference.json")) as f:
        lock = json.load(f)["locks"][0]
    vals = lock["validators"]
    n = len(vals[0]["shares"])
    dv = np.frombuffer(b"".join(bytes.fromhex(v["dpk"]) for v in vals), np.uint8)
    shares = np.frombuffer(b"".join(bytes.fromhex(x) for v in vals for x in v["shares"]), np.uint8)
    assert all(len(v["shares"]) == n for v in vals) and len(dv) == 48 * len(vals) and len(shares) == 48 * n * len(vals)
    for tables in (1, 0):
        cl = ch.Cluster(L, ch.Lock(dv, shares, n), tables)
        try:
            assert cl.key_status.shape == (len(vals), 1 + n) and not cl.key_status.any()
            assert cl.stats() == [len(vals) * (1 + n), 0, len(vals) * (1 + n) * tables, 0, 0, 0]
            du = ch.ClusterDuty(L, cl, lock["threshold"], 16)
            assert du.state()[0].tolist() == [0] * len(vals)
            du.close()
        finally:
            cl.close()


# 9: the Python layer
def test_parsig_duty_on_a_cluster(hipbls, ss, sh, clusters):
    from charon_amd import callers
    d = clusters[(4, 3)]
    V, n, t = 16, d["n"], d["t"]
    c = sh.case(ss, d)
    keys = [bytes(c["dv"][v]) for v in range(V)]
    shares = {keys[v]: {s + 1: bytes(c["pks"][v * n + s]) for s in range(n)} for v in range(V)}
    root_sigs = d["root_sigs"].reshape(-1, 96)

    def peer_set(s, vs=range(V)):
        return {keys[v]: callers.ParSig(s + 1, bytes(c["msgs"][v * n + s]), bytes(c["sigs"][v * n + s])) for v in vs}

    with callers.Cluster(hipbls, {k: k for k in keys}, shares) as cl:
        assert cl.key_status == [[0] * (1 + n)] * V and cl.stats()["keys"] == V * (1 + n) == cl.stats()["ladder_tables"]
        for kw in (dict(), dict(reject_sets=True), dict(reject_sets=True, first_error=True)):
            with callers.ParSigDuty(hipbls, t, cluster=cl, **kw) as du:
                for s in range(t - 1):
                    assert du.store_external(peer_set(s)) == {}
                with pytest.raises(callers.CallerError, match="^invalid partial signature: invalid shareIdx$"):
                    du.store_external({keys[0]: callers.ParSig(n + 1, bytes(32), bytes(c["sigs"][0]))})
                with pytest.raises(callers.CallerError, match="^invalid partial signature: unknown pubkey, not part of cluster lock$"):
                    du.store_external({bytes(48): peer_set(0)[keys[0]]})
                assert du.store_external(peer_set(t - 1)) == {keys[v]: bytes(root_sigs[v]) for v in range(V)}
        st = cl.stats()
        assert st["partials_resolved"] == 3 * t * V and st["partials_no_key"] == 0 and st["dv_keys_resolved"] == 3 * V
        with hipbls.duty_open((), t, cluster=cl) as raw:  # the binding refuses keys on a cluster duty before the library does
            with pytest.raises(callers.TblsError):
                raw.add([bytes(48)], [bytes(32)], [bytes(96)], [0], [1])
