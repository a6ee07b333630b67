"""Cluster handles (hbls_cluster_open / _close / _stats, hbls_duty_open_cluster) beside plain duties on
the same stream, for tests/gpu_helpers/cluster_cases.py.  Streams, sentinels and the calls' plumbing are
tests/gpu_helpers/duty.py's, duty_sets.py's and duty_first.py's: a cluster duty's adds have the plain
calls' signatures, so the plain helpers drive them through a library handle that answers the add entry
points with the wanted one and passes NULL for pks.

The reference is the defining property of include/hipbls.h (the twin): a cluster duty equals a plain duty
opened with the same dv_pks, threshold and max_stored under the same shard layout, fed the same calls
with pks[i] = the lock's 48 bytes for (group[i], share_idx[i]) where that names a key and 48 zero bytes
elsewhere.
"""
import ctypes

import numpy as np

from duty import NONE, _p
from duty_first import FirstDuty, check_contract
from duty_sets import same_call

OK, BAD_PUBKEY, UNCHECKED = 0, 1, 7
NO_KEY = 0xFFFFFFFF
S8, S64 = 0xA5, 0xA5A5A5A5A5A5A5A5


def cluster_key(group, share_idx, group_base, n_groups, n_shares, dv=False):
    """include/hipbls.h restated (tests/test_cluster_host.py holds cluster.h to the same words)"""
    if not group_base <= group < group_base + n_groups:
        return NO_KEY
    if not (0 if dv else 1) <= share_idx <= n_shares:
        return NO_KEY
    return (group - group_base) * (1 + n_shares) + share_idx


class Lock:
    """dv: V x 48, shares: V x n x 48 (share j of validator g at [g, j - 1])"""

    def __init__(self, dv, shares, n):
        self.dv = np.ascontiguousarray(dv, np.uint8).reshape(-1, 48).copy()
        self.V, self.n = len(self.dv), n
        self.shares = np.ascontiguousarray(shares, np.uint8).reshape(self.V, n, 48).copy()

    def key(self, g, j):
        return self.dv[g] if j == 0 else self.shares[g, j - 1]


def twin_stream(s, lock):
    """The stream the twin gets: the lock's 48 bytes where (group, share index) names a key, 48 zero bytes
    elsewhere; the lock's DV keys.  -> (stream, the partials that name no key)"""
    pks = np.zeros((len(s["group"]), 48), np.uint8)
    nokey = np.zeros(len(s["group"]), bool)
    for i, (g, j) in enumerate(zip(s["group"].tolist(), s["idx"].tolist())):
        if cluster_key(g, j, 0, lock.V, lock.n) == NO_KEY:
            nokey[i] = True
        else:
            pks[i] = lock.key(g, j)
    return dict(s, pks=pks, dv=lock.dv), nokey


class Cluster:
    def __init__(self, L, lock, tables=1, raw=False):
        self.L, self.lock = L, lock
        row = 1 + lock.n
        st = np.full(lock.V * row + 8, S8, np.uint8)
        h = ctypes.c_uint64(0)
        self.rc = L.hbls_cluster_open(_p(lock.dv.reshape(-1)), _p(lock.shares.reshape(-1)), lock.V, lock.n, tables, _p(st),
                                      ctypes.byref(h))
        self.h = h.value
        if raw:
            assert (st == S8).all() and h.value == 0, "a failed open wrote"
            return
        assert self.rc == 0, L.hbls_last_error().decode()
        assert h.value != 0 and (st[lock.V * row:] == S8).all(), "sentinel behind key_status"
        self.key_status = st[:lock.V * row].reshape(lock.V, row)

    def stats(self):
        out = np.full(6 + 2, S64, np.uint64)
        assert self.L.hbls_cluster_stats(self.h, _p(out), 6) == 0, self.L.hbls_last_error().decode()
        assert (out[6:] == S64).all()
        return [int(x) for x in out[:6]]

    def close(self):
        assert self.L.hbls_cluster_close(self.h) == 0, self.L.hbls_last_error().decode()


class _Entry:
    """The library with hbls_duty_add / hbls_duty_add_sets answered by `entry` (None: themselves) and,
    unless keys, pks replaced by NULL"""

    def __init__(self, L, entry, keys):
        self._L, self._entry, self._keys = L, entry, keys

    def __getattr__(self, name):
        if name not in ("hbls_duty_add", "hbls_duty_add_sets"):
            return getattr(self._L, name)
        fn = getattr(self._L, self._entry or name)
        return fn if self._keys else (lambda h, pks, *a: fn(h, None, *a))


class ClusterDuty(FirstDuty):
    """A duty on a cluster (keys=False), or a plain duty called as tests call a cluster duty"""

    def __init__(self, L, cluster, t, max_stored, raw=False):
        self.L, self.G, self.t = L, cluster.lock.V, t
        h = ctypes.c_uint64(0)
        self.rc = L.hbls_duty_open_cluster(cluster.h, t, max_stored, ctypes.byref(h))
        self.h = h.value
        if not raw:
            assert self.rc == 0, L.hbls_last_error().decode()
            assert h.value != 0

    def _via(self, entry, keys, fn, *a, **kw):
        real, self.L = self.L, _Entry(self.L, entry, keys)
        try:
            return fn(*a, **kw)
        finally:
            self.L = real

    def add(self, *a, keys=False, **kw):
        return self._via(None, keys, super().add, *a, **kw)

    def add_sets(self, *a, keys=False, **kw):
        return self._via(None, keys, super().add_sets, *a, **kw)

    def add_sets_first(self, *a, keys=False, **kw):
        return self._via("hbls_duty_add_sets_first", keys, super().add_sets, *a, **kw)


def no_keys(duty):
    """a plain duty (SetsDuty / FirstDuty) whose next calls pass NULL for pks: -> (add, add_sets) callables"""
    def call(fn, entry=None):
        def go(*a, **kw):
            real, duty.L = duty.L, _Entry(duty.L, entry, False)
            try:
                return fn(*a, **kw)
            finally:
                duty.L = real
        return go
    return call(duty.add), call(duty.add_sets), call(duty.add_sets, "hbls_duty_add_sets_first")


def run_twin(L, cl, s, bounds, sets_of_call, mode, t, max_stored=16, duties=None):
    """The stream through a duty on cluster `cl` and through its twin, call k = partials [bounds[k],
    bounds[k + 1]) in the sets sets_of_call[k] (offsets relative to the call), every call through the
    entry point `mode`: "add", "sets" or "first".  Every output of every call, hbls_duty_state and the
    three statistics are compared exactly; for "first" the twin goes through hbls_duty_add_sets_first as
    well (everything but vstatus exact), and a second twin through hbls_duty_add_sets gives the exact
    statuses the call's vstatus is held to under the contract of include/hipbls.h (duty_first.py
    check_contract).  duties: (cluster duty, twin, exact twin or None) opened by the caller (a shard
    layout of its own); they are closed here.
    -> dict(calls, twin, nokey, count, flag, stats, set_stats, first_stats, rejected_by_twin)"""
    tw, nokey = twin_stream(s, cl.lock)
    if duties is None:
        duties = (ClusterDuty(L, cl, t, max_stored), FirstDuty(L, cl.lock.dv, t, max_stored),
                  FirstDuty(L, cl.lock.dv, t, max_stored) if mode == "first" else None)
    a, b, c = duties
    res = dict(calls=[], twin=[], nokey=nokey, rejected_by_twin=0)
    unchecked = 0
    try:
        for k in range(len(bounds) - 1):
            lo, hi, off = bounds[k], bounds[k + 1], list(sets_of_call[k])
            if mode == "add":
                r, w = a.add(s, lo, hi), b.add(tw, lo, hi)
                same_call(r, w, k)
            elif mode == "sets":
                r, w = a.add_sets(s, lo, hi, off), b.add_sets(tw, lo, hi, off)
                same_call(r, w, k)
                assert np.array_equal(r["set_first"], w["set_first"]), (k, "set_first")
            else:
                r, w = a.add_sets_first(s, lo, hi, off), b.add_sets_first(tw, lo, hi, off)
                for key in ("first", "stored", "fired", "chosen", "out", "tst", "ast", "set_first"):
                    assert np.array_equal(r[key], w[key]), (k, key)
                w = c.add_sets(tw, lo, hi, off)  # the twin's exact statuses
                unchecked += check_contract(r, w, off, k)
            res["rejected_by_twin"] += int((w["vst"] != OK).sum())
            res["calls"].append(r)
            res["twin"].append(w)
        res["count"], res["flag"] = a.state()
        cb, fb = b.state()
        assert np.array_equal(res["count"], cb) and np.array_equal(res["flag"], fb), "hbls_duty_state against the twin's"
        res["stats"], res["set_stats"], res["first_stats"] = a.stats(), a.set_stats(), a.first_stats()
        assert res["stats"] == b.stats(), "hbls_duty_stats against the twin's"
        sa, sb = res["set_stats"], b.set_stats()
        if mode == "first":  # out[2] counts the partials *reported* OK: exact against the exact twin up to the UNCHECKED ones
            sc = c.set_stats()
            assert sa[:2] == sb[:2] == sc[:2] and sc[2] - unchecked <= sa[2] <= sc[2], (sa, sb, sc)
            assert res["first_stats"][0] == b.first_stats()[0] and res["first_stats"][1] == unchecked
            assert res["stats"] == c.stats()
        else:
            assert sa == sb, "hbls_duty_set_stats against the twin's"
            assert res["first_stats"] == b.first_stats() == [0, 0]
    finally:
        for d in duties:
            if d is not None:
                d.close()
    return res
