"""The cases of tests/test_gpu_lock_check.py: hbls_cluster_check through the ABI and callers.Cluster, -m gpu.
Not collected with the suite (the name): that file runs this one once, in a process of its own, and says
why.

The lock is built with the library's own hbls_threshold_split and hbls_secret_to_public_key_batch: 6
validators, n = 4 shares, t = 3.  Expected statuses and masks are stated from the criterion (a single
wrong key at p fails the windows k <= p <= k + t) and recomputed by the oracle restatement
(tests/gpu_helpers/lock_check.py check_points) over the lock's decompressed keys.  Every comparison is exact.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HELPERS = os.path.join(ROOT, "tests", "gpu_helpers")
for p in (ROOT, HELPERS):
    if p not in sys.path:
        sys.path.insert(0, p)

import lock_check as lc  # noqa: E402
from oracle import bls12381 as B  # noqa: E402

OK, BAD_PUBKEY, NOT_VERIFIED = 0, 1, 3
V, N, T = 6, 4, 3
S8, S64 = 0xA5, 0xA5A5A5A5A5A5A5A5
PAD = 8


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def L(hipbls):
    return hipbls._L


@pytest.fixture(scope="module")
def lock(hipbls):
    return make_lock(hipbls)


def make_lock(hipbls):
    """Per validator: the secret, its N share secrets, the DV key and the N pubshares, by the library's own split"""
    secrets, shares = [], []
    for v in range(V):
        sk = (0x1000003 * (v + 1) + 17).to_bytes(32, "big")
        coeffs = [(0x2000003 * (v + 1) + 101 * (k + 1)).to_bytes(32, "big") for k in range(T - 1)]
        sh = hipbls._split(sk, N, T, coeffs)
        secrets.append(sk)
        shares.append([sh[j] for j in range(1, N + 1)])
    sks = b"".join(secrets) + b"".join(s for row in shares for s in row)
    out = ctypes.create_string_buffer(48 * V * (1 + N))
    st = ctypes.create_string_buffer(V * (1 + N))
    assert hipbls._L.hbls_secret_to_public_key_batch(sks, V * (1 + N), out, st) == 0 and not any(st.raw)
    pks = np.frombuffer(out.raw, np.uint8).reshape(V * (1 + N), 48)
    return dict(secrets=secrets, shares=shares, dv=pks[:V].copy(), pub=pks[V:].reshape(V, N, 48).copy())


def bad_lock(lock):
    """validator 2's shares 1 and 3 swapped -- pubshares and the share secrets their holders sign with alike, as a
    lock that misnumbers two operators -- and validator 4's DV key replaced by validator 0's"""
    dv, pub = lock["dv"].copy(), lock["pub"].copy()
    pub[2, 0], pub[2, 2] = lock["pub"][2, 2], lock["pub"][2, 0]
    dv[4] = lock["dv"][0]
    shares = [list(r) for r in lock["shares"]]
    shares[2][0], shares[2][2] = shares[2][2], shares[2][0]
    return dict(lock, dv=dv, pub=pub, shares=shares)


class Cl:
    def __init__(self, L, lk, tables=0):
        self.L = L
        st = np.full(V * (1 + N) + PAD, S8, np.uint8)
        h = ctypes.c_uint64(0)
        assert L.hbls_cluster_open(_p(np.ascontiguousarray(lk["dv"])), _p(np.ascontiguousarray(lk["pub"])), V, N, tables,
                                   _p(st), ctypes.byref(h)) == 0, L.hbls_last_error().decode()
        self.h, self.key_status = h.value, st[:V * (1 + N)].reshape(V, 1 + N)
        assert (st[V * (1 + N):] == S8).all()

    def check(self, t, windows=True, n_bad=True, handle=None):
        """-> (rc, row_status, row_windows, n_bad), sentinels behind the outputs checked"""
        st = np.full(V + PAD, S8, np.uint8)
        win = np.full(V + PAD, S64, np.uint64)
        nb = ctypes.c_size_t(777)
        rc = self.L.hbls_cluster_check(self.h if handle is None else handle, t, _p(st), _p(win) if windows else None,
                                       ctypes.byref(nb) if n_bad else None)
        assert (st[V:] == S8).all() and (win[V:] == S64).all(), "sentinels behind row_status / row_windows"
        if not windows:
            assert (win == S64).all()
        if not n_bad:
            assert nb.value == 777
        return rc, st[:V].tolist(), [int(w) for w in win[:V]], nb.value

    def stats(self, n=6):
        out = np.full(n + 2, S64, np.uint64)
        assert self.L.hbls_cluster_stats(self.h, _p(out), n) == 0, self.L.hbls_last_error().decode()
        assert (out[n:] == S64).all()
        return [int(x) for x in out[:n]]

    def check_stats(self, n=2):
        out = np.full(n + 2, S64, np.uint64)
        assert self.L.hbls_cluster_check_stats(self.h, _p(out), n) == 0, self.L.hbls_last_error().decode()
        assert (out[n:] == S64).all()
        return [int(x) for x in out[:n]]

    def close(self):
        assert self.L.hbls_cluster_close(self.h) == 0, self.L.hbls_last_error().decode()


def oracle_rows(lk, t, key_status=None):
    """the oracle restatement over the lock's decompressed keys -> (row_status, row_windows)"""
    st, win = [], []
    for v in range(V):
        pts = [B.g1_decompress(bytes(lk["dv"][v]))] + [B.g1_decompress(bytes(lk["pub"][v, j])) for j in range(N)]
        s, w = lc.check_points(pts, [0] * (1 + N) if key_status is None else list(key_status[v]), t)
        st.append(s)
        win.append(w)
    return st, win


# 1
def test_an_honest_lock(L, lock):
    cl = Cl(L, lock)
    try:
        assert not cl.key_status.any()
        for t in (3, 4):  # degree 2 < 3 < 4
            assert cl.check(t) == (0, [OK] * V, [0] * V, 0)
        # at t = 2 the rows have degree 2: every second difference is 2 a_2 H, in every window
        assert cl.check(2) == (0, [NOT_VERIFIED] * V, [0b111] * V, V)
        assert cl.check(1) == (0, [NOT_VERIFIED] * V, [0b1111] * V, V)
        for t in (1, 2, 3, 4):
            r = cl.check(t)
            assert (r[1], r[2]) == oracle_rows(lock, t)
        assert cl.check_stats() == [8, 4 * V]
    finally:
        cl.close()


def duty_run(hipbls, cluster_handle, lk, t):
    """Every validator's partials of share indices 1 .. t, peer-major, through a duty on the cluster, each signed with
    the share secret the lock's holder of that index has -> per add the call's outputs"""
    from charon_amd.tbls import Duty
    msgs = [bytes([0x40 + v]) * 32 for v in range(V)]
    res = []
    with Duty(hipbls._L, (), t, 16, cluster=(cluster_handle, V)) as du:
        for j in range(1, t + 1):
            sigs = hipbls.sign_batch([lk["shares"][v][j - 1] for v in range(V)], msgs)
            r = du.add(None, msgs, sigs, list(range(V)), [j] * V)
            res.append((r.vstatus, r.stored, r.first_serial, r.fired, r.chosen, r.aggregates, r.ta_status, r.agg_vstatus))
    return res


# 2
def test_a_lock_with_swapped_pubshares_and_a_wrong_dv_key(L, hipbls, lock):
    bad = bad_lock(lock)
    cl = Cl(L, bad)
    try:
        assert not cl.key_status.any(), "the open sees nothing: every key decodes and is in the subgroup"
        want_st = [OK, OK, NOT_VERIFIED, OK, NOT_VERIFIED, OK]
        # validator 2: positions 1 and 3 lie in both windows (0..3 and 1..4) and the coefficient differences
        # c_1 - c_3 = 2, c_0 - c_2 = 2 do not cancel; validator 4: position 0 lies in window 0 alone
        want_win = [0, 0, 0b11, 0, 0b01, 0]
        assert cl.check(T) == (0, want_st, want_win, 2)
        assert oracle_rows(bad, T) == (want_st, want_win)
        assert cl.check_stats() == [1, 2]
        # the failure the check predicts: every partial verifies under its pubshare and is stored, every validator
        # fires, and the aggregates of exactly those two validators do not verify
        res = duty_run(hipbls, cl.h, bad, T)
        for vst, stored, *_ in res:
            assert vst == [OK] * V and stored == [1] * V
        fired, ta_status, agg = res[-1][3], res[-1][6], res[-1][7]
        assert fired == list(range(V)) and ta_status == [OK] * V
        assert agg == [OK, OK, NOT_VERIFIED, OK, NOT_VERIFIED, OK]
    finally:
        cl.close()
    good = Cl(L, lock)
    try:
        res = duty_run(hipbls, good.h, lock, T)
        assert res[-1][3] == list(range(V)) and res[-1][7] == [OK] * V, "the honest lock's duty fires clean"
    finally:
        good.close()


# 3
def test_call_errors_write_nothing(L, lock):
    cl = Cl(L, lock)

    def err(r):
        rc, st, win, nb = r
        assert st == [S8] * V and win == [S64] * V and nb == 777, "a call error wrote"
        return rc, L.hbls_last_error().decode()

    try:
        msg = "hbls_cluster_check: threshold must be in 1..4 (the cluster's n_shares)"
        for t in (0, N + 1, 65, 0xFFFFFFFF):
            assert err(cl.check(t)) == (-1, msg)
        none = "hbls_cluster_check: no such cluster (never opened, or closed)"
        for h in (0, cl.h + 1000):
            assert err(cl.check(T, handle=h)) == (-1, none)
        out = np.full(4, S64, np.uint64)
        assert L.hbls_cluster_check_stats(cl.h + 1000, _p(out), 2) == -1
        assert L.hbls_cluster_check_stats(cl.h, _p(out), 3) == -1
        assert L.hbls_last_error().decode() == "hbls_cluster_check_stats: out is null or n above 2"
        assert L.hbls_cluster_check_stats(cl.h, None, 1) == -1 and (out == S64).all()
        assert cl.check_stats() == [0, 0], "a call error counts nothing"
        # nullable outputs left null
        assert cl.check(T, windows=False)[:2] == (0, [OK] * V)
        assert cl.check(T, n_bad=False)[:3] == (0, [OK] * V, [0] * V)
        assert cl.check(2, windows=False, n_bad=False)[:2] == (0, [NOT_VERIFIED] * V)
        assert cl.check_stats() == [3, V] and cl.check_stats(1) == [3] and cl.check_stats(0) == []
    finally:
        closed = cl.h
        cl.close()
    assert err(cl.check(T, handle=closed)) == (-1, "hbls_cluster_check: no such cluster (never opened, or closed)")


# 4
def test_an_unusable_row_is_not_an_inconsistent_one(L, lock):
    lk = bad_lock(lock)
    lk["pub"][1, 3] = 0xFF  # validator 1's pubshare 4 does not decode
    lk["pub"][3, 1] = np.frombuffer(lc.INF, np.uint8)  # validator 3's pubshare 2 is the point at infinity: status 0
    cl = Cl(L, lk)
    try:
        want_ks = np.zeros((V, 1 + N), np.uint8)
        want_ks[1, 4] = BAD_PUBKEY
        assert np.array_equal(cl.key_status, want_ks)
        # validator 3: the identity at position 2, in both windows -- the group law decides
        want = (0, [OK, BAD_PUBKEY, NOT_VERIFIED, NOT_VERIFIED, NOT_VERIFIED, OK], [0, 0, 0b11, 0b11, 0b01, 0], 4)
        assert cl.check(T) == want
        lk2 = dict(lk, pub=lk["pub"].copy())
        lk2["pub"][1, 3] = lock["pub"][1, 3]  # (the oracle needs a key that decodes; its status decides before any sum)
        assert oracle_rows(lk2, T, want_ks) == (want[1], want[2])
        assert cl.check_stats() == [1, 3], "rows reported NOT_VERIFIED, not every bad row"
    finally:
        cl.close()


# 5
@pytest.mark.parametrize("copies", [2, 3])
def test_shards(L, lock, copies):
    lk = bad_lock(lock)
    lk["pub"][5, 0] = 0xFF
    one = Cl(L, lk)
    try:
        want = {t: one.check(t) for t in (1, 2, 3, 4)}
    finally:
        one.close()
    devices = L.hbls_device_count()
    try:
        assert L.hbls_debug_split(copies) == 0 and L.hbls_device_count() == copies * devices
        cl = Cl(L, lk)
        try:
            assert np.array_equal(cl.key_status, one.key_status)
            got = {t: cl.check(t) for t in (1, 2, 3, 4)}
        finally:
            assert L.hbls_debug_split(1) == 0
            again = cl.check(T)  # the cluster keeps the shards it was opened under
            cl.close()
    finally:
        assert L.hbls_debug_split(1) == 0
    assert got == want and again == want[T]
    assert want[T][1] == [OK, OK, NOT_VERIFIED, OK, NOT_VERIFIED, BAD_PUBKEY] and want[T][3] == 3


# 6
def test_a_check_changes_nothing_a_duty_returns(L, hipbls, lock):
    bad = bad_lock(lock)
    for tables in (0, 1):
        cl = Cl(L, bad, tables)
        try:
            before = duty_run(hipbls, cl.h, bad, T)
            stats = cl.stats()
            keys = V * (1 + N)
            assert stats == [keys, 0, keys * tables, T * V, 0, V]
            r = cl.check(T)
            assert cl.stats() == stats, "hbls_cluster_stats counts what it counted"
            assert cl.check_stats() == [1, 2]
            after = duty_run(hipbls, cl.h, bad, T)
            assert after == before
            assert cl.check(T) == r and cl.check_stats() == [2, 4]
            assert cl.stats() == [keys, 0, keys * tables, 2 * T * V, 0, 2 * V]
        finally:
            cl.close()


# 7: the Python layer
def test_callers_cluster(hipbls, lock):
    from charon_amd import callers
    from charon_amd.tbls import TblsError
    bad = bad_lock(lock)
    keys = [bytes(lock["dv"][v]) for v in range(V)]  # the validators' names: the honest DV keys
    dvs = {keys[v]: bytes(bad["dv"][v]) for v in range(V)}
    shares = {keys[v]: {j + 1: bytes(bad["pub"][v, j]) for j in range(N)} for v in range(V)}
    with callers.Cluster(hipbls, dvs, shares, ladder_tables=False) as cl:
        assert cl.check(T) == ([OK, OK, NOT_VERIFIED, OK, NOT_VERIFIED, OK], [0, 0, 0b11, 0, 0b01, 0])
        inc = cl.inconsistent(T)
        # validator 2: positions 1 .. 3 lie in both windows; validator 4: position 0 in window 0 alone -- the DV key
        assert inc == {keys[2]: (NOT_VERIFIED, [0, 1], [1, 2, 3]), keys[4]: (NOT_VERIFIED, [0], [0])}
        assert cl.check_stats() == {"checks": 2, "rows_not_verified": 4}
        with pytest.raises(TblsError, match="threshold must be in 1..4"):
            cl.check(0)
    honest = {keys[v]: {j + 1: bytes(lock["pub"][v, j]) for j in range(N)} for v in range(V)}
    with callers.Cluster(hipbls, {k: k for k in keys}, honest, ladder_tables=False) as cl:
        assert cl.inconsistent(T) == {} and cl.inconsistent(N) == {}
        assert sorted(cl.inconsistent(2)) == sorted(keys)
