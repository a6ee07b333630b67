"""The cases of tests/test_gpu_cluster_verify.py: hbls_cluster_verify_batch, hbls_cluster_verify_aggregate
and hbls_cluster_verify_stats through the ABI and callers.Cluster, -m gpu.  Not collected with the suite
(the name): that file runs this one once, in a process of its own, and says why.

The synthetic lock is tests/gpu_helpers/lock_check_cases.py's (6 validators, n = 4 shares, t = 3, built with
the library's own split), signed with hbls_sign_batch from the lock's own secrets; the reference locks are
the four of tests/golden/kat_reference.json.  The reference is the two defining properties of
include/hipbls.h, the twins: hbls_verify_batch with the named keys' 48 bytes (48 zero bytes where a pair
names no key) and hbls_verify_aggregate_batch over the selected keys in row-major order.  Beside each
twin stand the statuses the construction itself gives, so that a wrong twin cannot hide a wrong kernel.
Every comparison is exact.
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

from lock_check_cases import L, lock, N, T, V  # noqa: E402,F401 -- its fixtures: the same lock

OK, BAD_PUBKEY, BAD_SIGNATURE, NOT_VERIFIED = 0, 1, 2, 3
S8, S64 = 0xA5, 0xA5A5A5A5A5A5A5A5
PAD = 8
I64_MIN = -(1 << 63)
INF_PK = bytes([0xC0]) + bytes(47)
INF_SIG = bytes([0xC0]) + bytes(95)
BAD_SIG = b"\xff" * 96
M = [bytes([0x51]) * 32, bytes([0x52]) * 32, bytes([0x53]) * 32]
NONE = "no such cluster (never opened, or closed)"


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def neg_pk(pk):
    """the inverse of a finite compressed G1 point: the sign bit of its first byte"""
    return bytes([pk[0] ^ 0x20]) + bytes(pk[1:])


class Cl:
    """An open cluster over dv (V x 48 bytes) and pub (V x n x 48 bytes), with sentinels behind every output"""

    def __init__(self, L, dv, pub, tables=0):
        self.L, self.dv, self.pub = L, np.ascontiguousarray(dv), np.ascontiguousarray(pub)
        self.V, self.n = self.pub.shape[0], self.pub.shape[1]
        keys = self.V * (1 + self.n)
        st = np.full(keys + PAD, S8, np.uint8)
        h = ctypes.c_uint64(0)
        assert L.hbls_cluster_open(_p(self.dv), _p(self.pub), self.V, self.n, tables, _p(st), ctypes.byref(h)) == 0, \
            L.hbls_last_error().decode()
        self.h, self.key_status = h.value, st[:keys].reshape(self.V, 1 + self.n)
        assert (st[keys:] == S8).all()

    def key(self, g, j):
        """the lock's 48 bytes for (g, j), or 48 zero bytes where the pair names no key: the twin's pks"""
        if not 0 <= g < self.V or not 0 <= j <= self.n:
            return bytes(48)
        return bytes(self.dv[g]) if j == 0 else bytes(self.pub[g, j - 1])

    def selected(self, mask, with_dv):
        """the selected keys' 48-byte forms in row-major order: the aggregate twin's group"""
        sel = ([0] if with_dv else []) + [j for j in range(1, self.n + 1) if (mask >> (j - 1)) & 1]
        return [self.key(g, j) for g in range(self.V) for j in sel]

    def verify(self, items, handle=None, null=()):
        """items: (group, key_idx, msg, sig) -> (rc, statuses or None when rc != 0 and nothing was written)"""
        n = len(items)
        group = np.array([g for g, _, _, _ in items], np.uint32)
        idx = np.array([j for _, j, _, _ in items], np.int64)
        sigs = np.frombuffer(b"".join(s for _, _, _, s in items), np.uint8).copy() if n else np.zeros(1, np.uint8)
        msgs = np.frombuffer(b"".join(m for _, _, m, _ in items) or b"\0", np.uint8).copy()
        length = np.array([len(m) for _, _, m, _ in items], np.uint32)
        off = np.concatenate([[0], np.cumsum(length)[:-1]]).astype(np.uint64) if n else np.zeros(0, np.uint64)
        st = np.full(n + PAD, S8, np.uint8)
        a = dict(group=group, idx=idx, sigs=sigs, msgs=msgs, off=off, length=length, st=st)
        for k in null:
            a[k] = None
        rc = self.L.hbls_cluster_verify_batch(self.h if handle is None else handle, _p(a["group"]), _p(a["idx"]),
                                              _p(a["sigs"]), _p(a["msgs"]), _p(a["off"]), _p(a["length"]), n, _p(a["st"]))
        assert (st[n:] == S8).all(), "sentinels behind status"
        if rc != 0:
            assert (st == S8).all(), "a call error wrote"
            return rc, None
        return rc, st[:n].tolist()

    def aggregate(self, mask, with_dv, sig, msg, handle=None, null=()):
        """-> (rc, status or None when rc != 0 and nothing was written)"""
        st = np.full(1 + PAD, S8, np.uint8)
        sg = np.frombuffer(sig, np.uint8).copy()
        mg = np.frombuffer(msg or b"\0", np.uint8).copy()
        rc = self.L.hbls_cluster_verify_aggregate(self.h if handle is None else handle, mask, with_dv,
                                                  None if "sig" in null else _p(sg), None if "msg" in null else _p(mg),
                                                  len(msg), None if "status" in null else _p(st))
        assert (st[1:] == S8).all(), "sentinels behind status"
        if rc != 0:
            assert (st == S8).all(), "a call error wrote"
            return rc, None
        return rc, int(st[0])

    def _ctr(self, fn, n):
        out = np.full(n + 2, S64, np.uint64)
        assert fn(self.h, _p(out), n) == 0, self.L.hbls_last_error().decode()
        assert (out[n:] == S64).all()
        return [int(x) for x in out[:n]]

    def stats(self):
        return self._ctr(self.L.hbls_cluster_stats, 6)

    def check_stats(self):
        return self._ctr(self.L.hbls_cluster_check_stats, 2)

    def vstats(self, n=5):
        return self._ctr(self.L.hbls_cluster_verify_stats, n)

    def close(self):
        assert self.L.hbls_cluster_close(self.h) == 0, self.L.hbls_last_error().decode()


def secret(lock, g, j):
    return lock["secrets"][g] if j == 0 else lock["shares"][g][j - 1]


@pytest.fixture(scope="module")
def signed(hipbls, lock):
    return make_signed(hipbls, lock)


def make_signed(hipbls, lock):
    """{(g, j, m): the signature of M[m] under key (g, j) of the lock} for every pair over two messages"""
    keys = [(g, j, m) for m in (0, 1) for g in range(V) for j in range(N + 1)]
    sigs = hipbls.sign_batch([secret(lock, g, j) for g, j, _ in keys], [M[m] for _, _, m in keys])
    return dict(zip(keys, sigs))


def bad_key_lock(lock):
    """validator 1's pubshare 4 does not decode; validator 3's pubshare 2 is the point at infinity (status 0)"""
    pub = lock["pub"].copy()
    pub[1, 3] = 0xFF
    pub[3, 1] = np.frombuffer(INF_PK, np.uint8)
    return lock["dv"].copy(), pub


# ---- 1
def ref_lock(k):
    dv = np.frombuffer(b"".join(bytes.fromhex(v["dpk"]) for v in k["validators"]), np.uint8).reshape(-1, 48).copy()
    pub = np.frombuffer(b"".join(bytes.fromhex(s) for v in k["validators"] for s in v["shares"]), np.uint8)
    return dv, pub.reshape(len(dv), -1, 48).copy()


def test_reference_locks(L, hipbls, kats):
    shapes = []
    for k in kats["locks"]:
        dv, pub = ref_lock(k)
        shapes.append((pub.shape[0], pub.shape[1]))
        sig, lock_hash = bytes.fromhex(k["signature_aggregate"]), bytes.fromhex(k["lock_hash"])
        flipped = bytes([lock_hash[0] ^ 1]) + lock_hash[1:]
        regs = [(g, bytes.fromhex(v["registration"]["msg"]), bytes.fromhex(v["registration"]["sig"]))
                for g, v in enumerate(k["validators"]) if "registration" in v]
        for tables in (1, 0):
            cl = Cl(L, dv, pub, tables)
            try:
                assert not cl.key_status.any()
                all_shares = (1 << cl.n) - 1
                assert cl.aggregate(all_shares, 0, sig, lock_hash) == (0, OK)
                assert cl.aggregate(all_shares, 0, sig, flipped) == (0, NOT_VERIFIED)
                assert cl.aggregate(all_shares, 1, sig, lock_hash) == (0, NOT_VERIFIED), "the DV keys are not in the aggregate"
                assert hipbls.verify_aggregate_batch([cl.selected(all_shares, 0)] * 2, [sig] * 2, [lock_hash, flipped]) == \
                    [OK, NOT_VERIFIED], "the twin"
                if regs:
                    assert cl.verify([(g, 0, m, s) for g, m, s in regs]) == (0, [OK] * len(regs))
                    assert cl.verify([(g, 1, m, s) for g, m, s in regs]) == (0, [NOT_VERIFIED] * len(regs))
                assert cl.vstats() == [2 if regs else 0, 2 * len(regs), 0, 3, (2 * cl.n + cl.n + 1) * cl.V]
            finally:
                cl.close()
    assert shapes == [(5, 4), (1, 6), (1, 4), (3, 4)] and "registration" in kats["locks"][3]["validators"][0]


# ---- 2
NO_KEY_PAIRS = [(V, 1), (0xFFFFFFFF, 0), (V + 1000, N), (0, -1), (0, N + 1), (2, (1 << 32) + 1), (2, 1 << 32), (5, I64_MIN),
                (1, (1 << 32) + N), (3, -(1 << 32) + 1)]


def batch_items(signed):
    """-> (items, the statuses the construction gives)"""
    items, want = [], []
    for (g, j, m), s in signed.items():          # every (validator, 0 .. 4) pair over two messages
        items.append((g, j, M[m], s))
        want.append(OK)
    items.append((0, 1, M[2], signed[0, 1, 0]))   # a wrong message
    items.append((1, 2, M[0], signed[1, 3, 0]))   # a signature under the neighbouring share
    items.append((2, 0, M[0], signed[3, 0, 0]))   # a DV signature of another validator
    items.append((4, 0, M[1], signed[4, 1, 1]))   # a partial offered as the DV key's
    want += [NOT_VERIFIED] * 4
    items.append((3, 4, M[1], BAD_SIG))           # undecodable signature bytes
    want.append(BAD_SIGNATURE)
    items.append((5, 2, M[0], INF_SIG))           # the identity signature
    want.append(NOT_VERIFIED)
    for g, j in NO_KEY_PAIRS:                     # every pair that names no key, under a signature that would verify
        items.append((g, j, M[0], signed[0, 1, 0]))
        want.append(BAD_PUBKEY)
    items.append((V, 0, M[0], BAD_SIG))           # no key decides before the signature's decoding
    want.append(BAD_PUBKEY)
    return items, want


def twin_batch(hipbls, cl, items):
    return hipbls.verify_batch([cl.key(g, j) for g, j, _, _ in items], [m for _, _, m, _ in items], [s for _, _, _, s in items])


def padded(items, n):
    """the call padded past n items by repeating its good items (the first 2 V (1 + N) of batch_items)"""
    good = items[:2 * V * (1 + N)]
    out = list(items)
    while len(out) <= n:
        out += good
    return out


def run_batch_cases(L, hipbls, lock, signed):
    """Every verify-batch call of case 2 -> [(name, statuses)], each asserted against its twin"""
    res = []
    items, want = batch_items(signed)
    for tables in (0, 1):
        cl = Cl(L, lock["dv"], lock["pub"], tables)
        try:
            calls = [items]
            rc, st = cl.verify(items)
            assert rc == 0 and st == want, "the construction"
            assert st == twin_batch(hipbls, cl, items), "the twin"
            res.append((f"plain tables={tables}", st))
            # past HBLS_SINGLE_MAX (128: groups of up to 16 over one message, the combination ladders and the
            # ladder tables) and past HBLS_FE_BATCH (128 groups: the batched final exponentiation)
            for n in (128, 16 * 128):
                big = padded(items, n)
                calls.append(big)
                rc, st = cl.verify(big)
                assert rc == 0 and st[:len(items)] == want and set(st[len(items):]) == {OK}
                assert st == twin_batch(hipbls, cl, big), "the twin"
                res.append((f"padded past {n} tables={tables}", st))
            named = [sum(1 for g, j, _, _ in its if cl.key(g, j) != bytes(48)) for its in calls]
            assert cl.vstats() == [3, sum(named), sum(len(its) for its in calls) - sum(named), 0, 0]
        finally:
            cl.close()
    # a lock with an undecodable pubshare and one at infinity: items name each
    dv, pub = bad_key_lock(lock)
    for tables in (0, 1):
        cl = Cl(L, dv, pub, tables)
        try:
            want_ks = np.zeros((V, 1 + N), np.uint8)
            want_ks[1, 4] = BAD_PUBKEY
            assert np.array_equal(cl.key_status, want_ks), "the key at infinity opens with status 0"
            extra = [(1, 4, M[0], signed[1, 4, 0]), (1, 4, M[0], BAD_SIG), (3, 2, M[0], signed[3, 2, 0]), (3, 2, M[0], INF_SIG),
                     (1, 3, M[0], signed[1, 3, 0]), (3, 1, M[1], signed[3, 1, 1])]
            rc, st = cl.verify(extra)
            assert rc == 0 and st == [BAD_PUBKEY, BAD_PUBKEY, NOT_VERIFIED, NOT_VERIFIED, OK, OK]
            assert st == twin_batch(hipbls, cl, extra), "the twin"
            res.append((f"bad keys tables={tables}", st))
            big = padded(items, 128) + extra
            rc, st = cl.verify(big)
            assert rc == 0 and st == twin_batch(hipbls, cl, big), "the twin"
            assert st[-len(extra):] == [BAD_PUBKEY, BAD_PUBKEY, NOT_VERIFIED, NOT_VERIFIED, OK, OK]
            res.append((f"bad keys padded tables={tables}", st))
        finally:
            cl.close()
    return res


@pytest.fixture(scope="module")
def batch_unsplit(L, hipbls, lock, signed):
    return run_batch_cases(L, hipbls, lock, signed)


def test_twin_of_verify_batch(batch_unsplit):
    assert len(batch_unsplit) == 10


# ---- 3
SELECTIONS = [("all shares", 0b1111, 0), ("dv only", 0, 1), ("shares 1 3", 0b0101, 0), ("share 2 and dv", 0b0010, 1),
              ("empty", 0, 0)]


def sel_entries(mask, with_dv):
    return ([0] if with_dv else []) + [j for j in range(1, N + 1) if (mask >> (j - 1)) & 1]


def agg_sig(hipbls, lock, pairs, msg):
    """the aggregate of msg's signatures under exactly the secrets of `pairs` [(g, j)] (none: the identity)"""
    if not pairs:
        return INF_SIG
    sigs = hipbls.sign_batch([secret(lock, g, j) for g, j in pairs], [msg] * len(pairs))
    out, st = hipbls.aggregate_batch([sigs])
    assert st == [OK]
    return out[0]


def twin_agg(hipbls, cl, mask, with_dv, sig, msg):
    return hipbls.verify_aggregate_batch([cl.selected(mask, with_dv)], [sig], [msg])[0]


def run_aggregate_cases(L, hipbls, lock):
    """Every aggregate call of case 3 -> [(name, status)], each asserted against its twin"""
    res = []
    msg = M[2]
    own = {name: agg_sig(hipbls, lock, [(g, j) for g in range(V) for j in sel_entries(mask, dv)], msg)
           for name, mask, dv in SELECTIONS}
    for tables in (0, 1):
        cl = Cl(L, lock["dv"], lock["pub"], tables)
        try:
            calls = 0
            for k, (name, mask, dv) in enumerate(SELECTIONS):
                other = SELECTIONS[(k + 1) % len(SELECTIONS)][0]
                for what, sig, m, want in (("own", own[name], msg, NOT_VERIFIED if name == "empty" else OK),
                                           ("other", own[other], msg, NOT_VERIFIED),
                                           ("other message", own[name], M[0], NOT_VERIFIED),
                                           ("undecodable", BAD_SIG, msg, BAD_SIGNATURE),
                                           ("identity", INF_SIG, msg, NOT_VERIFIED)):
                    rc, st = cl.aggregate(mask, dv, sig, m)
                    calls += 1
                    assert (rc, st) == (0, want), (name, what, "the construction")
                    assert st == twin_agg(hipbls, cl, mask, dv, sig, m), (name, what, "the twin")
                    res.append((f"{name} / {what} tables={tables}", st))
            per_call = sum(len(sel_entries(mask, dv)) for _, mask, dv in SELECTIONS) * 5 * V
            assert cl.vstats() == [0, 0, 0, calls, per_call]
        finally:
            cl.close()
    # the bad-key lock: the undecodable pubshare (1, 4) selected and unselected; the key at infinity (3, 2) selected
    dv, pub = bad_key_lock(lock)
    cl = Cl(L, dv, pub)
    try:
        no_inf = agg_sig(hipbls, lock, [(g, 2) for g in range(V) if g != 3], msg)
        for name, mask, wdv, sig, want in (
                ("bad key selected", 0b1111, 0, own["all shares"], BAD_PUBKEY),
                ("bad key selected, undecodable signature", 0b1000, 0, BAD_SIG, BAD_SIGNATURE),
                ("bad key selected, identity signature", 0b1000, 1, INF_SIG, BAD_PUBKEY),
                ("bad key unselected", 0b0101, 0, own["shares 1 3"], OK),
                ("a key at infinity is the identity in the sum", 0b0010, 0, no_inf, OK),
                ("a key at infinity, the signature over all six", 0b0010, 0,
                 agg_sig(hipbls, lock, [(g, 2) for g in range(V)], msg), NOT_VERIFIED)):
            rc, st = cl.aggregate(mask, wdv, sig, msg)
            assert (rc, st) == (0, want), (name, "the construction")
            assert st == twin_agg(hipbls, cl, mask, wdv, sig, msg), (name, "the twin")
            res.append((name, st))
    finally:
        cl.close()
    # pubshare 2 is the inverse of pubshare 1 in every row: under shares {1, 2} the sum is the identity
    pub = lock["pub"].copy()
    for g in range(V):
        pub[g, 1] = np.frombuffer(neg_pk(bytes(pub[g, 0])), np.uint8)
    cl = Cl(L, lock["dv"], pub, 1)
    try:
        assert not cl.key_status.any()
        for name, mask, wdv, sig, want in (
                ("inverse pair, identity signature", 0b0011, 0, INF_SIG, NOT_VERIFIED),
                ("inverse pair, a signature", 0b0011, 0, own["shares 1 3"], NOT_VERIFIED),
                ("inverse pair and share 3", 0b0111, 0, agg_sig(hipbls, lock, [(g, 3) for g in range(V)], msg), OK),
                ("inverse pair and the dv key", 0b0011, 1, own["dv only"], OK)):
            rc, st = cl.aggregate(mask, wdv, sig, msg)
            assert (rc, st) == (0, want), (name, "the construction")
            assert st == twin_agg(hipbls, cl, mask, wdv, sig, msg), (name, "the twin")
            res.append((name, st))
    finally:
        cl.close()
    return res


@pytest.fixture(scope="module")
def aggregate_unsplit(L, hipbls, lock):
    return run_aggregate_cases(L, hipbls, lock)


def test_twin_of_verify_aggregate(aggregate_unsplit):
    assert len(aggregate_unsplit) == 2 * 25 + 6 + 4


# ---- 4
@pytest.mark.parametrize("copies", [2, 3])
def test_shards(L, hipbls, lock, signed, kats, batch_unsplit, aggregate_unsplit, copies):
    want = batch_unsplit, aggregate_unsplit
    k = kats["locks"][1]  # one validator: under three contexts two of them have no row
    dv, pub = ref_lock(k)
    sig, lock_hash = bytes.fromhex(k["signature_aggregate"]), bytes.fromhex(k["lock_hash"])
    devices = L.hbls_device_count()
    try:
        assert L.hbls_debug_split(copies) == 0 and L.hbls_device_count() == copies * devices
        got = run_batch_cases(L, hipbls, lock, signed), run_aggregate_cases(L, hipbls, lock)
        cl = Cl(L, dv, pub, 1)
        try:
            assert pub.shape[:2] == (1, 6)
            assert cl.aggregate(0b111111, 0, sig, lock_hash) == (0, OK)
            assert cl.aggregate(0b111111, 0, sig, M[0]) == (0, NOT_VERIFIED)
            assert cl.aggregate(0, 0, sig, lock_hash) == (0, NOT_VERIFIED)
            assert cl.verify([(0, 1, M[0], BAD_SIG), (1, 0, M[0], BAD_SIG)]) == (0, [BAD_SIGNATURE, BAD_PUBKEY])
        finally:
            assert L.hbls_debug_split(1) == 0
            again = cl.aggregate(0b111111, 0, sig, lock_hash)  # the cluster keeps the shards it was opened under
            cl.close()
    finally:
        assert L.hbls_debug_split(1) == 0
    assert got == want and again == (0, OK)


# ---- 5
def duty_run(hipbls, cl, lock, between):
    """Every validator's partials of share indices 1 .. T through a duty on the cluster, between() behind every add
    -> every output of every add, then hbls_duty_state"""
    from charon_amd.tbls import Duty
    msgs = [bytes([0x40 + v]) * 32 for v in range(V)]
    res = []
    with Duty(hipbls._L, (), T, 16, cluster=(cl.h, V)) as du:
        for j in range(1, T + 1):
            sigs = hipbls.sign_batch([lock["shares"][v][j - 1] for v in range(V)], msgs)
            if j == 2:
                sigs[3] = BAD_SIG
            r = du.add(None, msgs, sigs, list(range(V)), [j] * V)
            res.append((r.vstatus, r.stored, r.first_serial, r.fired, r.chosen, r.aggregates, r.ta_status, r.agg_vstatus))
            between()
        res.append(du.state())
    return res


def test_verifies_only_read(L, hipbls, lock, signed):
    items, want = batch_items(signed)
    sig = agg_sig(hipbls, lock, [(g, j) for g in range(V) for j in range(1, N + 1)], M[2])
    for tables in (0, 1):
        a, b = Cl(L, lock["dv"], lock["pub"], tables), Cl(L, lock["dv"], lock["pub"], tables)
        try:
            def between():
                assert a.verify(items) == (0, want)
                assert a.aggregate(0b1111, 0, sig, M[2]) == (0, OK)
                assert a.aggregate(1 << N, 0, sig, M[2])[0] == -1, "a failed call"
                assert a.verify(items, null=("sigs",))[0] == -1, "a failed call"
            ra, rb = duty_run(hipbls, a, lock, between), duty_run(hipbls, b, lock, lambda: None)
            assert ra == rb, "every output of every add and hbls_duty_state"
            assert ra[-2][3] == [0, 1, 2, 4, 5] and ra[1][0][3] == BAD_SIGNATURE, "the duty did fire, and did reject"
            assert a.stats() == b.stats() and a.check_stats() == b.check_stats() == [0, 0]
            named = sum(1 for g, j, _, _ in items if a.key(g, j) != bytes(48))
            assert a.vstats() == [T, T * named, T * (len(items) - named), T, T * N * V], "exactly the calls that returned 0"
            assert b.vstats() == [0] * 5
            assert a.vstats(2) == [T, T * named] and a.vstats(0) == []
        finally:
            a.close()
            b.close()


# ---- 6
def test_call_errors_write_nothing(L, lock, signed):
    cl = Cl(L, lock["dv"], lock["pub"])
    items = [(0, 1, M[0], signed[0, 1, 0]), (1, 0, M[1], signed[1, 0, 1])]
    sig = signed[0, 1, 0]

    def err(r):
        assert r == (-1, None)
        msg = L.hbls_last_error().decode()
        assert msg
        return msg

    try:
        for h in (0, cl.h + 1000):  # never issued
            assert err(cl.verify(items, handle=h)) == "hbls_cluster_verify_batch: " + NONE
            assert err(cl.verify([], handle=h)) == "hbls_cluster_verify_batch: " + NONE
            assert err(cl.aggregate(1, 0, sig, M[0], handle=h)) == "hbls_cluster_verify_aggregate: " + NONE
        for k in ("group", "idx", "sigs", "off", "length", "st"):
            assert "are required" in err(cl.verify(items, null=(k,))), k
        assert "msgs is required" in err(cl.verify(items, null=("msgs",)))
        assert "n_shares (4)" in err(cl.aggregate(1 << N, 0, sig, M[0])), "a mask bit at n_shares"
        assert "n_shares (4)" in err(cl.aggregate(1 << 63, 0, sig, M[0]))
        assert "with_dv" in err(cl.aggregate(1, 2, sig, M[0]))
        for k in ("sig", "status", "msg"):
            assert "are required" in err(cl.aggregate(1, 0, sig, M[0], null=(k,))), k
        out = np.full(8, S64, np.uint64)
        assert L.hbls_cluster_verify_stats(cl.h + 1000, _p(out), 5) == -1
        assert L.hbls_cluster_verify_stats(cl.h, _p(out), 6) == -1
        assert L.hbls_last_error().decode() == "hbls_cluster_verify_stats: out is null or n above 5"
        assert L.hbls_cluster_verify_stats(cl.h, None, 1) == -1 and (out == S64).all()
        assert cl.vstats() == [0] * 5, "a call error counts nothing"
        # valid: n == 0 writes nothing (null pointers and all); an empty message with a NULL msg
        assert cl.verify([]) == (0, [])
        assert cl.verify([], null=("group", "idx", "sigs", "msgs", "off", "length", "st")) == (0, [])
        assert cl.aggregate(1, 0, sig, b"", null=("msg",)) == (0, NOT_VERIFIED)
        assert cl.vstats() == [2, 0, 0, 1, V]
        assert cl.stats()[3:] == [0, 0, 0] and cl.check_stats() == [0, 0], "the other counters are not touched"
    finally:
        closed = cl.h
        cl.close()
    assert err(cl.verify(items, handle=closed)) == "hbls_cluster_verify_batch: " + NONE
    assert err(cl.aggregate(1, 0, sig, M[0], handle=closed)) == "hbls_cluster_verify_aggregate: " + NONE


# ---- 7: the kernels each call enqueues, in order, against tests/golden/cluster_traces.json
def test_launch_traces(L, hipbls, lock, signed):
    """The fixture was recorded by tests/golden/make_cluster_traces.py with the library of the commit before the
    handle layer's shard runner, buffer owner, handle table and counter reader became one each; a change that
    is not meant to alter the launch sequences must reproduce them.  Name by name, except the two-shard
    traces (SORTED there): their shard threads race, so those compare as sorted lists."""
    import json
    golden = os.path.join(ROOT, "tests", "golden")
    if golden not in sys.path:
        sys.path.insert(0, golden)
    import make_cluster_traces as mc
    with open(mc.PATH) as f:
        want = json.load(f)["traces"]
    assert set(want) == {t for c in mc.CASES for t in mc.TRACES[c]} and mc.SORTED <= set(want)
    got = mc.run_cases(mc.Ctx(L, hipbls, lock, signed))
    assert set(got) == set(want)
    for name, names in got.items():
        assert names, name
        a, b = (sorted(names), sorted(want[name])) if name in mc.SORTED else (names, want[name])
        diff = next((f"launch {k}: {x} (recorded: {y})" for k, (x, y) in enumerate(zip(a, b)) if x != y),
                    f"{len(a)} launches (recorded: {len(b)})")
        assert a == b, (name, diff)
    # the cases do take different paths
    assert "k_cluster_wide" in got["cluster_open_tables1"] and "k_cluster_wide" not in got["cluster_open_tables0"]
    assert got["cluster_check"].count("k_lock_check") == 1
    assert "k_cluster_row_sum" in got["cluster_verify_aggregate_all"]
    assert "k_cluster_row_sum" not in got["cluster_verify_aggregate_empty"]
    assert got["cluster_verify_aggregate_split2"].count("k_cluster_row_sum") == 2
    assert "k_duty_gather" in got[f"cluster_duty_add_{T}"] and "k_duty_gather" not in got["cluster_duty_add_1"]


# ---- 8: the Python layer
def test_callers_cluster(hipbls, kats):
    from charon_amd import callers
    from charon_amd.tbls import TblsError
    k = kats["locks"][3]
    vals = k["validators"]
    keys = [bytes.fromhex(v["dpk"]) for v in vals]
    shares = {pk: {j + 1: bytes.fromhex(s) for j, s in enumerate(v["shares"])} for pk, v in zip(keys, vals)}
    sig, lock_hash = bytes.fromhex(k["signature_aggregate"]), bytes.fromhex(k["lock_hash"])
    regs = {pk: (bytes.fromhex(v["registration"]["msg"]), bytes.fromhex(v["registration"]["sig"])) for pk, v in zip(keys, vals)}
    flat = [s for pk in keys for s in shares[pk].values()]
    for tables in (False, True):
        with callers.Cluster(hipbls, {pk: pk for pk in keys}, shares, ladder_tables=tables) as cl:
            assert cl.verify([(pk, 0) + regs[pk] for pk in keys]) == [OK] * 3
            assert cl.verify([]) == []
            assert cl.verify_aggregate(sig, lock_hash) == OK
            assert cl.verify_aggregate(sig, lock_hash, shares=[1, 2, 3, 4]) == OK
            assert cl.verify_aggregate(sig, lock_hash, shares=[1, 2, 3]) == NOT_VERIFIED
            assert cl.verify_aggregate(sig, lock_hash, with_dv=True) == NOT_VERIFIED
            assert cl.verify_lock_signatures(sig, lock_hash) is None
            assert cl.verify_lock_signatures(sig, lock_hash, regs) is None
            # a tampered aggregate: the same string as lock_verify_signatures
            bad = bytes([lock_hash[0] ^ 1]) + lock_hash[1:]
            with pytest.raises(callers.CallerError) as e1:
                cl.verify_lock_signatures(sig, bad, regs)
            with pytest.raises(callers.CallerError) as e2:
                callers.lock_verify_signatures(hipbls, flat, sig, bad)
            assert str(e1.value) == str(e2.value) and str(e1.value).startswith("verify lock signature aggregate: ")
            # a tampered second registration: lock.go's chain around the tbls.Verify error
            bad_regs = dict(regs)
            bad_regs[keys[1]] = (regs[keys[1]][0], regs[keys[2]][1])
            with pytest.raises(callers.CallerError) as e3:
                cl.verify_lock_signatures(sig, lock_hash, bad_regs)
            with pytest.raises(TblsError) as e4:
                hipbls.verify(keys[1], *bad_regs[keys[1]])
            assert str(e3.value) == "verify pre-generated builder registrations: verify builder registration signature: " + str(e4.value)
            # a validator pubkey that is not in the cluster: the library itself answers
            stranger = bytes.fromhex(kats["locks"][0]["validators"][0]["dpk"])
            assert cl.verify([(stranger, 0) + regs[keys[0]], (keys[0], 0) + regs[keys[0]], (keys[0], 5) + regs[keys[0]]]) == \
                [BAD_PUBKEY, OK, BAD_PUBKEY]
            with pytest.raises(TblsError, match="n_shares"):
                cl.verify_aggregate(sig, lock_hash, shares=[5])
            assert cl.verify_stats() == {"verify_calls": 4, "items_resolved": 3 + 3 + 3 + 1, "items_no_key": 2,
                                         "aggregate_calls": 8, "aggregate_keys": 3 * (4 + 4 + 3 + 5 + 4 + 4 + 4 + 4)}
