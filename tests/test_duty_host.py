"""The host side of duty sessions on the CPU, through the g++ harness tests/native/dutycheck.cpp:
the storing and firing rule (charon_amd/csrc/dutysel.h duty_store_group, what duty.hip's k_duty_store
runs per lane) against a Python restatement, the defining property against the one-shot rule
(charon_amd/csrc/tasel.h ta_select_matching over the concatenation), and the host plan of
hbls_duty_add (charon_amd/csrc/hduty.h): message ids, routing, serials and the touched groups' CSR.
"""
import ctypes

import numpy as np
import pytest

NONE = 0xFFFFFFFF
FEW = 1


@pytest.fixture(scope="module")
def H():
    from gpu_helpers import harness
    lib = harness.load("dutycheck")
    lib.dc_session_new.restype = ctypes.c_void_p
    lib.dc_session_new.argtypes = [ctypes.c_size_t, ctypes.c_size_t]
    lib.dc_session_free.argtypes = [ctypes.c_void_p]
    lib.dc_session_shards.restype = ctypes.c_size_t
    lib.dc_session_shards.argtypes = [ctypes.c_void_p]
    lib.dc_session_add.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_size_t, ctypes.c_uint32, ctypes.c_size_t]
    lib.dc_shard_info.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.dc_shard_copy.argtypes = [ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 8
    lib.dc_shard_msg.restype = ctypes.c_void_p
    lib.dc_shard_msg.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p]
    lib.dc_store_group.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_uint32] * 2 + [ctypes.c_void_p] * 3 + [ctypes.c_uint32] + \
        [ctypes.c_void_p] * 2 + [ctypes.c_uint32] * 2 + [ctypes.c_void_p] * 6
    lib.dc_select_matching.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_uint32] + [ctypes.c_void_p] * 2 + [ctypes.c_uint32] * 3 + \
        [ctypes.c_void_p] * 3
    return lib


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


# ---------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------
class PyGroup:
    """The rule of include/hipbls.h restated: one group's records and what an add does to them."""

    def __init__(self, t, max_stored):
        self.t, self.max_stored, self.rec, self.fired = t, max_stored, [], False

    def add(self, partials):
        """[(status, message, share index, serial)] -> (stored flags, slots, full, members or None)"""
        stored, slots, full, members = [], [], 0, None
        for st, m, x, ser in partials:
            stored.append(0)
            slots.append(NONE)
            if st != 0 or self.fired or any(r[0] == x for r in self.rec):
                continue
            if len(self.rec) == self.max_stored:
                full += 1
                continue
            stored[-1], slots[-1] = 1, len(self.rec)
            self.rec.append((x, m, ser))
            same = [(k, r) for k, r in enumerate(self.rec) if r[1] == m]
            if len(same) >= self.t:
                self.fired = True
                members = [(k, r[2], r[0]) for k, r in same[:self.t]]
        return stored, slots, full, members


class CGroup:
    def __init__(self, H, t, max_stored):
        self.H, self.t, self.max_stored = H, t, max_stored
        self.idx = np.full(max_stored + 1, -77, np.int64)  # one sentinel entry behind each record array
        self.msg = np.full(max_stored + 1, 0xA5A5A5A5, np.uint32)
        self.ser = np.full(max_stored + 1, 0xA5A5A5A5, np.uint32)
        self.count, self.fired = np.zeros(1, np.uint32), np.zeros(1, np.uint8)

    def add(self, partials, pad, rng):
        """The partials as items of a larger add: pad other items around them, positions shuffled."""
        k, n = len(partials), len(partials) + pad
        pos = np.sort(rng.choice(n, size=k, replace=False)).astype(np.uint32) if k else np.zeros(0, np.uint32)
        vst, midx, ser = np.full(n, 3, np.uint8), np.full(n, 99, np.uint32), np.full(n, 0xEEEEEEEE, np.uint32)
        for (st, m, x, s), q in zip(partials, pos):
            vst[q], midx[q], ser[q] = st, m, s
        # the group's partials sit at [b, e) of a longer CSR
        b = int(rng.integers(0, 3))
        cpos = np.concatenate([np.full(b, n + 5, np.uint32), pos, np.full(2, 0, np.uint32)])
        cidx = np.concatenate([np.zeros(b, np.int64), np.asarray([p[2] for p in partials], np.int64), np.zeros(2, np.int64)])
        stored, slot = np.full(n, 0x5A, np.uint8), np.full(n, 0x5A5A5A5A, np.uint32)
        mslot, mser, mi = np.full(self.t, NONE, np.uint32), np.full(self.t, NONE, np.uint32), np.full(self.t, -1, np.int64)
        res = np.zeros(5, np.uint32)
        self.H.dc_store_group(_p(self.idx), _p(self.msg), _p(self.ser), _p(self.count), _p(self.fired), self.max_stored, self.t,
                              _p(vst), _p(midx), _p(ser), n, _p(cpos), _p(cidx), b, b + k, _p(stored), _p(slot), _p(mslot),
                              _p(mser), _p(mi), _p(res))
        others = np.setdiff1d(np.arange(n), pos)
        assert (stored[others] == 0x5A).all() and (slot[others] == 0x5A5A5A5A).all(), "items of other groups are not touched"
        assert self.idx[-1] == -77 and self.msg[-1] == 0xA5A5A5A5 and self.ser[-1] == 0xA5A5A5A5
        members = [(int(mslot[j]), int(mser[j]), int(mi[j])) for j in range(self.t)] if res[2] else None
        return [int(x) for x in stored[pos]], [int(x) for x in slot[pos]], int(res[1]), members, int(res[0]), int(res[3])


def random_stream(rng):
    t = int(rng.integers(1, 17))
    max_stored = int(rng.choice([1, 2, t, t + 1, 2 * t, 64, int(rng.integers(1, 65))]))
    max_stored = max(1, min(64, max_stored))
    n_msgs = int(rng.integers(1, 4))
    n_share = int(rng.integers(max(1, t - 2), t + 6))
    length = int(rng.integers(0, 3 * t + 8))
    parts = []
    for k in range(length):
        st = 0 if rng.random() < 0.8 else int(rng.choice([1, 2, 3]))
        m = int(rng.integers(0, n_msgs)) if rng.random() < 0.5 else 0
        x = int(rng.integers(0, n_share + 1)) if rng.random() < 0.9 else int(rng.choice([-1, 1 << 40]))
        parts.append((st, 10 + m, x, 1000 + k))
    n_cuts = int(rng.integers(0, min(length, 6) + 1))
    cuts = sorted(rng.integers(0, length + 1, size=n_cuts).tolist())  # repeated points: empty adds
    return t, max_stored, parts, [0] + cuts + [length]


def test_rule_against_restatement_and_one_shot(H):
    rng = np.random.default_rng(20260117)
    n_fired = n_full = n_multi = 0
    for _ in range(3000):
        t, max_stored, parts, bounds = random_stream(rng)
        py, c = PyGroup(t, max_stored), CGroup(H, t, max_stored)
        fired_add, members = None, None
        all_stored = []
        for a in range(len(bounds) - 1):
            chunk = parts[bounds[a]:bounds[a + 1]]
            ws, wslot, wfull, wmem = py.add(chunk)
            gs, gslot, gfull, gmem, gn, gmsg = c.add(chunk, int(rng.integers(0, 4)), rng)
            assert (gs, gslot, gfull, gmem) == (ws, wslot, wfull, wmem)
            assert gn == sum(ws)
            all_stored += gs
            if gmem is not None:
                assert fired_add is None, "a group fires once"
                fired_add, members = a, gmem
                assert gmsg == py.rec[gmem[0][0]][1]
            # every record
            assert int(c.count[0]) == len(py.rec) and bool(c.fired[0]) == py.fired
            for k, (x, m, ser) in enumerate(py.rec):
                assert (int(c.idx[k]), int(c.msg[k]), int(c.ser[k])) == (x, m, ser)
            n_full += wfull
        n_fired += fired_add is not None
        n_multi += len({p[1] for p in parts}) > 1
        # the defining property: ta_select_matching over the concatenation
        if max_stored < len(parts):
            continue  # the one-shot rule has no limit: compared only where the limit cannot bind
        n = len(parts)
        vst = np.asarray([p[0] for p in parts] + [0], np.uint8)
        midx = np.asarray([p[1] for p in parts] + [0], np.uint32)
        src = np.arange(n + 1, dtype=np.uint32)
        idx = np.asarray([p[2] for p in parts] + [0], np.int64)
        chosen, cidx, res = np.zeros(t, np.uint32), np.zeros(t, np.int64), np.zeros(3, np.uint32)
        H.dc_select_matching(_p(vst), _p(midx), n, _p(src), _p(idx), 0, n, t, _p(chosen), _p(cidx), _p(res))
        assert (res[2] == 0) == (fired_add is not None)
        if fired_add is not None:
            assert [1000 + int(p) for p in chosen] == [m[1] for m in members]
            assert [int(x) for x in cidx] == [m[2] for m in members]
            last = int(chosen[t - 1])
            assert bounds[fired_add] <= last < bounds[fired_add + 1], "fires in the add that holds its t-th member"
        elif len({p[1] for p in parts}) <= 1:
            assert int(res[0]) == len(py.rec), "stored count of a group over one message"
    assert n_fired > 500 and n_full > 100 and n_multi > 500


# ---------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------
def shard_plan(H, s, k):
    info = np.zeros(9, np.uint64)
    H.dc_shard_info(s, k, _p(info))
    gb, ge, m, nvg, before, after, resident, nt, npos = (int(x) for x in info)
    a = dict(order=np.zeros(m, np.uint32), midx=np.zeros(m, np.uint32), serial=np.zeros(m, np.uint32),
             vgoff=np.zeros(nvg + 1, np.uint32), tgroup=np.zeros(nt, np.uint32), toff=np.zeros(nt + 1, np.uint32),
             tpos=np.zeros(npos, np.uint32), tidx=np.zeros(npos, np.int64))
    H.dc_shard_copy(s, k, *(_p(a[x]) for x in ("order", "midx", "serial", "vgoff", "tgroup", "toff", "tpos", "tidx")))
    a.update(gb=gb, ge=ge, m=m, before=before, after=after, resident=resident)
    return a


def shard_msg(H, s, k, mid):
    ln = ctypes.c_uint32(0)
    ptr = H.dc_shard_msg(s, k, mid, ctypes.byref(ln))
    return ctypes.string_at(ptr, ln.value)


@pytest.mark.parametrize("nd", [1, 2, 3])
def test_plan(H, nd):
    rng = np.random.default_rng(7 + nd)
    G, gmax = 11, 3
    pool = [bytes(rng.integers(0, 256, size=int(ln), dtype=np.uint8)) for ln in (32, 32, 32, 32, 5, 0, 32)]
    s = H.dc_session_new(G, nd)
    try:
        assert H.dc_session_shards(s) == nd
        ids = [dict() for _ in range(nd)]  # per shard: message bytes -> id, as first seen
        serial = 0
        sizes = [9, 0, 40, 1, 6, 25]
        for a, n in enumerate(sizes):
            msgs = [pool[int(rng.integers(0, min(len(pool), 2 + a)))] for _ in range(n)]
            blob = np.frombuffer(b"".join(msgs) + b"\0", np.uint8).copy()
            ln = np.asarray([len(m) for m in msgs] + [0], np.uint32)
            off = np.concatenate([[0], np.cumsum(ln[:-1])]).astype(np.uint64)
            group = rng.integers(0, G, size=n + 1).astype(np.uint32)
            if a == 4:
                group[:] = NONE  # only verify-only items
            else:
                group[rng.random(n + 1) < 0.2] = rng.choice([G, G + 7, NONE])
            sidx = rng.integers(-2, 9, size=n + 1).astype(np.int64)
            H.dc_session_add(s, _p(blob), _p(off), _p(ln), _p(group), _p(sidx), n, serial, gmax)
            seen = np.zeros(n, np.int64)
            for k in range(nd):
                p = shard_plan(H, s, k)
                assert (p["gb"], p["ge"]) == (G * k // nd, G * (k + 1) // nd)
                # routing: a group's owner, a verify-only item by position
                for i in p["order"]:
                    g = int(group[i])
                    assert p["gb"] <= g < p["ge"] if g < G else int(i) * nd // n == k
                    seen[i] += 1
                assert len(set(p["order"].tolist())) == p["m"]
                assert np.array_equal(p["serial"], serial + p["order"])
                # message ids: stable across adds, new once, in order of first appearance in arrival order
                assert p["before"] == len(ids[k])
                new = 0
                for i in sorted(p["order"].tolist()):
                    if msgs[i] not in ids[k]:
                        ids[k][msgs[i]] = len(ids[k])
                        new += 1
                assert p["after"] == len(ids[k]) and p["resident"] == p["m"] - new
                for q, i in enumerate(p["order"]):
                    assert p["midx"][q] == ids[k][msgs[i]] and shard_msg(H, s, k, int(p["midx"][q])) == msgs[i]
                # verification order: by message id, stable, groups of at most gmax over one message
                key = [(int(p["midx"][q]), int(p["order"][q])) for q in range(p["m"])]
                assert key == sorted(key)
                vg = p["vgoff"]
                assert vg[0] == 0 and vg[-1] == p["m"] and (np.diff(vg.astype(np.int64)) > 0).all()
                for b, e in zip(vg[:-1], vg[1:]):
                    assert e - b <= gmax and len(set(p["midx"][b:e].tolist())) == 1
                starts = set(vg.tolist())
                for q in range(1, p["m"]):  # a group ends only where it must
                    if q in starts and p["midx"][q] == p["midx"][q - 1]:
                        assert q - max(x for x in starts if x < q) == gmax
                # the CSR: touched groups ascending, each group's partials in arrival order
                tg = p["tgroup"].astype(np.int64) + p["gb"]
                assert (np.diff(tg) > 0).all() and p["toff"][0] == 0 and p["toff"][-1] == len(p["tpos"])
                want = {}
                for i in sorted(p["order"].tolist()):
                    if group[i] < G:
                        want.setdefault(int(group[i]), []).append(i)
                assert sorted(want) == tg.tolist()
                for u, g in enumerate(tg.tolist()):
                    b, e = int(p["toff"][u]), int(p["toff"][u + 1])
                    assert p["order"][p["tpos"][b:e]].tolist() == want[g]
                    assert p["tidx"][b:e].tolist() == sidx[want[g]].tolist()
                if a == 4:
                    assert len(tg) == 0 and (n == 0 or p["m"] > 0 or nd > 1)
                if n == 0:
                    assert p["m"] == 0 and len(p["vgoff"]) == 1
            assert (seen == 1).all(), "every partial is an item of exactly one shard"
            serial += n
    finally:
        H.dc_session_free(s)
