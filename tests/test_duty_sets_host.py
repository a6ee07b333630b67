"""The host side of set-atomic duty adds (hbls_duty_add_sets) on the CPU, through the g++ harness
tests/native/dutysetcheck.cpp: the validation of set_off, the plan's set ids and arrival indices and
the shards' min-merge (charon_amd/csrc/hduty.h), the admission predicate (charon_amd/csrc/dutysel.h
duty_admit, what duty.hip's k_duty_gate runs per lane), and the defining property: over seeded
streams, (set verdict -> duty_store_group) equals a Python restatement of include/hipbls.h and
equals hbls_duty_add's rule on a twin whose partials of rejected sets have no group.
"""
import copy
import ctypes

import numpy as np
import pytest

NONE = 0xFFFFFFFF
REJECTED = 0xFF


@pytest.fixture(scope="module")
def H():
    from gpu_helpers import harness
    lib = harness.load("dutysetcheck")
    V, SZ, U32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    lib.ds_check_sets.restype = ctypes.c_char_p
    lib.ds_check_sets.argtypes = [V, SZ, SZ]
    lib.ds_admit.restype = ctypes.c_uint8
    lib.ds_admit.argtypes = [ctypes.c_uint8, U32, V, U32]
    lib.ds_merge.argtypes = [V, V, SZ]
    lib.ds_new.restype = V
    lib.ds_new.argtypes = [SZ, SZ, U32, U32]
    lib.ds_free.argtypes = [V]
    lib.ds_shards.restype = SZ
    lib.ds_shards.argtypes = [V]
    lib.ds_next_serial.restype = U32
    lib.ds_next_serial.argtypes = [V]
    lib.ds_add.argtypes = [V] * 5 + [SZ, V, SZ, ctypes.c_int] + [V] * 5
    lib.ds_state.argtypes = [V] * 3
    lib.ds_shard_m.restype = SZ
    lib.ds_shard_m.argtypes = [V, SZ]
    lib.ds_shard_plan.argtypes = [V, SZ, V, V, V]
    return lib


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


class CDuty:
    """One duty in the harness: hduty.h's plan, dutysel.h's predicate and rule, over given verdicts."""

    def __init__(self, H, G, nd, t, max_stored):
        self.H, self.G, self.t = H, G, t
        self.h = H.ds_new(G, nd, t, max_stored)
        self.nd = H.ds_shards(self.h)

    def close(self):
        self.H.ds_free(self.h)

    def add(self, c, sets=True, group=None):
        n, n_sets = len(c["vst"]), len(c["set_off"]) - 1
        grp = c["group"] if group is None else group
        stored, sf = np.full(n + 1, 0x5A, np.uint8), np.full(n_sets + 1, 0x5A5A5A5A, np.uint32)
        fired, chosen = np.full(n + 1, 0x5A5A5A5A, np.uint32), np.full(n * self.t + 1, 0x5A5A5A5A, np.uint32)
        res = np.zeros(3, np.uint32)
        rc = self.H.ds_add(self.h, _p(c["msg"]), _p(grp), _p(c["idx"]), _p(c["vst"]), n, _p(c["set_off"]), n_sets, int(sets),
                           _p(stored), _p(sf), _p(fired), _p(chosen), _p(res))
        if rc:
            return None
        f = int(res[0])
        assert stored[n] == 0x5A and fired[f] == 0x5A5A5A5A and chosen[f * self.t] == 0x5A5A5A5A, "sentinels"
        assert sf[n_sets] == 0x5A5A5A5A and (not sets or n_sets == 0 or (sf[:n_sets] != 0x5A5A5A5A).all())
        return dict(stored=stored[:n].tolist(), set_first=sf[:n_sets].tolist() if sets else None,
                    fired=[(int(fired[k]), chosen[k * self.t:(k + 1) * self.t].tolist()) for k in range(f)],
                    full=int(res[1]), first=int(res[2]))

    def state(self):
        cnt, fl = np.zeros(max(self.G, 1), np.uint32), np.zeros(max(self.G, 1), np.uint8)
        self.H.ds_state(self.h, _p(cnt), _p(fl))
        return cnt[:self.G].tolist(), fl[:self.G].tolist()

    def shard(self, k, n_sets):
        m = self.H.ds_shard_m(self.h, k)
        order, sid, sf = np.zeros(m + 1, np.uint32), np.zeros(m + 1, np.uint32), np.zeros(n_sets + 1, np.uint32)
        self.H.ds_shard_plan(self.h, k, _p(order), _p(sid), _p(sf))
        return order[:m].tolist(), sid[:m].tolist(), sf[:n_sets].tolist()


# ---------------------------------------------------------------------------------------------
# include/hipbls.h restated
# ---------------------------------------------------------------------------------------------
def set_verdicts(c):
    off, vst = c["set_off"], c["vst"]
    out = []
    for k in range(len(off) - 1):
        bad = [i for i in range(int(off[k]), int(off[k + 1])) if vst[i] != 0]
        out.append(bad[0] if bad else NONE)
    return out


class PyDuty:
    def __init__(self, G, t, max_stored):
        self.G, self.t, self.max_stored = G, t, max_stored
        self.rec = [[] for _ in range(G)]  # (share index, message, serial) in stored order
        self.fired = [False] * G
        self.next_serial = 0

    def add(self, c, sets=True):
        """-> stored, set_first, fired [(group, members' serials)] ascending, full, first serial, and
        per fired group the call index of its last member"""
        n = len(c["vst"])
        sf = set_verdicts(c) if sets else [NONE] * (len(c["set_off"]) - 1)
        set_of = np.repeat(np.arange(len(sf)), np.diff(c["set_off"].astype(np.int64))) if len(sf) else []
        stored, full, fired, last = [0] * n, 0, {}, {}
        for i in range(n):
            g = int(c["group"][i])
            if c["vst"][i] != 0 or g >= self.G or (sets and sf[set_of[i]] != NONE):
                continue
            if self.fired[g] or any(r[0] == c["idx"][i] for r in self.rec[g]):
                continue
            if len(self.rec[g]) == self.max_stored:
                full += 1
                continue
            stored[i] = 1
            self.rec[g].append((int(c["idx"][i]), int(c["msg"][i]), self.next_serial + i))
            same = [r for r in self.rec[g] if r[1] == c["msg"][i]]
            if len(same) >= self.t:
                self.fired[g] = True
                fired[g] = [r[2] for r in same[:self.t]]
                last[g] = i
        first = self.next_serial
        self.next_serial += n
        return dict(stored=stored, set_first=sf if sets else None, fired=sorted(fired.items()), full=full, first=first), last

    def state(self):
        return [len(r) for r in self.rec], [int(f) for f in self.fired]


# ---------------------------------------------------------------------------------------------
# set_off, the predicate, the merge, the plan
# ---------------------------------------------------------------------------------------------
def test_set_off_validation(H):
    def chk(off, n_sets, n):
        a = None if off is None else np.asarray(off, np.uint32)
        return H.ds_check_sets(_p(a), n_sets, n)

    assert chk([0, 2, 2, 5], 3, 5) is None
    assert chk([0, 0, 0], 2, 0) is None, "empty sets only"
    assert chk([0, 0, 5, 5], 3, 5) is None, "empty sets first and last"
    assert chk(None, 0, 0) is None, "no sets, no partials"
    assert chk([0], 0, 0) is None
    assert b"set_off[0]" in chk([1, 2, 5], 2, 5)
    assert b"decrease" in chk([0, 4, 3, 5], 3, 5)
    assert b"set_off[n_sets]" in chk([0, 2, 4], 2, 5)
    assert b"set_off[n_sets]" in chk([0, 2, 6], 2, 5)
    assert b"n_sets is 0" in chk([0], 0, 3)
    assert b"n_sets is 0" in chk(None, 0, 3)
    assert b"required" in chk(None, 2, 5)


def test_malformed_calls_do_nothing(H):
    d = CDuty(H, 4, 1, 2, 4)
    try:
        c = dict(msg=np.full(5, 7, np.uint32), group=np.asarray([0, 1, 2, 3, 0], np.uint32), idx=np.arange(1, 6, dtype=np.int64),
                 vst=np.zeros(5, np.uint8))
        for off in ([1, 2, 5], [0, 4, 3, 5], [0, 2, 4], [0]):
            assert d.add(dict(c, set_off=np.asarray(off, np.uint32))) is None, off
            assert d.state() == ([0] * 4, [0] * 4) and H.ds_next_serial(d.h) == 0
        assert d.add(dict(c, set_off=np.asarray([0, 2, 5], np.uint32)))["stored"] == [1] * 5
        assert H.ds_next_serial(d.h) == 5
    finally:
        d.close()


def test_admission_predicate(H):
    sf = np.asarray([NONE, 3, NONE, 0], np.uint32)
    for vst in (0, 1, 2, 3, 7, 255):
        for sid in range(4):
            want = vst if vst else (REJECTED if sf[sid] != NONE else 0)
            assert H.ds_admit(vst, sid, _p(sf), 4) == want, (vst, sid)
    # a set id outside the call's sets admits nothing and reads nothing
    for sid in (4, 5, 1 << 20, NONE):
        assert H.ds_admit(0, sid, _p(sf), 4) == REJECTED
        assert H.ds_admit(0, sid, None, 0) == REJECTED
        assert H.ds_admit(5, sid, None, 0) == 5


def test_merge(H):
    a = np.asarray([NONE, 7, 3, NONE, 0], np.uint32)
    b = np.asarray([NONE, 2, 9, 4, NONE], np.uint32)
    m = a.copy()
    H.ds_merge(_p(m), _p(b), 5)
    assert m.tolist() == [NONE, 2, 3, 4, 0]
    H.ds_merge(_p(m), _p(b), 0)
    assert m.tolist() == [NONE, 2, 3, 4, 0]


@pytest.mark.parametrize("nd", [1, 2, 3])
def test_plan_set_ids_and_merge_over_shards(H, nd):
    rng = np.random.default_rng(100 + nd)
    for _ in range(60):
        c = random_call(rng, G=int(rng.integers(1, 30)), t=3, n_roots=3, fail=0.3)
        n, n_sets = len(c["vst"]), len(c["set_off"]) - 1
        d = CDuty(H, c["G"], nd, 3, 8)
        try:
            r = d.add(c)
            assert d.nd == min(nd, c["G"])
            set_of = np.repeat(np.arange(n_sets), np.diff(c["set_off"].astype(np.int64))).tolist()
            seen, merged = [], [NONE] * n_sets
            for k in range(d.nd):
                order, sid, sf = d.shard(k, n_sets)
                assert sid == [set_of[i] for i in order], "each item's set id is its arrival index's set"
                want = [NONE] * n_sets  # the shard's own verdicts: over its items only
                for i in order:
                    if c["vst"][i] != 0:
                        want[set_of[i]] = min(want[set_of[i]], i)
                assert sf == want
                merged = [min(x, y) for x, y in zip(merged, sf)]
                seen += order
            assert sorted(seen) == list(range(n)), "every partial is some shard's item, once"
            assert merged == set_verdicts(c) == r["set_first"], "the merge is the verdict over the whole call"
        finally:
            d.close()


# ---------------------------------------------------------------------------------------------
# the defining property
# ---------------------------------------------------------------------------------------------
def random_call(rng, G, t, n_roots, fail):
    n_sets = int(rng.integers(0, 13))
    sizes = [int(rng.choice([0, 0, 1, 1, 2, 3, 5, 8])) for _ in range(n_sets)]
    n = sum(sizes)
    group = rng.integers(0, G, size=n).astype(np.uint32)
    if n and rng.random() < 0.5:  # few groups: thresholds are reached
        group = rng.integers(0, min(G, 3), size=n).astype(np.uint32)
    group[rng.random(n) < 0.1] = NONE  # verify only
    idx = rng.integers(1, t + 3, size=n).astype(np.int64)
    msg = (1000 + rng.integers(0, n_roots, size=n)).astype(np.uint32)
    vst = np.where(rng.random(n) < fail, rng.integers(1, 7, size=n), 0).astype(np.uint8)
    return dict(G=G, msg=msg, group=group, idx=idx, vst=vst,
                set_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32))


N_STREAMS = 2000


def test_defining_property(H):
    rng = np.random.default_rng(20240607)
    seen = dict(lone_failure=0, held_tth_store=0, fires_later_instead=0, all_rejected=0, none_rejected=0, calls=0)
    for _ in range(N_STREAMS):
        G, t, max_stored = int(rng.integers(1, 41)), int(rng.integers(1, 6)), int(rng.integers(1, 9))
        nd, n_roots, fail = int(rng.integers(1, 4)), int(rng.integers(1, 4)), float(rng.choice([0.0, 0.05, 0.15, 0.3]))
        ds, tw, py = CDuty(H, G, nd, t, max_stored), CDuty(H, G, nd, t, max_stored), PyDuty(G, t, max_stored)
        try:
            for _call in range(int(rng.integers(1, 6))):
                c = random_call(rng, G, t, n_roots, fail)
                n_sets = len(c["set_off"]) - 1
                sf = set_verdicts(c)
                set_of = np.repeat(np.arange(n_sets), np.diff(c["set_off"].astype(np.int64)))
                # what hbls_duty_add's rule would do from the same state (the coverage counts only)
                plain, plain_last = copy.deepcopy(py).add(c, sets=False)
                want, last = py.add(c)
                got = ds.add(c)
                assert got == want, "harness against the restated rule"
                # the twin: hbls_duty_add's rule, no group for the partials of rejected sets
                g2 = c["group"].copy()
                for i in range(len(g2)):
                    if sf[set_of[i]] != NONE:
                        g2[i] = NONE
                twin = tw.add(c, sets=False, group=g2)
                assert twin == dict(got, set_first=None), "harness against the twin rule"
                assert ds.state() == tw.state() == py.state()
                # coverage
                seen["calls"] += 1
                sizes = np.diff(c["set_off"].astype(np.int64))
                rej = [k for k in range(n_sets) if sf[k] != NONE]
                seen["lone_failure"] += sum(1 for k in rej if sizes[k] >= 2 and
                                            (c["vst"][int(c["set_off"][k]):int(c["set_off"][k + 1])] != 0).sum() == 1)
                if n_sets and len(rej) == n_sets:
                    seen["all_rejected"] += 1
                if n_sets and not rej:
                    seen["none_rejected"] += 1
                for g, i in plain_last.items():
                    if sf[set_of[i]] != NONE:
                        seen["held_tth_store"] += 1
                        if g in last and set_of[last[g]] > set_of[i]:
                            seen["fires_later_instead"] += 1
        finally:
            ds.close()
            tw.close()
    # the generator reaches every situation the rule distinguishes, many times over
    assert seen["calls"] >= N_STREAMS
    assert seen["lone_failure"] >= 100, seen
    assert seen["held_tth_store"] >= 100, seen
    assert seen["fires_later_instead"] >= 20, seen
    assert seen["all_rejected"] >= 20, seen
    assert seen["none_rejected"] >= 100, seen
