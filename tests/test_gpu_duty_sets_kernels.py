"""The kernels of set-atomic duty adds on the GPU, one launcher at a time, through the device harness
tests/native/dutysetdev.hip (which compiles the product's charon_amd/csrc/duty.hip): k_duty_set_first
and k_duty_gate on explicit words against Python, exactly, and k_duty_store behind the gate against
the rule of include/hipbls.h restated.  Every output array carries sentinel entries behind it.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
REJECTED = 0xFF
PAD = 8
S8, S32 = 0xA5, 0xA5A5A5A5


@pytest.fixture(scope="module")
def D(hipbls):
    from gpu_helpers import harness
    lib = harness.load("dutysetdev")
    I, V = ctypes.c_int, ctypes.c_void_p
    lib.dsd_set_first.argtypes = [I, V, V, V, I, I, V]
    lib.dsd_gate.argtypes = [I, V, V, V, I, I, V]
    lib.dsd_store.argtypes = [I, V, V, V, I, V, V, I, I, V, V, V, V, I, I, I, V, V, V, V, V, I, V, V, V, V, V, V, V]
    return lib


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def u8(x):
    return np.ascontiguousarray(x, dtype=np.uint8)


def u32(x):
    return np.ascontiguousarray(x, dtype=np.uint32)


# ---------------------------------------------------------------------------------------------
# k_duty_set_first / k_duty_gate
# ---------------------------------------------------------------------------------------------
def model_set_first(vst, sid, arr, n_sets):
    sf = [NONE] * n_sets
    for q in range(len(vst)):
        if vst[q] != 0 and sid[q] < n_sets:
            sf[sid[q]] = min(sf[sid[q]], int(arr[q]))
    return sf


def model_gate(vst, sid, sf):
    return [int(v) if v else (REJECTED if sid[q] >= len(sf) or sf[sid[q]] != NONE else 0) for q, v in enumerate(vst)]


def run_set_first(D, vst, sid, arr, n_sets):
    vst, sid, arr = u8(vst), u32(sid), u32(arr)
    sf = np.concatenate([np.full(n_sets, NONE, np.uint32), np.full(PAD, S32, np.uint32)])
    assert D.dsd_set_first(len(vst), _p(vst), _p(sid), _p(arr), n_sets, PAD, _p(sf)) == 0
    assert (sf[n_sets:] == S32).all(), "sentinel behind set_first"
    return sf[:n_sets].tolist()


def run_gate(D, vst, sid, sf):
    vst, sid, n_sets = u8(vst), u32(sid), len(sf)
    sfa = u32(sf if n_sets else [S32])
    adm = np.concatenate([np.full(len(vst), 0x5A, np.uint8), np.full(PAD, S8, np.uint8)])
    assert D.dsd_gate(len(vst), _p(vst), _p(sid), _p(sfa), n_sets, PAD, _p(adm)) == 0
    assert (adm[len(vst):] == S8).all(), "sentinel behind admit"
    return adm[:len(vst)].tolist()


def check_both(D, vst, sid, arr, n_sets, what):
    want = model_set_first(vst, sid, arr, n_sets)
    got = run_set_first(D, vst, sid, arr, n_sets)
    assert got == want, what
    assert run_gate(D, vst, sid, got) == model_gate(vst, sid, want), what
    return got


def runs(off, n):
    """contiguous sets over item positions: set k is positions off[k] .. off[k + 1] - 1"""
    assert off[0] == 0 and off[-1] == n
    return np.repeat(np.arange(len(off) - 1), np.diff(off)).astype(np.uint32)


SIZES = [1, 63, 64, 65, 130]


@pytest.mark.parametrize("n", SIZES)
def test_no_failure_and_every_item_failing(D, n):
    # boundaries at 0, mid-wave and (where n reaches it) exactly on a wave edge; empty sets first, in the middle, last
    off = sorted({0, min(10, n), min(64, n), n})
    off = [0] + off[:2] + [off[1]] + off[2:] + [n]  # an empty set first, one in the middle, one last
    sid, arr = runs(off, n), np.arange(n) + 0
    n_sets = len(off) - 1
    assert check_both(D, np.zeros(n), sid, arr, n_sets, "clean") == [NONE] * n_sets
    got = check_both(D, np.full(n, 3), sid, arr, n_sets, "all failing")
    assert got == [off[k] if off[k + 1] > off[k] else NONE for k in range(n_sets)]
    # arrival order against the lanes: the smallest arrival index is each set's last lane
    got = check_both(D, np.full(n, 1), sid, (n - 1 - np.arange(n)), n_sets, "all failing, reversed arrival")
    assert got == [n - off[k + 1] if off[k + 1] > off[k] else NONE for k in range(n_sets)]


@pytest.mark.parametrize("n", SIZES)
def test_failing_item_first_and_last_of_its_set(D, n):
    cuts = sorted({0, n // 3, min(64, n), n})
    sid, n_sets = runs(cuts, n), len(cuts) - 1
    for which in ("first", "last"):
        vst = np.zeros(n, np.uint8)
        for k in range(n_sets):
            vst[cuts[k] if which == "first" else cuts[k + 1] - 1] = 2 + k
        got = check_both(D, vst, sid, np.arange(n) + 1000, n_sets, which)
        assert got == [1000 + (cuts[k] if which == "first" else cuts[k + 1] - 1) for k in range(n_sets)]


def test_two_failures_of_one_set(D):
    n = 130
    sid = runs([0, 5, 129, 130], n)  # set 1 spans the wave edges at 64 and 128
    for a, b in ((20, 90), (20, 40), (63, 64), (70, 124), (64, 127), (5, 128)):  # different waves; the same wave
        for arr in (np.arange(n), n - 1 - np.arange(n), np.random.default_rng(a * b).permutation(n)):
            vst = np.zeros(n, np.uint8)
            vst[[a, b]] = [1, 4]
            got = check_both(D, vst, sid, arr, 3, (a, b))
            assert got == [NONE, int(min(arr[a], arr[b])), NONE], "the smaller arrival index wins"


def test_64_singleton_sets_in_one_wave_all_failing(D):
    for n in (64, 130):
        sid, arr = np.arange(n), np.random.default_rng(n).permutation(n) + 7
        got = check_both(D, np.full(n, 5), sid, arr, n, n)
        assert got == arr.tolist()


@pytest.mark.parametrize("n", SIZES)
def test_shuffled_sets(D, n):
    """set ids as a shard's verification order leaves them: any set in any lane"""
    rng = np.random.default_rng(n)
    for n_sets in (1, 2, 7, 64, 200):
        for fail in (0.02, 0.3, 0.9):
            sid = rng.integers(0, n_sets, size=n)
            vst = np.where(rng.random(n) < fail, rng.integers(1, 7, size=n), 0)
            check_both(D, vst, sid, rng.permutation(n) + 3, n_sets, (n_sets, fail))


# ---------------------------------------------------------------------------------------------
# k_duty_store behind the gate
# ---------------------------------------------------------------------------------------------
class Shard:
    """The records of n_groups groups, as the device holds them, with sentinels behind each array."""

    def __init__(self, n_groups, max_stored, t):
        self.G, self.ms, self.t = n_groups, max_stored, t
        s = n_groups * max_stored
        self.idx = np.concatenate([np.zeros(s, np.int64), np.full(PAD, -77, np.int64)])
        self.msg = np.concatenate([np.zeros(s, np.uint32), np.full(PAD, S32, np.uint32)])
        self.ser = np.concatenate([np.zeros(s, np.uint32), np.full(PAD, S32, np.uint32)])
        self.count = np.concatenate([np.zeros(n_groups, np.uint32), np.full(PAD, S32, np.uint32)])
        self.fired = np.concatenate([np.zeros(n_groups, np.uint8), np.full(PAD, S8, np.uint8)])

    def records(self, g):
        c, r0 = int(self.count[g]), g * self.ms
        return [(int(self.idx[r0 + k]), int(self.msg[r0 + k]), int(self.ser[r0 + k])) for k in range(c)]

    def put(self, g, recs, fired=False):
        r0 = g * self.ms
        for k, (x, m, s) in enumerate(recs):
            self.idx[r0 + k], self.msg[r0 + k], self.ser[r0 + k] = x, m, s
        self.count[g], self.fired[g] = len(recs), int(fired)


def model_store(sh, seen, midx, serial, tgroup, toff, tpos, tidx):
    """The rule over the touched groups, given what the gate lets the store see -> the groups' new
    records, stored, slot, fired rows (touched index -> members' serials), copies, full"""
    n = len(seen)
    stored, slot, fired, copies, full = [0] * n, [S32] * n, {}, [], 0
    new = {}
    for u, g in enumerate(tgroup):
        rec, closed = sh.records(g), bool(sh.fired[g])
        for j in range(toff[u], toff[u + 1]):
            q = int(tpos[j])
            stored[q], slot[q] = 0, NONE
            if closed or seen[q] != 0 or any(r[0] == tidx[j] for r in rec):
                continue
            if len(rec) == sh.ms:
                full += 1
                continue
            stored[q], slot[q] = 1, len(rec)
            copies.append((g * sh.ms + len(rec), q))
            rec.append((int(tidx[j]), int(midx[q]), int(serial[q])))
            same = [r for r in rec if r[1] == midx[q]]
            if len(same) >= sh.t:
                closed = True
                fired[u] = [r[2] for r in same[:sh.t]]
        new[g] = (rec, closed)
    return new, stored, slot, fired, copies, full


def run_store(D, sh, vst, sid, sf, midx, serial, tgroup, toff, tpos, tidx):
    n, nt, np_ = len(vst), len(tgroup), len(tpos)
    want_seen = model_gate(vst, sid, sf)
    want = model_store(sh, want_seen, midx, serial, tgroup, toff, tpos, tidx)
    untouched = {g: (sh.records(g), bool(sh.fired[g])) for g in range(sh.G) if g not in tgroup}
    o = dict(admit=np.concatenate([np.full(n, 0x5A, np.uint8), np.full(PAD, S8, np.uint8)]),
             stored=np.concatenate([np.zeros(n, np.uint8), np.full(PAD, S8, np.uint8)]),
             slot=np.full(n + PAD, S32, np.uint32), mserial=np.full(nt * sh.t + PAD, S32, np.uint32),
             copies=np.full(2 * (n + PAD), S32, np.uint32), fired_u=np.full(nt + PAD, S32, np.uint32),
             ctr=np.concatenate([np.zeros(4, np.uint32), np.full(PAD, S32, np.uint32)]))
    a = [u8(vst), u32(sid), u32(sf if len(sf) else [S32]), u32(midx), u32(serial), u32(tgroup), u32(toff), u32(tpos),
         np.ascontiguousarray(tidx, dtype=np.int64)]
    rc = D.dsd_store(n, _p(a[0]), _p(a[1]), _p(a[2]), len(sf), _p(a[3]), _p(a[4]), nt, np_, _p(a[5]), _p(a[6]), _p(a[7]), _p(a[8]),
                     sh.G, sh.ms, sh.t, _p(sh.idx), _p(sh.msg), _p(sh.ser), _p(sh.count), _p(sh.fired), PAD, _p(o["admit"]),
                     _p(o["stored"]), _p(o["slot"]), _p(o["mserial"]), _p(o["copies"]), _p(o["fired_u"]), _p(o["ctr"]))
    assert rc == 0
    new, stored, slot, fired, copies, full = want
    # sentinels: behind every array, and in every entry the kernels have no business writing
    assert sh.idx[-PAD:].tolist() == [-77] * PAD and (sh.msg[-PAD:] == S32).all() and (sh.ser[-PAD:] == S32).all()
    assert (sh.count[-PAD:] == S32).all() and (sh.fired[-PAD:] == S8).all()
    assert (o["admit"][n:] == S8).all() and (o["stored"][n:] == S8).all() and (o["slot"][n:] == S32).all()
    assert (o["ctr"][4:] == S32).all() and (o["fired_u"][len(fired):] == S32).all()
    assert (o["copies"][2 * len(copies):] == S32).all(), "no copy entry beyond the stored partials"
    assert o["admit"][:n].tolist() == want_seen
    assert o["stored"][:n].tolist() == stored
    walked = sorted(int(q) for u in range(nt) for q in tpos[toff[u]:toff[u + 1]])
    assert [int(o["slot"][q]) for q in walked] == [slot[q] for q in walked]
    assert all(o["slot"][q] == S32 for q in range(n) if q not in walked), "an item of no touched group is not walked"
    for g, (rec, closed) in {**new, **untouched}.items():
        assert sh.records(g) == rec and bool(sh.fired[g]) == closed, g
    assert o["ctr"][:4].tolist() == [len(copies), len(fired), full, 0], "DUTY_CTR_COPIES / _FIRED / _FULL"
    got_copies = o["copies"][:2 * len(copies)].reshape(-1, 2)
    got_fired = o["fired_u"][:len(fired)].tolist()
    if nt <= 64:  # one wave: the lists are in lane order
        assert [tuple(x) for x in got_copies.tolist()] == copies
        assert got_fired == sorted(fired)
    else:  # the waves' segments come in any order
        assert sorted(tuple(x) for x in got_copies.tolist()) == sorted(copies)
        assert sorted(got_fired) == sorted(fired)
    for u, members in fired.items():
        assert o["mserial"][u * sh.t:(u + 1) * sh.t].tolist() == members
    assert (o["mserial"][nt * sh.t:] == S32).all()
    return o, want


def test_group_whose_only_partial_is_in_a_rejected_set(D):
    sh = Shard(3, 4, 2)
    sh.put(1, [(1, 7, 100)])  # one stored partial: the new one (share 2, same message) would fire the group
    # items: 0 fails (set 0), 1 verifies (set 0: rejected with it), 2 verifies (set 1)
    vst, sid, sf = [3, 0, 0], [0, 0, 1], [0, NONE]
    o, want = run_store(D, sh, vst, sid, sf, midx=[7, 7, 7], serial=[200, 201, 202], tgroup=[1], toff=[0, 1], tpos=[1],
                        tidx=[2])
    assert o["admit"][:3].tolist() == [3, REJECTED, 0]
    assert o["stored"][:3].tolist() == [0, 0, 0] and sh.count[1] == 1 and sh.fired[1] == 0
    assert o["ctr"][:3].tolist() == [0, 0, 0], "no copy entry, nothing fired"


def test_group_with_one_partial_rejected_and_one_admitted(D):
    sh = Shard(2, 4, 2)
    sh.put(0, [(1, 7, 100)])
    # group 0 gets share 2 through rejected set 0 (item 1) and share 3 through admitted set 1 (item 2): it fires through
    # the later set, with members (1, 3)
    vst, sid, sf = [5, 0, 0, 0], [0, 0, 1, 1], [0, NONE]
    o, want = run_store(D, sh, vst, sid, sf, midx=[7, 7, 7, 9], serial=[300, 301, 302, 303], tgroup=[0, 1], toff=[0, 2, 3],
                        tpos=[1, 2, 3], tidx=[2, 3, 1])
    assert o["stored"][:4].tolist() == [0, 0, 1, 1]
    assert sh.records(0) == [(1, 7, 100), (3, 7, 302)] and sh.fired[0] == 1
    assert o["mserial"][:2].tolist() == [100, 302]
    assert o["ctr"][:3].tolist() == [2, 1, 0]


@pytest.mark.parametrize("nt_max", [5, 64, 70])
def test_store_counters_against_the_restated_rule(D, nt_max):
    rng = np.random.default_rng(nt_max)
    for rnd in range(6):
        G, t, ms = nt_max + 3, int(rng.integers(1, 5)), int(rng.integers(1, 6))
        sh = Shard(G, ms, t)
        for g in range(G):  # resident records: distinct share indices, below the threshold per message
            k = int(rng.integers(0, ms + 1))
            recs = [(int(x), 50 + j, 10 + j) for j, x in enumerate(rng.permutation(8)[:k] + 1)]
            sh.put(g, recs[:k], fired=bool(rng.random() < 0.1))
            if t == 1 and k:
                sh.put(g, recs[:k], fired=True)
        n = int(rng.integers(nt_max, 3 * nt_max + 2))
        n_sets = int(rng.integers(1, 9))
        sid = rng.integers(0, n_sets, size=n)
        vst = np.where(rng.random(n) < 0.1, rng.integers(1, 7, size=n), 0)
        sf = model_set_first(vst, sid, rng.permutation(n), n_sets)
        groups = np.where(rng.random(n) < 0.1, NONE, rng.integers(0, G, size=n))
        tgroup = sorted(int(g) for g in set(groups.tolist()) if g != NONE)[:nt_max]
        tpos, toff = [], [0]
        for g in tgroup:
            tpos += np.flatnonzero(groups == g).tolist()
            toff.append(len(tpos))
        tidx = rng.integers(1, 9, size=len(tpos))
        midx, serial = rng.integers(50, 52, size=n), 1000 + np.arange(n)
        run_store(D, sh, vst, sid, sf, midx, serial, tgroup, toff, tpos, tidx)
