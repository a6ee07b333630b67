"""The cases of tests/test_gpu_duty_first.py: first-error duty set adds through the ABI
(hbls_duty_add_sets_first / hbls_duty_first_stats), -m gpu: a rejected set is stopped at its first
failure.  Not collected with the suite (the name): that file runs this one once, in a process of its own,
and says why.

Inputs are the clusters and streams of tests/test_gpu_duty.py (256 validators, 5 of 7 and 3 of 4; the
clean streams are peer-major, and consecutive validators sign different messages, so a call's
verification groups are runs of one partial: 7 x 256 = 1 792 groups for a duty in one call, in batches
of 64).  The reference is the defining property of include/hipbls.h: every call is compared with a twin
duty given the same calls through hbls_duty_add_sets -- set_first, stored, first_serial, the fired
rows, the duty's state and statistics exactly, vstatus under the call's contract (tests/gpu_helpers/
duty_first.py run_first_pair).
"""
import ctypes
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

OK, BAD_SIGNATURE, NOT_VERIFIED, UNCHECKED = 0, 2, 3, 7
NONE = 0xFFFFFFFF

from test_gpu_duty import L, clusters, dh, sh, ss, streams  # noqa: E402,F401 -- its fixtures: the same clusters and streams


@pytest.fixture(scope="module")
def df():
    import duty_first
    return duty_first


def whole(s):
    return [0, len(s["pks"])]


STRADDLING = [0, 100, 300, 500, 700, 900, 1100, 1300, 1500, 1700, 1792]  # no boundary on a multiple of 64


# 1
def test_clean_one_set_per_call_and_all_sets_in_one_call(L, df, clusters, streams):
    d = clusters[(7, 5)]
    s, _ = streams["clean", (7, 5)]
    V, n, t = d["V"], d["n"], d["t"]
    r = df.run_first_pair(L, s, [k * V for k in range(n + 1)], [[0, V]] * n)
    assert [len(c["fired"]) for c in r["calls"]] == [0] * (t - 1) + [V] + [0] * (n - t)
    assert np.array_equal(r["calls"][t - 1]["out"], d["root_sigs"].reshape(V, 96))
    assert r["first_stats"] == [n * V, 0] and r["set_stats"] == [n, 0, 0]
    for key, off in (((7, 5), [k * V for k in range(8)]), ((4, 3), [0, 0, 100, 300, 300, 1024, 1024])):
        s, _ = streams["clean", key]
        r = df.run_first_pair(L, s, whole(s), [off])
        c = r["calls"][0]
        assert (c["vst"] == OK).all() and (c["set_first"] == NONE).all() and c["fired"].tolist() == list(range(V))
        assert np.array_equal(c["out"], clusters[key]["root_sigs"].reshape(V, 96))
        assert r["first_stats"] == [len(s["pks"]), 0] and r["set_stats"] == [len(off) - 1, 0, 0]


# 2
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_corrupted_partial(L, df, clusters, streams, where):
    d = clusters[(7, 5)]
    s0, _ = streams["clean", (7, 5)]
    V, n = d["V"], d["n"]
    at = {"first": 2 * V, "middle": 2 * V + 77, "last": 3 * V - 1}[where]
    s = df.spoiled(s0, [at])
    r = df.run_first_pair(L, s, whole(s), [[k * V for k in range(n + 1)]])  # one call: 1 792 groups, batches of 64
    c = r["calls"][0]
    assert c["set_first"].tolist() == [NONE, NONE, at] + [NONE] * 4
    assert c["vst"][at] == NOT_VERIFIED and (np.delete(c["vst"], at) == OK).all(), "the only failure: nothing is left unchecked"
    assert not c["stored"][2 * V:3 * V].any() and c["fired"].tolist() == list(range(V)), "they fire through peer 5's set"
    assert r["set_stats"] == [7, 1, V - 1] and r["first_stats"] == [n * V, 0]
    r = df.run_first_pair(L, s, [k * V for k in range(n + 1)], [[0, V]] * n)  # one set per call: 256 groups
    assert [c["set_first"].tolist() for c in r["calls"]] == [[NONE]] * 2 + [[at - 2 * V]] + [[NONE]] * 4
    assert [len(c["fired"]) for c in r["calls"]] == [0, 0, 0, 0, 0, V, 0]


# 3
def test_sets_cut_across_the_batches(L, df, streams):
    s0, _ = streams["clean", (7, 5)]
    # bad partials: in a set's head batch only (310), in head and later batches (520, 650), first and last of a
    # set (900, 1099), a run across a boundary (1298 .. 1301), in a set of its own batch range (1750)
    bad = [310, 520, 650, 900, 1099, 1298, 1299, 1300, 1301, 1750]
    s = df.spoiled(s0, bad)
    r = df.run_first_pair(L, s, whole(s), [STRADDLING])
    c = r["calls"][0]
    assert c["set_first"].tolist() == [NONE, NONE, 310, 520, NONE, 900, 1298, 1300, NONE, 1750]
    assert (c["vst"][np.asarray([310, 520, 900, 1298, 1300, 1750])] == NOT_VERIFIED).all()
    assert r["set_stats"][:2] == [10, 6]


# 4
def test_head_batch_failing_through_the_previous_set_only(L, df, streams):
    s0, _ = streams["clean", (7, 5)]
    # batch 64 .. 127 straddles sets 0 and 1 and fails through set 0's last partials alone; set 1's only bad
    # partial lies 150 groups into it, in batch 192 .. 255: set 1 must still be rejected, at that partial
    s = df.spoiled(s0, [96, 97, 98, 99, 250])
    r = df.run_first_pair(L, s, whole(s), [STRADDLING])
    c = r["calls"][0]
    assert c["set_first"].tolist() == [96, 250] + [NONE] * 8
    assert c["vst"][96] == NOT_VERIFIED and c["vst"][250] == NOT_VERIFIED
    assert (c["vst"][100:250] == OK).all() and (c["vst"][251:300] == OK).all(), "set 1: exact, its one failure found"
    assert not c["stored"][:300].any() and c["stored"][300:1280].all()
    assert r["set_stats"][:2] == [10, 2]


# 5: the test that shows the mode is not the exact one under another name
def test_a_set_with_bad_partials_in_many_batches_is_left_unchecked_behind_the_first(L, df, clusters, streams):
    d = clusters[(7, 5)]
    s0, _ = streams["clean", (7, 5)]
    V = d["V"]
    bad = [300, 700, 1100, 1500, 1501]
    s = df.spoiled(s0, bad)
    r = df.run_first_pair(L, s, whole(s), [[0, V, 7 * V]])
    c, w = r["calls"][0], r["twin"][0]
    assert c["set_first"].tolist() == [NONE, 300] and (w["vst"][bad] == NOT_VERIFIED).all()
    assert c["vst"][300] == NOT_VERIFIED and (c["vst"][np.asarray(bad[1:])] == UNCHECKED).all()
    assert r["first_stats"][0] == 7 * V and r["first_stats"][1] >= 3 * 64, "the later failing batches are not descended into"
    assert c["stored"][:V].all() and not c["stored"][V:].any() and len(c["fired"]) == 0


# 6
def test_all_undecodable_and_all_wrong(L, df, clusters, streams):
    d = clusters[(4, 3)]
    s0, _ = streams["clean", (4, 3)]
    V = d["V"]
    off = [0, 100, V, 2 * V]
    s = df.undecodable(s0, range(2 * V))
    r = df.run_first_pair(L, s, [0, 2 * V], [off])
    c = r["calls"][0]
    assert (c["vst"] == BAD_SIGNATURE).all() and c["set_first"].tolist() == [0, 100, V] and r["unchecked"] == 0
    s = df.spoiled(s0, range(2 * V))
    r = df.run_first_pair(L, s, [0, 2 * V], [off])
    c = r["calls"][0]
    assert c["set_first"].tolist() == [0, 100, V] and (c["vst"][[0, 100, V]] == NOT_VERIFIED).all()
    assert set(c["vst"].tolist()) == {NOT_VERIFIED, UNCHECKED} and r["unchecked"] > 0
    assert r["set_stats"] == [3, 3, 0] and not r["count"].any()


# 7
def test_slot_wide_check_and_the_adaptive_per_batch_path(L, df, clusters, streams):
    d = clusters[(7, 5)]
    s0, _ = streams["clean", (7, 5)]
    V = d["V"]
    s = df.spoiled(s0, [96, 97, 98, 99, 250, 700, 1100])
    prev = L.hbls_slot_msm(256)
    try:
        # the first call's slot-wide check fails and falls to its batches; the second knows and goes there directly
        res = [df.run_first_pair(L, s, whole(s), [STRADDLING]) for _ in range(2)]
        clean = df.run_first_pair(L, s0, whole(s0), [STRADDLING])
    finally:
        L.hbls_slot_msm(prev)
    for r in res:
        assert r["calls"][0]["set_first"].tolist() == [96, 250, NONE, NONE, 700, NONE, 1100, NONE, NONE, NONE]
    assert (clean["calls"][0]["set_first"] == NONE).all() and clean["first_stats"] == [7 * V, 0]


# 8
def test_chunked_groups(L, df, streams):
    s0, _ = streams["clean", (7, 5)]
    s = df.spoiled(s0, [96, 97, 98, 99, 250, 700, 900, 1100, 1500])
    prev = ctypes.c_size_t(0)
    assert L.hbls_tune(b"HBLS_GROUP_CHUNK", 136, ctypes.byref(prev)) == 0  # 1 792 groups in chunks of 136: batches restart
    try:
        r = df.run_first_pair(L, s, whole(s), [STRADDLING])
        one = df.run_first_pair(L, s, whole(s), [whole(s)])
    finally:
        assert L.hbls_tune(b"HBLS_GROUP_CHUNK", prev.value, None) == 0
    assert r["calls"][0]["set_first"].tolist() == [96, 250, NONE, NONE, 700, 900, 1100, NONE, 1500, NONE]
    assert one["calls"][0]["set_first"].tolist() == [96] and one["unchecked"] > 0


# 9
def test_below_the_batched_final_exponentiation_statuses_are_exact(L, df, streams):
    s0, _ = streams["clean", (4, 3)]
    s = df.spoiled(s0, [5, 30, 31, 60, 99, 150])
    r = df.run_first_pair(L, s, [0, 100, 127, 200], [[0, 40, 100], [0, 27], [0, 0, 73]], exact=True)
    assert [c["set_first"].tolist() for c in r["calls"]] == [[5, 60], [NONE], [NONE, 23]]
    assert r["first_stats"] == [200, 0]


# 10
@pytest.mark.parametrize("copies", [2, 3])
def test_device_split(L, df, streams, copies):
    s0, _ = streams["clean", (7, 5)]
    # sets span the shards (validators 0 .. 255 in ranges); a set's first failure on one shard, a later one on another
    s = df.spoiled(s0, [96, 97, 98, 99, 250, 520, 700, 900, 1100, 1101, 1500])
    devices = L.hbls_device_count()
    want = df.run_first_pair(L, s, whole(s), [STRADDLING])
    try:
        assert L.hbls_debug_split(copies) == 0 and L.hbls_device_count() == copies * devices
        got = df.run_first_pair(L, s, whole(s), [STRADDLING])
        per_set = df.run_first_pair(L, s, [k * 256 for k in range(8)], [[0, 100, 256]] * 7)
    finally:
        assert L.hbls_debug_split(1) == 0
    for k in df.ROWS + ("set_first",):
        assert np.array_equal(want["calls"][0][k], got["calls"][0][k]), k
    assert np.array_equal(want["count"], got["count"]) and want["set_stats"][:2] == got["set_stats"][:2]
    assert got["calls"][0]["set_first"].tolist() == [96, 250, NONE, 520, 700, 900, 1100, NONE, 1500, NONE]
    assert [c["set_first"].tolist() for c in per_set["calls"]] == \
        [[96, 250], [NONE, NONE], [8, 188], [NONE, 132], [76, NONE], [NONE, 220], [NONE, NONE]]
    assert got["first_stats"][0] == 1792 and got["set_stats"][:2] == [10, 7] and len(got["calls"][0]["fired"]) == 0


# 11
def test_the_three_add_calls_mixed_on_one_duty(L, df, clusters, streams):
    d = clusters[(7, 5)]
    s0, _ = streams["clean", (7, 5)]
    V, n = d["V"], d["n"]
    s = df.spoiled(s0, [V + 10, V + 200, 3 * V, 5 * V + 150])
    bounds = [k * V for k in range(n + 1)]
    modes = ["add", "first", "sets", "first", "add", "first", "sets"]
    r = df.run_first_pair(L, s, bounds, [[0, 100, V]] * n, modes=modes)
    assert r["calls"][1]["set_first"].tolist() == [10, 200] and r["calls"][3]["set_first"].tolist() == [0, NONE]
    assert r["calls"][5]["set_first"].tolist() == [NONE, 150]
    assert r["first_stats"][0] == 3 * V and r["set_stats"][:2] == [10, 4]
    # validators 0 .. 99: peers 0, 2, 4, 5, 6 -> fire in call 6; 100 .. 255: peers 0, 2, 3, 4, 6 -> in call 6 as well
    assert [len(c["fired"]) for c in r["calls"]] == [0, 0, 0, 0, 0, 0, V]
    assert np.array_equal(r["calls"][6]["out"], d["root_sigs"].reshape(V, 96))


# 12
def test_call_errors(L, df, streams):
    s, _ = streams["clean", (4, 3)]
    V = 256
    du = df.FirstDuty(L, s["dv"], s["t"], 8)

    def err(rc):
        return rc, L.hbls_last_error().decode()

    pre = "hbls_duty_add_sets_first: "
    none = "no such duty (never opened, or closed)"
    out = np.zeros(4, np.uint64)
    p = ctypes.c_void_p(out.ctypes.data)
    try:
        du.add_sets_first(s, 0, V, [0, 10, V])
        snap = lambda: (du.state()[0].tolist(), du.state()[1].tolist(), du.stats(), du.set_stats(), du.first_stats())  # noqa: E731
        before = snap()
        assert before[2][:2] == [V, V] and before[3] == [2, 0, 0] and before[4] == [V, 0]
        n = 5
        for off, msg in (([1, 2, n], "set_off[0] must be 0"), ([0, 4, 3, n], "set_off must not decrease"),
                         ([0, 2, 4], "set_off[n_sets] must be n"), ([0, 2, n + 1], "set_off[n_sets] must be n"),
                         ([0], "n_sets is 0 with partials in the call")):
            assert err(du.add_sets_first(s, V, V + n, off, raw=True)) == (-1, pre + msg), off
        assert err(du.add_sets_first(s, V, V + n, None, raw=True, n_sets=2)) == (-1, pre + "set_off is required")
        assert err(du.add_sets_first(s, V, V + n, [0, 2, n], raw=True, no_set_first=True)) == (-1, pre + "set_first is required")
        for bad in (0, du.h + 1000):
            assert err(du.add_sets_first(s, V, V + n, [0, 2, n], raw=True, handle=bad)) == (-1, pre + none)
            assert err(L.hbls_duty_first_stats(bad, p, 1)) == (-1, "hbls_duty_first_stats: " + none)
        assert err(L.hbls_duty_first_stats(du.h, p, 3)) == (-1, "hbls_duty_first_stats: out is null or n above 2")
        assert err(L.hbls_duty_first_stats(du.h, None, 1)) == (-1, "hbls_duty_first_stats: out is null or n above 2")
        assert not out.any()
        assert snap() == before, "nothing was verified, stored or numbered, and the state is unchanged"
        r = du.add_sets_first(s, V, V + n, [0, 0, 2, n, n])  # the next serial is unchanged; empty sets count as seen
        assert r["first"] == V and r["set_first"].tolist() == [NONE] * 4 and du.set_stats() == [6, 0, 0]
        r = du.add_sets_first(s, V + n, V + n, [0, 0])  # no partials: one empty set
        assert r["first"] == V + n and r["set_first"].tolist() == [NONE] and du.set_stats() == [7, 0, 0]
        assert du.first_stats() == [V + n, 0]
    finally:
        closed = du.h
        du.close()
    assert err(du.add_sets_first(s, V, V + 5, [0, 2, 5], raw=True, handle=closed)) == (-1, pre + none)
    assert err(L.hbls_duty_first_stats(closed, p, 2)) == (-1, "hbls_duty_first_stats: " + none)


# 13: the Python layers
def test_parsig_duty_first_error(hipbls, ss, sh, clusters):
    from charon_amd import callers
    d = clusters[(4, 3)]
    V, n, t = d["V"], d["n"], d["t"]
    c = sh.case(ss, d)
    keys = [bytes(c["dv"][v]) for v in range(V)]
    shares = {keys[v]: {s + 1: bytes(c["pks"][v * n + s]) for s in range(n)} for v in range(V)}
    root_sigs = d["root_sigs"].reshape(-1, 96)
    not_verified = "^invalid partial signature: invalid signature: signature not verified$"

    def peer_set(s, vs=range(V)):
        return {keys[v]: callers.ParSig(s + 1, bytes(c["msgs"][v * n + s]), bytes(c["sigs"][v * n + s])) for v in vs}

    def spoiled(s, vs):
        bad = peer_set(s)
        for v in vs:
            bad[keys[v]] = callers.ParSig(s + 1, bad[keys[v]].signing_root, bytes(c["sigs"][((v + 1) % V) * n + s]))
        return bad

    with callers.ParSigDuty(hipbls, t, {k: k for k in keys}, shares, reject_sets=True, first_error=True) as du:
        for s in range(t - 1):
            assert du.store_external(peer_set(s)) == {}
        before = du.state()
        # bad entries in three batches of the set's 256 groups: the error is the first one's, never "unchecked"
        with pytest.raises(callers.CallerError, match=not_verified) as ei:
            du.store_external(spoiled(t - 1, [10, 100, 200]))
        assert ei.value.fired == {} and du.state() == before == {k: (t - 1, False) for k in keys}
        assert du._duty.first_stats()["unchecked"] > 0 and du._duty.first_stats()["partials"] == t * V
        assert du._duty.set_stats()["sets"] == t and du._duty.set_stats()["rejected"] == 1
        res = du.store_external_many([spoiled(t - 1, [3]), {}, peer_set(t - 1)])
        assert isinstance(res[0], callers.CallerError) and str(res[0]) == not_verified[1:-1] and res[1] == {}
        assert res[2] == {keys[v]: bytes(root_sigs[v]) for v in range(V)}
    with callers.ParSigDuty(hipbls, t, {k: k for k in keys}, shares) as du:  # the exact calls stay the default
        du.store_external_many([peer_set(0)])
        assert du._duty.first_stats() == dict(partials=0, unchecked=0)
