"""The batched G2 subgroup test of large device-buffer calls (hipbls.hip verify_subgroup_batch,
msm.hip k_subg_*, subgbatch.h) through the C ABI, -m gpu.

hbls_subgroup_batch(1) brings the test to calls of 96 to 128 signatures, through hbls_verify_device
and hbls_slot_device.  Every status and output byte must equal the same call with the test off
(threshold 0: the per-item ladders alone), and the items the oracle finds off G2 -- exactly those --
are BAD_SIGNATURE.  A wrong sum would hide behind the ladders that run when the test fails, so every
case pins down through hbls_subgroup_batch_stats what ran: with no point off G2 anywhere the test
passes and NO signature is laddered; with one, the test fails and every checked signature is."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

from charon_amd import _lib
from charon_amd._lib import BAD_SIGNATURE, OK

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPERS = os.path.join(ROOT, "tests", "gpu_helpers")
for p in (ROOT, HELPERS):
    if p not in sys.path:
        sys.path.insert(0, p)

import key_learn_slot as ks  # noqa: E402
from oracle import bls12381 as B  # noqa: E402

INF = bytes([0xC0]) + bytes(95)


@pytest.fixture(scope="module")
def L(hipbls):
    return _lib.load_library()


@pytest.fixture(scope="module")
def cluster(L):
    """24 validators x 4 partials over 4 messages (key_learn_slot.WL): 96 signatures"""
    return ks.make_inputs(L)


@pytest.fixture(scope="module")
def torsion():
    with open(os.path.join(ROOT, "tests", "golden", "torsion_points.json")) as f:
        pts = json.load(f)["g2"]["points"]
    return {(x["q"], x["kind"]): B.g2_decompress(bytes.fromhex(x["point"]), subgroup_check=False) for x in pts}


@pytest.fixture(autouse=True)
def _threshold(L):
    prev_a = L.hbls_adaptive(1)
    prev = L.hbls_subgroup_batch(1)
    yield
    L.hbls_subgroup_batch(prev)
    L.hbls_adaptive(prev_a)


def stats(L):
    return _lib.subgroup_batch_stats(L)[0]


def delta(a, b):
    return {k: b[k] - a[k] for k in a}


def verify_device(L, d, sigs):
    """hbls_verify_device over the cluster's partials with the given signatures: the statuses"""
    import torch
    dev = torch.device("cuda", 0)
    NP, M, V = d["NP"], d["M"], d["V"]
    sigs = np.ascontiguousarray(sigs).reshape(-1)
    assert sigs.size == 96 * NP

    def up(a):
        return torch.from_numpy(a).to(dev)

    g = dict(msgs=up(d["msgs"]), moff=up(d["moff"].view(np.int64)), mlen=up(d["mlen"].view(np.int32)), pks=up(d["pks"]),
             sigs=up(sigs), midx=up(d["midx"].view(np.int32)), vgoff=up(d["vgrp_off"].view(np.int32)))
    hm = torch.zeros(M * L.hbls_hm_entry_bytes(), dtype=torch.uint8, device=dev)
    st = torch.full((NP,), 255, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    sp = ctypes.c_void_p(s.cuda_stream)
    ks.chk(L, L.hbls_hash_to_g2_device(ks._p(g["msgs"]), ks._p(g["moff"]), ks._p(g["mlen"]), M, ks._p(hm), sp))
    ks.chk(L, L.hbls_verify_device(ks._p(g["pks"]), ks._p(g["sigs"]), ks._p(g["midx"]), ks._p(hm), NP, ks._p(g["vgoff"]),
                                   V, ks._p(st), sp))
    s.synchronize()
    return st.cpu().numpy().tobytes()


def both(L, d, sigs):
    """the verification and the slot with these signatures: (verify statuses, slot outputs)"""
    return verify_device(L, d, sigs), ks.run_slots(L, dict(d, sigs=np.ascontiguousarray(sigs).reshape(-1)))[0]


def reference(L, d, sigs):
    """the same calls with the batched test off"""
    prev = L.hbls_subgroup_batch(0)
    try:
        s0 = stats(L)
        out = both(L, d, sigs)
        assert delta(s0, stats(L)) == dict(run=0, failed=0, laddered=0, skipped=0)
    finally:
        L.hbls_subgroup_batch(prev)
    return out


def batched(L, d, sigs):
    """the two calls with the batched test on, each from a clean history: the outputs and each
    call's counters"""
    L.hbls_subgroup_batch(1)
    s0 = stats(L)
    v = verify_device(L, d, sigs)
    s1 = stats(L)
    L.hbls_subgroup_batch(1)
    s = ks.run_slots(L, dict(d, sigs=np.ascontiguousarray(sigs).reshape(-1)))[0]
    s2 = stats(L)
    return (v, s), delta(s0, s1), delta(s1, s2)


def add_point(sig_bytes, T):
    return np.frombuffer(B.g2_compress(B.g2_add(B.g2_decompress(bytes(sig_bytes), subgroup_check=False), T)), dtype=np.uint8)


def check_clean(L, d, sigs, checked):
    """no point off G2 among the signatures: the test runs and passes, nothing is laddered"""
    ref = reference(L, d, sigs)
    out, dv, dslot = batched(L, d, sigs)
    assert out == ref
    want = dict(run=1, failed=0, laddered=0, skipped=0)
    assert dv == want and dslot == want
    return np.frombuffer(out[0], dtype=np.uint8)


def check_bad(L, d, sigs, bad, checked=None):
    """the items `bad` are off G2 (by the oracle; the first eight of them asked): exactly they are
    BAD_SIGNATURE, the test fails and every checked signature is laddered"""
    sg = np.ascontiguousarray(sigs).reshape(-1, 96)
    for i in bad[:8]:
        assert not B.g2_in_subgroup(B.g2_decompress(sg[i].tobytes(), subgroup_check=False))
    ref = reference(L, d, sigs)
    out, dv, dslot = batched(L, d, sigs)
    assert out == ref
    for st in (np.frombuffer(out[0], dtype=np.uint8), np.frombuffer(out[1][0], dtype=np.uint8)):
        assert sorted(np.nonzero(st == BAD_SIGNATURE)[0].tolist()) == sorted(bad)
    want = dict(run=1, failed=1, laddered=d["NP"] if checked is None else checked, skipped=0)
    assert dv == want and dslot == want


def test_clean_set(L, cluster):
    st = check_clean(L, cluster, cluster["sigs"], cluster["NP"])
    assert not st.any()


def test_copies_and_negations(L, cluster):
    """64 copies of one valid signature and 16 of its negation (a point of G2 that verifies nothing):
    class sums that add equal points, and sums at infinity"""
    d = cluster
    sg = d["sigs"].reshape(-1, 96).copy()
    one = sg[0].copy()
    neg = np.frombuffer(B.g2_compress(B.g2_neg(B.g2_decompress(one.tobytes()))), dtype=np.uint8)
    sg[:64] = one
    sg[64:80] = neg
    st = check_clean(L, d, sg, d["NP"])
    assert st[0] == OK and st[80:].tolist() == [OK] * (d["NP"] - 80)


def test_undecodable_and_infinity_are_left_out(L, cluster):
    d = cluster
    sg = d["sigs"].reshape(-1, 96).copy()
    und = sg[5].copy()
    und[0] &= 0x7F  # no compression flag
    sg[5] = und
    sg[17] = np.frombuffer(INF, dtype=np.uint8)
    sg[40] = np.frombuffer(bytes([0xBF]) + bytes([0xFF]) * 95, dtype=np.uint8)  # x >= p
    sg[95] = np.frombuffer(INF, dtype=np.uint8)
    st = check_clean(L, d, sg, d["NP"] - 4)
    assert st[5] != OK and st[40] != OK and st[17] != OK and st[95] != OK


@pytest.mark.parametrize("q", ["13", "23"])
def test_one_small_torsion_point(L, cluster, torsion, q):
    d = cluster
    sg = d["sigs"].reshape(-1, 96).copy()
    sg[37] = add_point(sg[37], torsion[(q, "T")])
    check_bad(L, d, sg, [37])


def test_one_point_of_each_larger_order(L, cluster, torsion):
    d = cluster
    sg = d["sigs"].reshape(-1, 96).copy()
    qs = sorted({q for q, _ in torsion} - {"13", "23"}, key=int)
    assert len(qs) == 4
    pos = [3, 30, 64, 95]
    for i, q in zip(pos, qs):
        sg[i] = add_point(sg[i], torsion[(q, "T")])
    check_bad(L, d, sg, pos)


def test_t_and_minus_t(L, cluster, torsion):
    d = cluster
    sg = d["sigs"].reshape(-1, 96).copy()
    sg[10] = add_point(sg[10], torsion[("13", "T")])
    sg[11] = add_point(sg[11], torsion[("13", "-T")])
    check_bad(L, d, sg, [10, 11])


def test_thirteen_items_with_the_same_point(L, cluster, torsion):
    d = cluster
    sg = d["sigs"].reshape(-1, 96).copy()
    pos = list(range(20, 33))
    for i in pos:
        sg[i] = add_point(sg[i], torsion[("13", "T")])
    check_bad(L, d, sg, pos)


def test_every_item_bad(L, cluster, torsion):
    d = cluster
    sg = d["sigs"].reshape(-1, 96).copy()
    T13, T23 = torsion[("13", "T")], torsion[("23", "T")]
    for i in range(d["NP"]):
        sg[i] = add_point(sg[i], T13 if i % 2 else T23)
    check_bad(L, d, sg, list(range(d["NP"])))


def test_committed_off_subgroup_point(L, cluster):
    d = cluster
    with open(os.path.join(ROOT, "tests", "golden", "off_subgroup_g2.json")) as f:
        pt = bytes.fromhex(json.load(f)["points"][0])
    sg = d["sigs"].reshape(-1, 96).copy()
    sg[63] = np.frombuffer(pt, dtype=np.uint8)
    check_bad(L, d, sg, [63])


def test_adaptive_history(L, cluster, torsion):
    """a bad call, then clean ones: the second skips the test and ladders, the third runs it again"""
    d = cluster
    sg = d["sigs"].reshape(-1, 96).copy()
    sg[37] = add_point(sg[37], torsion[("13", "T")])
    L.hbls_subgroup_batch(1)
    s0 = stats(L)
    first = verify_device(L, d, sg)
    s1 = stats(L)
    second = verify_device(L, d, d["sigs"])
    s2 = stats(L)
    third = verify_device(L, d, d["sigs"])
    s3 = stats(L)
    assert delta(s0, s1) == dict(run=1, failed=1, laddered=d["NP"], skipped=0)
    assert delta(s1, s2) == dict(run=0, failed=0, laddered=d["NP"], skipped=1)
    assert delta(s2, s3) == dict(run=1, failed=0, laddered=0, skipped=0)
    assert np.frombuffer(first, dtype=np.uint8)[37] == BAD_SIGNATURE
    assert not any(second) and second == third
    # with the history off every call runs the test
    L.hbls_adaptive(0)
    L.hbls_subgroup_batch(1)
    s0 = stats(L)
    verify_device(L, d, sg)
    verify_device(L, d, d["sigs"])
    assert delta(s0, stats(L)) == dict(run=2, failed=1, laddered=d["NP"], skipped=0)


# ---- device-level comparison: the class sums and the weighted sums on explicit buckets
# (tests/native/subgdev.hip)

R13 = 13 ** 4


@pytest.fixture(scope="module")
def subg_lib(hipbls):
    from gpu_helpers import harness
    D = harness.load("subgdev")
    assert D.sd_keys() == 5 * R13
    D.sd_sums.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.c_char_p, ctypes.c_char_p]
    return D


def _sums(D, buckets):
    """buckets: {(window, value): point}; the 20 sums from the device, and from the oracle"""
    keys = (ctypes.c_uint32 * len(buckets))(*[w * R13 + d for w, d in buckets])
    pts = b"".join(B.g2_compress(P) for P in buckets.values())
    out = ctypes.create_string_buffer(20 * 96)
    assert D.sd_sums(len(buckets), keys, pts, out) == 0
    want = []
    for w in range(5):
        for j in range(4):
            S = None
            for (bw, d), P in buckets.items():
                c = (d // 13 ** j) % 13
                if bw == w and c and P is not None:
                    S = B.g2_add(S, B.g2_mul(P, c))
            want.append(B.g2_compress(S))
    return [out.raw[96 * k:96 * k + 96] for k in range(20)], want


def test_device_sums_against_the_oracle(subg_lib, torsion):
    """one bucket only; digits 0 and 12; a class that sums to infinity; buckets at the slice
    boundaries of a wave's lanes.  Exact."""
    pts = [torsion[k] for k in sorted(torsion)]  # 18 curve points, in G2 and out of it
    P, Q = pts[2], pts[5]
    dig = lambda a, b, c, e: a + 13 * b + 169 * c + 2197 * e  # noqa: E731
    # one bucket only: value 1 of window 0 -- one sum is P, nineteen are at infinity
    got, want = _sums(subg_lib, {(0, 1): P})
    assert got == want and want[0] == B.g2_compress(P) and want[1:] == [INF] * 19
    # digits 0 and 12 in every place, the largest value, and the unused value 0
    got, want = _sums(subg_lib, {(1, dig(12, 0, 12, 0)): P, (1, dig(0, 12, 0, 12)): Q, (4, R13 - 1): pts[8],
                                 (2, 0): pts[11], (3, dig(0, 0, 0, 12)): pts[14]})
    assert got == want and want[8:12] == [INF] * 4
    # a class that sums to infinity: P and -P in two buckets with digit 0 = 7 (their other digits differ)
    got, want = _sums(subg_lib, {(2, dig(7, 1, 0, 0)): P, (2, dig(7, 2, 0, 0)): B.g2_neg(P), (2, dig(3, 0, 0, 5)): Q})
    assert got == want
    # the same point in two buckets of a class (the class sum doubles), and in two lanes' first entries
    got, want = _sums(subg_lib, {(3, dig(4, 0, 0, 0)): P, (3, dig(4, 1, 0, 0)): P, (3, dig(4, 2, 0, 0)): Q})
    assert got == want
    # class (place 0, digit 5) of window 0 has members m -> 5 + 13 m, lane m % 64: the first and last
    # lanes, both sides of each 64-member round, the last round's last member (lane 20) and lane 21's last
    ms = [0, 1, 63, 64, 127, 128, 2175, 2176, 2196, 2133]
    got, want = _sums(subg_lib, {(0, 5 + 13 * m): pts[k % 18] for k, m in enumerate(ms)})
    assert got == want
    # and of a higher place: (place 3, digit 12) has members m -> m + 12 * 2197
    got, want = _sums(subg_lib, {(4, m + 12 * 2197): pts[(k + 3) % 18] for k, m in enumerate(ms)})
    assert got == want
