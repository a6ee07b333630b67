"""The learned key cache of the device entry points (hipbls.hip key side of verify_pipeline,
vbatch.hip k_pk_lookup / k_pk_miss_dec / k_pk_miss_subgroup / k_pk_learn), -m gpu.

The reference of every test is the same call with HBLS_KEY_LEARN tuned to 0 (every key
decompressed by k_dec_pk + k_g1_subgroup): all status arrays and the aggregates must be byte-equal,
whether a key is a miss (decompressed from the compacted miss list), a hit (copied from the table)
or dropped by a full table.  The counters of hbls_key_learn_stats pin down which of these happened.
Small clusters (tests/gpu_helpers/key_learn_slot.py: 96 pubshares + 24 DV keys, so both lookups
end in a partial wave)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from charon_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPERS = os.path.join(ROOT, "tests", "gpu_helpers")
for p in (ROOT, HELPERS):
    if p not in sys.path:
        sys.path.insert(0, p)

CAP = 4096  # a table far larger than any key set here (the default 2^21 behaves the same)


@pytest.fixture(scope="module")
def L(hipbls):
    return _lib.load_library()


@pytest.fixture(scope="module")
def ks():
    import key_learn_slot
    return key_learn_slot


@pytest.fixture(scope="module")
def cluster(L, ks):
    return ks.make_inputs(L)


@pytest.fixture(autouse=True)
def _restore_knob(L, ks):
    prev = ks.tune(L, "HBLS_KEY_LEARN", CAP)
    yield
    ks.tune(L, "HBLS_KEY_LEARN", prev)


def _reference(L, ks, d, **kw):
    """The same call with the cache off: one output set (every repetition gives the same)."""
    prev = ks.tune(L, "HBLS_KEY_LEARN", 0)
    try:
        before = ks.stats(L)
        out = ks.run_slots(L, d, calls=1, **kw)[0]
        after = ks.stats(L)
    finally:
        ks.tune(L, "HBLS_KEY_LEARN", prev)
    assert (after["hits"], after["misses"], after["size"]) == (before["hits"], before["misses"], 0)
    return out


def _delta(a, b):
    return b["hits"] - a["hits"], b["misses"] - a["misses"]


def _distinct(*arrays):
    return len({bytes(k) for a in arrays for k in np.asarray(a).reshape(-1, 48)})


@pytest.fixture(scope="module")
def ref_clean(L, ks, cluster):
    prev = ks.tune(L, "HBLS_KEY_LEARN", 0)
    try:
        out = ks.run_slots(L, cluster, calls=1)[0]
    finally:
        ks.tune(L, "HBLS_KEY_LEARN", prev)
    assert not any(out[0]) and not any(out[1]) and not any(out[2])  # a clean cluster: every status OK
    assert out[3] == cluster["root_sigs"].tobytes()
    return out


def test_same_outputs_three_calls(L, ks, cluster, ref_clean):
    d = cluster
    keys = _distinct(d["pks"], d["dv_pks"])
    assert keys == d["NP"] + d["V"] == 120
    s = [ks.stats(L)]
    outs = []
    for _ in range(3):
        outs += ks.run_slots(L, d, calls=1)
        s.append(ks.stats(L))
    assert all(o == ref_clean for o in outs)
    assert s[0]["size"] == 0 and s[0]["capacity"] == CAP
    assert _delta(s[0], s[1]) == (0, keys) and s[1]["size"] == keys
    assert _delta(s[1], s[2]) == (keys, 0) and _delta(s[2], s[3]) == (keys, 0)
    assert s[3]["size"] == keys


def _rejected_keys(valid):
    """Keys every decompression must reject (or, the infinity, decode to no point), and one valid
    key: (name, 48 bytes)."""
    from oracle import bls12381 as B
    out = []
    k = bytearray(valid)
    k[0] &= 0x7F
    out.append(("no compression flag", bytes(k)))
    x = 5
    while B.fp_is_square((x * x * x + B.B_G1) % B.P):
        x += 1
    k = bytearray(x.to_bytes(48, "big"))
    k[0] |= 0x80
    out.append(("x with no point on the curve", bytes(k)))
    out.append(("infinity", bytes([0xC0]) + bytes(47)))
    out.append(("non-canonical infinity", bytes([0xC0]) + bytes(46) + b"\x01"))
    out.append(("infinity with the sign flag", bytes([0xE0]) + bytes(47)))
    # on-curve points outside G1: a curve point times r * (the cofactor without its powers of q)
    # has order a power of q; multiplied by q until the next step would reach infinity, order q
    for q in (3, 11):
        h = B.H1
        assert h % q == 0
        while h % q == 0:
            h //= q
        T = None
        for x in range(2, 200):
            y = B.fp_sqrt((x * x * x + B.B_G1) % B.P)
            if y is not None:
                T = B.g1_mul((x, y), B.R * h)
            if T is not None:
                break
        assert T is not None
        while B.g1_mul(T, q) is not None:
            T = B.g1_mul(T, q)
        assert B.ec_is_on_curve(T, B._FpOps, B.B_G1) and not B.g1_in_subgroup(T)
        out.append(("order %d" % q, B.g1_compress(T)))
        with pytest.raises(B.DecodeError):
            B.g1_decompress(out[-1][1])
    for name, kb in out[:2] + out[3:5]:
        with pytest.raises(B.DecodeError):
            B.g1_decompress(kb)
    out.append(("valid", bytes(valid)))
    return out


def test_rejected_keys_cold_and_warm(L, ks, cluster):
    d = cluster
    pks = d["pks"].reshape(-1, 48).copy()
    dv = d["dv_pks"].reshape(-1, 48).copy()
    bad = _rejected_keys(pks[0])
    for j, (_, kb) in enumerate(bad):  # as pubshares (spread over validators) and as DV keys
        pks[5 * j + 1] = np.frombuffer(kb, dtype=np.uint8)
        dv[2 * j + 1] = np.frombuffer(kb, dtype=np.uint8)
    ref = _reference(L, ks, d, pks=pks, dv_pks=dv)
    vst = np.frombuffer(ref[0], dtype=np.uint8)
    ast = np.frombuffer(ref[2], dtype=np.uint8)
    for j, (name, _) in enumerate(bad[:2] + bad[3:7]):  # the reference itself rejects them
        jj = j if j < 2 else j + 1
        assert vst[5 * jj + 1] == _lib.BAD_PUBKEY and ast[2 * jj + 1] != _lib.OK, name
    keys = _distinct(pks, dv)
    s0 = ks.stats(L)
    cold = ks.run_slots(L, d, pks=pks, dv_pks=dv)[0]
    s1 = ks.stats(L)
    warm = ks.run_slots(L, d, pks=pks, dv_pks=dv)[0]
    s2 = ks.stats(L)
    assert cold == ref and warm == ref
    occurrences = d["NP"] + d["V"]
    # the keys used twice (as a pubshare and as a DV key) miss twice in the cold call: the
    # partials' keys are learned behind both lookups
    assert _delta(s0, s1) == (0, occurrences) and s1["size"] == occurrences > keys
    assert _delta(s1, s2) == (occurrences, 0) and s2["size"] == occurrences


def test_mixed_wave(L, ks, cluster, ref_clean):
    d = cluster
    NP, V = d["NP"], d["V"]
    new = ks.fresh_keys(L, 18, seed=3)
    pks = d["pks"].reshape(-1, 48).copy()
    pos = list(range(2, 62, 3))  # 20 positions interleaved with K1 over the first wave
    assert len(pos) == 20
    for j, i in enumerate(pos):
        pks[i] = new[0] if j in (4, 9, 17) else new[1 + (j - (j > 4) - (j > 9) - (j > 17))]
    assert _distinct(pks[pos]) == 18 and sum(bytes(pks[i]) == bytes(new[0]) for i in pos) == 3
    ref = _reference(L, ks, d, pks=pks)  # (first: re-tuning the knob empties the table)
    assert ks.run_slots(L, d)[0] == ref_clean  # K1 warm
    s0 = ks.stats(L)
    assert s0["size"] == NP + V
    out = ks.run_slots(L, d, pks=pks)[0]
    s1 = ks.stats(L)
    again = ks.run_slots(L, d, pks=pks)[0]
    s2 = ks.stats(L)
    assert out == ref and again == ref and ref != ref_clean
    assert _delta(s0, s1) == (NP - 20 + V, 20)  # K1's occurrences hit; every new occurrence misses
    assert s1["size"] == s0["size"] + 20  # at most one entry per occurrence
    assert _delta(s1, s2) == (NP + V, 0) and s2["size"] == s1["size"]


@pytest.mark.parametrize("cap", [64, 4, 3, 1])
def test_full_table_and_wrap(L, ks, cap):
    """200 distinct keys against a table of `cap` entries (its index has the next power of two
    >= 2 cap slots: with so few, probes that start near its end wrap around)."""
    wl = dict(validators=40, n=4, t=3, distinct=False, n_msgs=4)
    d = ks.make_inputs(L, wl)
    assert _distinct(d["pks"], d["dv_pks"]) == 200
    ref = _reference(L, ks, d)
    ks.tune(L, "HBLS_KEY_LEARN", cap)
    s = ks.stats(L)
    assert (s["size"], s["capacity"]) == (0, cap)
    for call in range(4):
        assert ks.run_slots(L, d)[0] == ref, call
        s1 = ks.stats(L)
        assert s1["size"] == cap
        # the table filled in the first call and keeps its entries: exactly they hit afterwards
        assert _delta(s, s1) == ((0, 200) if call == 0 else (cap, 200 - cap)), call
        s = s1


def test_slots_in_flight_from_cold(L, ks, cluster, ref_clean):
    d = cluster
    s0 = ks.stats(L)
    assert s0["size"] == 0
    outs = ks.run_slots(L, d, calls=3, sync_between=False)
    s1 = ks.stats(L)
    assert all(o == ref_clean for o in outs)
    keys = d["NP"] + d["V"]
    # the ordering invariant: the second and third slots' lookups ran behind the first's inserts
    assert _delta(s0, s1) == (2 * keys, keys) and s1["size"] == keys


def test_reset(L, ks, cluster, ref_clean):
    d = cluster
    keys = d["NP"] + d["V"]
    assert ks.run_slots(L, d)[0] == ref_clean
    assert ks.stats(L)["size"] == keys
    ks.chk(L, L.hbls_pubkey_cache_clear())
    s0 = ks.stats(L)
    assert s0["size"] == 0
    assert ks.run_slots(L, d)[0] == ref_clean
    s1 = ks.stats(L)
    assert _delta(s0, s1) == (0, keys) and s1["size"] == keys
    assert ks.tune(L, "HBLS_KEY_LEARN", 2 * CAP) == CAP
    s2 = ks.stats(L)
    assert (s2["size"], s2["capacity"]) == (0, 2 * CAP)
    assert ks.run_slots(L, d)[0] == ref_clean
    s3 = ks.stats(L)
    assert _delta(s2, s3) == (0, keys) and s3["size"] == keys
    # key tables bypass the cache
    assert ks.run_slots(L, d, tables=True)[0] == ref_clean
    assert ks.stats(L) == s3


@pytest.mark.parametrize("value", ["0", "50"])
def test_environment(ks, cluster, ref_clean, value):
    env = {k: v for k, v in os.environ.items() if k != "HBLS_KEY_LEARN"}
    env["HBLS_KEY_LEARN"] = value
    p = subprocess.run([sys.executable, "-u", os.path.join(HELPERS, "key_learn_slot.py")], env=env,
                       capture_output=True, text=True, timeout=240)
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert p.returncode == 0 and lines, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    res = json.loads(lines[-1])
    assert res["env"] == value and res["vstatus_all_ok"]
    assert res["digests"] == [ks.digest(ref_clean)] * 3
    keys = cluster["NP"] + cluster["V"]
    st = res["stats"]
    if value == "0":
        assert st == {"size": 0, "capacity": 0, "hits": 0, "misses": 0}
    else:  # 50 entries: filled by the first call, 50 hits in each of the next two
        assert st == {"size": 50, "capacity": 50, "hits": 100, "misses": 3 * keys - 100}
