"""The ladder tables of learned keys through the C ABI (hipbls.hip kl_table, vbatch.hip k_pk_wide,
k_rlc_msm<1, *>, k_rlc<1>; ec28.h g1_wide_build, g1l_msm_ladder_wide, g1l_mul_wide), -m gpu.

A slot of 64 validators of a 10-operator threshold-7 cluster over distinct messages (640 pubshares
+ 64 DV keys), with hbls_fe_batch, hbls_slot_msm and hbls_rlc_lanes set so that the slot-wide check
and the chunked combination run at this size: one chunk of 10 items per validator, one per-item
ladder per DV key.  A wrong table sum would hide behind the per-batch fallback (which recomputes
everything without tables and still returns the right verdicts), so every test pins down through
hbls_key_wide_stats which ladders ran, and the child-process test through hbls_stats that the
slot-wide check passed."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from charon_amd import _lib
from charon_amd._lib import BAD_PUBKEY, NOT_VERIFIED, OK

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPERS = os.path.join(ROOT, "tests", "gpu_helpers")
for p in (ROOT, HELPERS):
    if p not in sys.path:
        sys.path.insert(0, p)

import key_wide_slot as kw  # noqa: E402

V, N, NP = kw.WL["validators"], kw.WL["n"], kw.WL["validators"] * kw.WL["n"]
KEYS = NP + V  # 704


@pytest.fixture(scope="module")
def L(hipbls):
    return _lib.load_library()


@pytest.fixture(scope="module")
def cluster(L):
    return kw.make_inputs(L)


@pytest.fixture(scope="module")
def other(L):
    """a second cluster of the same shape with other keys, messages and signatures"""
    return kw.make_inputs(L, rank=1)


@pytest.fixture(autouse=True)
def _knobs(L):
    """the slot-wide check and the chunked combination at this size; a cleared cache"""
    prev = kw.set_knobs(L)
    kw.ks.chk(L, L.hbls_pubkey_cache_clear())
    yield
    kw.restore_knobs(L, prev)


def _delta(a, b):
    return {k: b[k] - a[k] for k in a}


def _zero(**kv):
    z = dict(built=0, wide_chunks=0, narrow_chunks=0, wide_items=0, narrow_items=0)
    z.update(kv)
    return z


def _all_ok(d, out):
    vst, tst, ast, tout = out
    return not any(vst) and not any(tst) and not any(ast) and tout == d["root_sigs"].tobytes()


def test_two_calls_from_a_cleared_cache(L, cluster):
    d = cluster
    s0 = kw.wide_stats(L)
    first = kw.ks.run_slots(L, d)[0]
    s1 = kw.wide_stats(L)
    second = kw.ks.run_slots(L, d)[0]
    s2 = kw.wide_stats(L)
    assert _delta(s0, s1) == _zero(built=KEYS, narrow_chunks=V, narrow_items=V)
    assert _delta(s1, s2) == _zero(wide_chunks=V, wide_items=V)
    assert second == first
    assert _all_ok(d, first)  # every status OK, the aggregates are the root keys' signatures


def test_slot_wide_check_passes_through_tables():
    """the same two calls in a child process with HBLS_STATS=1: the second call's slot-wide check
    ran and passed, so the sums through the tables are the right group elements"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("HBLS_")}
    env["HBLS_STATS"] = "1"
    p = subprocess.run([sys.executable, "-u", os.path.join(HELPERS, "key_wide_slot.py")], env=env,
                       capture_output=True, text=True, timeout=240)
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert p.returncode == 0 and lines, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    res = json.loads(lines[-1])
    assert res["second_call_wide"] == _zero(wide_chunks=V, wide_items=V)
    assert res["second_call_stats"][4] >= 1 and res["second_call_stats"][5] == 0
    assert res["equal"] and res["all_ok"]


def _mixed(d, o, which):
    """d with the keys, partials, messages and root signatures of validators `which` taken from o"""
    m = dict(d)
    pks, opks = d["pks"].reshape(V, N * 48).copy(), o["pks"].reshape(V, N * 48)
    sigs, osigs = d["sigs"].reshape(V, N * 96).copy(), o["sigs"].reshape(V, N * 96)
    dv, odv = d["dv_pks"].reshape(V, 48).copy(), o["dv_pks"].reshape(V, 48)
    root, oroot = d["root_sigs"].reshape(V, 96).copy(), o["root_sigs"].reshape(V, 96)
    msgs, omsgs = d["msgs"].reshape(-1, 32).copy(), o["msgs"].reshape(-1, 32)
    assert d["M"] == V and np.array_equal(d["midx"], np.repeat(np.arange(V, dtype=np.uint32), N))
    for v in which:
        pks[v], sigs[v], dv[v], root[v], msgs[v] = opks[v], osigs[v], odv[v], oroot[v], omsgs[v]
    m.update(pks=pks.reshape(-1), sigs=sigs.reshape(-1), dv_pks=dv.reshape(-1), root_sigs=root.reshape(-1),
             msgs=msgs.reshape(-1))
    return m


def test_one_wave_with_both_kinds(L, cluster, other):
    d = cluster
    assert _all_ok(d, kw.ks.run_slots(L, d)[0])
    fresh = list(range(1, V, 2))  # every other validator: table chunks and others in neighbouring lanes
    m = _mixed(d, other, fresh)
    s0 = kw.wide_stats(L)
    out = kw.ks.run_slots(L, m)[0]
    s1 = kw.wide_stats(L)
    assert _all_ok(m, out)
    h = V // 2
    assert _delta(s0, s1) == _zero(built=h * (N + 1), wide_chunks=h, narrow_chunks=h, wide_items=h, narrow_items=h)


def test_corrupted_partial_inside_a_table_chunk(L, cluster):
    import bench
    d = cluster
    assert _all_ok(d, kw.ks.run_slots(L, d)[0])
    c = dict(d, sigs=d["sigs"].copy())
    bench.corrupt(L, c, 3 / NP, seed=5, classes=(2,))  # bench.py's wrong-message class, one partial
    assert c["n_corrupted"] == 1 and int((c["exp_v"] != OK).sum()) == 1
    s0 = kw.wide_stats(L)
    vst, tst, ast, _ = kw.ks.run_slots(L, c)[0]
    s1 = kw.wide_stats(L)
    assert _delta(s0, s1) == _zero(wide_chunks=V, wide_items=V)
    vst = np.frombuffer(vst, dtype=np.uint8)
    assert np.array_equal(vst, c["exp_v"]) and vst[np.nonzero(c["exp_v"])[0][0]] == NOT_VERIFIED
    assert np.array_equal(np.frombuffer(tst, dtype=np.uint8), c["exp_ta"])
    assert np.array_equal(np.frombuffer(ast, dtype=np.uint8), c["exp_agg"])


def test_bad_keys_in_a_chunk(L, cluster):
    """an undecodable key, an off-subgroup key and the infinity key in validator 3's chunk: no
    tables for them, the chunk runs without tables, statuses as without any table"""
    d = cluster
    with open(os.path.join(ROOT, "tests", "golden", "torsion_points.json")) as f:
        tors = [x for x in json.load(f)["g1"]["points"] if x["kind"] == "G+T"][0]
    pks = d["pks"].reshape(NP, 48).copy()
    und = bytearray(pks[0].tobytes())
    und[0] &= 0x7F  # no compression flag
    bad = [bytes(und), bytes.fromhex(tors["point"]), bytes([0xC0]) + bytes(47)]
    pos = [3 * N + 1, 3 * N + 4, 3 * N + 8]  # (positions 1, 4, 8: aggregated members and others)
    for i, kb in zip(pos, bad):
        pks[i] = np.frombuffer(kb, dtype=np.uint8)
    prev = kw.ks.tune(L, "HBLS_KEY_WIDE", 0)
    try:
        ref = kw.ks.run_slots(L, d, pks=pks)[0]
    finally:
        kw.ks.tune(L, "HBLS_KEY_WIDE", prev)
    rv = np.frombuffer(ref[0], dtype=np.uint8)
    assert rv[pos[0]] == BAD_PUBKEY and rv[pos[1]] == BAD_PUBKEY and rv[pos[2]] != OK
    assert int((rv != OK).sum()) == 3
    s0 = kw.wide_stats(L)
    cold = kw.ks.run_slots(L, d, pks=pks)[0]
    s1 = kw.wide_stats(L)
    warm = kw.ks.run_slots(L, d, pks=pks)[0]
    s2 = kw.wide_stats(L)
    assert cold == ref and warm == ref
    assert _delta(s0, s1) == _zero(built=KEYS - 3, narrow_chunks=V, narrow_items=V)
    assert _delta(s1, s2) == _zero(wide_chunks=V - 1, narrow_chunks=1, wide_items=V)


def test_capacity(L, cluster):
    d = cluster
    ref = kw.ks.run_slots(L, d)[0]
    assert _all_ok(d, ref)
    # a cache of 64 entries for 704 keys: the keys that did not fit stay on the old path
    prev = kw.ks.tune(L, "HBLS_KEY_LEARN", 64)
    try:
        s0 = kw.wide_stats(L)
        outs = [kw.ks.run_slots(L, d)[0] for _ in range(2)]
        s1 = kw.wide_stats(L)
        assert outs == [ref, ref]
        dl = _delta(s0, s1)
        assert dl["built"] == 64 and kw.ks.stats(L)["size"] == 64
        # 64 of the 704 keys have a table: at most 6 whole chunks of 10, and every ladder is counted
        assert dl["wide_chunks"] + dl["narrow_chunks"] == 2 * V and dl["wide_chunks"] <= 6
        assert dl["wide_items"] + dl["narrow_items"] == 2 * V and dl["wide_items"] <= 64
    finally:
        kw.ks.tune(L, "HBLS_KEY_LEARN", prev)
    # no tables at all
    prev = kw.ks.tune(L, "HBLS_KEY_WIDE", 0)
    try:
        s0 = kw.wide_stats(L)
        outs = [kw.ks.run_slots(L, d)[0] for _ in range(2)]
        s1 = kw.wide_stats(L)
        assert outs == [ref, ref] and kw.ks.stats(L)["size"] == KEYS
        assert _delta(s0, s1) == _zero(narrow_chunks=2 * V, narrow_items=2 * V)
    finally:
        kw.ks.tune(L, "HBLS_KEY_WIDE", prev)
    # tables for the first 100 entries only
    prev = kw.ks.tune(L, "HBLS_KEY_WIDE", 100)
    try:
        s0 = kw.wide_stats(L)
        outs = [kw.ks.run_slots(L, d)[0] for _ in range(2)]
        s1 = kw.wide_stats(L)
        assert outs == [ref, ref] and _delta(s0, s1)["built"] == 100
    finally:
        kw.ks.tune(L, "HBLS_KEY_WIDE", prev)
    # after a clear the next call builds the tables again
    assert kw.ks.run_slots(L, d)[0] == ref
    kw.ks.chk(L, L.hbls_pubkey_cache_clear())
    s0 = kw.wide_stats(L)
    assert kw.ks.run_slots(L, d)[0] == ref
    s1 = kw.wide_stats(L)
    assert _delta(s0, s1) == _zero(built=KEYS, narrow_chunks=V, narrow_items=V)
    assert kw.ks.run_slots(L, d)[0] == ref
    assert _delta(s1, kw.wide_stats(L)) == _zero(wide_chunks=V, wide_items=V)


def test_call_too_small_to_chunk(L):
    """4 validators with the default hbls_rlc_lanes: one ladder per item, through the tables once
    the keys are learned"""
    wl = dict(kw.WL, validators=4)
    d = kw.make_inputs(L, wl=wl)
    prev = L.hbls_rlc_lanes(0)
    try:
        s0 = kw.wide_stats(L)
        cold = kw.ks.run_slots(L, d)[0]
        s1 = kw.wide_stats(L)
        warm = kw.ks.run_slots(L, d)[0]
        s2 = kw.wide_stats(L)
    finally:
        L.hbls_rlc_lanes(prev)
    assert _all_ok(d, cold) and warm == cold
    assert _delta(s0, s1) == _zero(built=44, narrow_items=44)
    assert _delta(s1, s2) == _zero(wide_items=44)


# ---- device-level comparison: the host test's chunk cases on the device (tests/native/widedev.hip)

@pytest.fixture(scope="module")
def wide_lib(hipbls):
    from gpu_helpers import harness
    W = harness.load("widedev")
    u32p = ctypes.POINTER(ctypes.c_uint32)
    W.wd_chunks.argtypes = [ctypes.c_int, ctypes.c_char_p, u32p, ctypes.c_int, u32p, u32p, ctypes.c_char_p,
                            ctypes.c_char_p]
    return W


def test_device_chunks_against_the_oracle(wide_lib):
    """every chunk case of tests/test_key_wide_host.py in ONE wave (a lane per chunk; chunks of 1,
    2, 10 and 16 items in neighbouring lanes), the tables built on the device; and each chunk's
    first item through the one-item ladder.  Exact."""
    import key_wide_cases as C
    from oracle import bls12381 as B
    cases = C.cases()
    # size-major -> case-major: lanes 4 j .. 4 j + 3 hold case j at the sizes 1, 2, 10, 16
    cases = [cases[s * C.PER_SIZE + j] for j in range(C.PER_SIZE) for s in range(len(C.SIZES))] + \
        cases[len(C.SIZES) * C.PER_SIZE:]
    assert len(cases) <= 64 and [len(pts) for pts, _ in cases[:4]] == list(C.SIZES)
    pts_all, ab_all, first, cnt = [], [], [], []
    for pts, ab in cases:
        first.append(len(pts_all))
        cnt.append(len(pts))
        pts_all += pts
        ab_all += ab
    n, nc = len(pts_all), len(cases)
    pks = b"".join(B.g1_compress(p) for p in pts_all)
    coef = (ctypes.c_uint32 * (2 * n))(*[w for pair in ab_all for w in pair])
    cf = (ctypes.c_uint32 * nc)(*first)
    cc = (ctypes.c_uint32 * nc)(*cnt)
    out = ctypes.create_string_buffer(48 * nc)
    one = ctypes.create_string_buffer(48 * nc)
    assert wide_lib.wd_chunks(n, pks, coef, nc, cf, cc, out, one) == 0
    for c, (pts, ab) in enumerate(cases):
        assert out.raw[48 * c:48 * c + 48] == C.want(pts, ab), (c, len(pts), ab)
        assert one.raw[48 * c:48 * c + 48] == C.want(pts[:1], ab[:1]), (c, ab[0])
