"""The batched G2 subgroup test on the CPU: its digits (charon_amd/csrc/subgbatch.h compiled by g++
into tests/native/libhbls_subgcheck.so) against a Python restatement, the soundness bound computed
from the window map, the plan's decision (vplan.h subg_batch / subg_skip), and a small model of the
tested sums on the oracle with the committed torsion points."""
import ctypes
import hashlib
import json
import os
import struct
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import bls12381 as B  # noqa: E402

BASE, DIGITS, WINDOWS, RANGE = 13, 4, 5, 13 ** 4


@pytest.fixture(scope="module")
def S():
    from gpu_helpers import harness
    lib = harness.load("subgcheck")
    lib.sg_max_multiplicity.restype = ctypes.c_uint64
    for f in (lib.sg_window_of, lib.sg_digit_of, lib.sg_class_member_of):
        f.restype = ctypes.c_uint32
    return lib


def test_constants(S):
    c = (ctypes.c_uint32 * 8)()
    S.sg_constants(c)
    assert list(c) == [BASE, DIGITS, WINDOWS, RANGE, WINDOWS * RANGE, WINDOWS * DIGITS, WINDOWS * DIGITS * (BASE - 1),
                       RANGE // BASE]
    # the largest digit is below the smallest prime of the G2 cofactor (tests/golden/torsion_points.json)
    with open(os.path.join(ROOT, "tests", "golden", "torsion_points.json")) as f:
        g2 = json.load(f)["g2"]
    primes = sorted({int(x["q"]) for x in g2["points"]})
    h2 = int(g2["cofactor"])
    assert all(h2 % q == 0 for q in primes) and primes[0] == 13 and BASE - 1 < primes[0]
    assert all(h2 % q for q in (2, 3, 5, 7, 11))


def test_every_value_maps_to_its_digits(S):
    for d in range(RANGE):
        want = [(d // BASE ** j) % BASE for j in range(DIGITS)]
        assert [S.sg_digit_of(d, j) for j in range(DIGITS)] == want, d
        assert sum(c * BASE ** j for j, c in enumerate(want)) == d


def test_class_members_are_the_values_with_that_digit(S):
    size = RANGE // BASE
    for j in range(DIGITS):
        for c in range(BASE):
            got = sorted(S.sg_class_member_of(j, c, m) for m in range(size))
            assert got == [d for d in range(RANGE) if (d // BASE ** j) % BASE == c], (j, c)


def test_window_map_and_soundness_bound(S):
    """the largest multiplicity of the window map over all 2^32 words, exact (every preimage
    interval's boundary confirmed through the map), is ceil(2^32 / 13^4); five windows: below 2^-64"""
    mult = S.sg_max_multiplicity()
    assert mult == -(-2 ** 32 // RANGE) == 150379
    # the same from the closed form, value by value
    lo = [-(-(d << 32) // RANGE) for d in range(RANGE + 1)]
    assert lo[0] == 0 and lo[RANGE] == 2 ** 32 and max(b - a for a, b in zip(lo, lo[1:])) == mult
    for d in (0, 1, 2, 12, 13, 28559, 28560):
        assert S.sg_window_of(lo[d]) == d and S.sg_window_of(lo[d + 1] - 1) == d
    assert S.sg_window_of(0) == 0 and S.sg_window_of(2 ** 32 - 1) == RANGE - 1
    # all 20 tests pass only if each of the item's five windows takes one determined value
    assert mult ** WINDOWS * 2 ** 64 < 2 ** (32 * WINDOWS)
    assert mult ** WINDOWS * 2 ** 74 < 2 ** (32 * WINDOWS)  # (2^-74.1)


def test_windows_are_a_sha256_block_of_key_item_domain(S):
    for seed in range(8):
        key = hashlib.sha256(b"subgroup batch key %d" % seed).digest()
        kw = (ctypes.c_uint32 * 8)(*struct.unpack(">8I", key))
        for item in (0, 1, 63, 64, 999_999, 2 ** 32 - 1):
            out = (ctypes.c_uint32 * WINDOWS)()
            S.sg_windows_of(kw, item, out)
            h = hashlib.sha256(key + struct.pack(">I", item) + b"SUBG").digest()
            words = struct.unpack(">8I", h)
            assert list(out) == [(w * RANGE) >> 32 for w in words[:WINDOWS]]
            # never a block the coefficients are drawn from (key || item alone)
            assert h != hashlib.sha256(key + struct.pack(">I", item)).digest()


def plan(S, n, own_sigs, failed, adaptive, min_items):
    out = (ctypes.c_uint64 * 2)()
    assert S.sg_plan((ctypes.c_uint64 * 5)(n, own_sigs, failed, adaptive, min_items), out) == 0
    return bool(out[0]), bool(out[1])


def test_plan(S):
    T = 1 << 19
    assert plan(S, T, 1, 0, 1, T) == (True, False)
    assert plan(S, T - 1, 1, 0, 1, T) == (False, False)  # below the threshold
    assert plan(S, 1_000_000, 1, 0, 1, T) == (True, False)
    assert plan(S, 1_000_000, 0, 0, 1, T) == (False, False)  # signatures handed over, or a host-buffer call
    assert plan(S, 1_000_000, 1, 0, 1, 0) == (False, False)  # 0 = never
    assert plan(S, 96, 1, 0, 1, 1) == (True, False)
    # the history: after a failed test the ladders alone, counted; not without HBLS_ADAPTIVE
    assert plan(S, 1_000_000, 1, 1, 1, T) == (False, True)
    assert plan(S, 1_000_000, 1, 1, 0, T) == (True, False)
    assert plan(S, T - 1, 1, 1, 1, T) == (False, False)
    assert plan(S, 1_000_000, 0, 1, 1, T) == (False, False)


def test_plan_fields_default_off_in_the_general_harness():
    """tests/native/hostcheck.cpp fills plans without the new inputs: no batched test"""
    from gpu_helpers import harness
    lib = harness.load("hostcheck")
    out = (ctypes.c_uint64 * 32)()
    err = ctypes.create_string_buffer(256)
    inp = (ctypes.c_uint64 * 14)(1_000_000, 100_000, 0, 1, 0, 0, 256, 0, 65536, 65536, 128, 32768, 65536, 1)
    assert lib.hc_verify_plan(inp, out, err, 256) == 0


def test_model_sums_leave_g2_exactly_when_the_digits_say(S):
    """sum_i c_i (G_i + T_i) with digits c_i <= 12: its cofactor component is sum_i c_i T_i, which
    is zero exactly when, order by order, the digits' weighted sum vanishes modulo the order"""
    with open(os.path.join(ROOT, "tests", "golden", "torsion_points.json")) as f:
        pts = {(x["q"], x["kind"]): B.g2_decompress(bytes.fromhex(x["point"]), subgroup_check=False)
               for x in json.load(f)["g2"]["points"]}
    T13, M13, Q13 = pts[("13", "T")], pts[("13", "-T")], pts[("13", "G+T")]
    T23, Q23 = pts[("23", "T")], pts[("23", "G+T")]
    G13, G23 = B.g2_add(Q13, M13), B.g2_add(Q23, B.g2_neg(T23))  # the G2 parts
    items = [(Q13, G13, (1, 0)), (B.g2_add(G13, M13), G13, (-1, 0)), (Q23, G23, (0, 1)), (G23, G23, (0, 0)),
             (B.g2_add(Q13, T23), G13, (1, 1))]
    patterns = [(1, 0, 0, 0, 0), (12, 0, 0, 0, 0), (5, 5, 0, 0, 0), (12, 12, 0, 7, 0), (3, 4, 0, 0, 0), (0, 0, 0, 9, 0),
                (0, 0, 11, 0, 0), (1, 2, 0, 0, 1), (6, 7, 0, 0, 0), (0, 1, 1, 0, 1), (0, 1, 12, 3, 1), (0, 0, 0, 0, 0)]
    n_out = 0
    for cs in patterns:
        total, g2part = None, None
        for c, (Q, G, _) in zip(cs, items):
            total = B.g2_add(total, B.g2_mul(Q, c)) if c else total
            g2part = B.g2_add(g2part, B.g2_mul(G, c)) if c else g2part
        w13 = sum(c * t[0] for c, (_, _, t) in zip(cs, items)) % 13
        w23 = sum(c * t[1] for c, (_, _, t) in zip(cs, items)) % 23
        inside = w13 == 0 and w23 == 0
        # G2 and the cofactor group meet in the identity alone: the sum is in G2 iff it IS its G2 part
        diff = B.g2_add(total, B.g2_neg(g2part)) if g2part is not None else total
        assert (diff is None) == inside, cs
        n_out += not inside
    assert 0 < n_out < len(patterns)
    # and by the definition of the subgroup, on one pattern of each kind
    one_in = B.g2_add(B.g2_mul(items[0][0], 5), B.g2_mul(items[1][0], 5))
    one_out = B.g2_add(B.g2_mul(items[0][0], 6), B.g2_mul(items[1][0], 7))
    assert B.g2_in_subgroup(one_in) and not B.g2_in_subgroup(one_out)
