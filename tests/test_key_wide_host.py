"""The ladder tables of learned keys on the CPU (tests/native/widecheck.cpp: the g++ build of
ec28.h g1_wide_build, g1l_msm_ladder_wide and g1l_mul_wide, what vbatch.hip k_pk_wide,
k_rlc_msm<1, 2> and k_rlc<1> run on the device).  Every comparison is exact, against the oracle's
group law on compressed points (tests/key_wide_cases.py)."""
import ctypes
import random

import pytest

import key_wide_cases as C
from oracle import bls12381 as B


@pytest.fixture(scope="module")
def lib():
    from gpu_helpers import harness
    L = harness.load("widecheck")
    u32p = ctypes.POINTER(ctypes.c_uint32)
    L.wc_table.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    L.wc_chunk_wide.argtypes = [ctypes.c_int, ctypes.c_char_p, u32p, ctypes.c_char_p]
    L.wc_chunk_narrow.argtypes = [ctypes.c_int, ctypes.c_char_p, u32p, ctypes.c_char_p]
    L.wc_item_wide.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p]
    return L


def _chunk(lib, fn, pts, ab):
    buf = b"".join(B.g1_compress(p) for p in pts)
    flat = (ctypes.c_uint32 * (2 * len(ab)))(*[x for pair in ab for x in pair])
    out = ctypes.create_string_buffer(48)
    assert getattr(lib, fn)(len(pts), buf, flat, out) == 0
    return out.raw


@pytest.mark.parametrize("which", ["random key", "generator"])
def test_table_entries(lib, which):
    """all 15 entries are [d0 + 2^16 d1 + lambda (d2 + 2^16 d3)] P"""
    P = C.keys()[0] if which == "random key" else B.G1_GEN
    out = ctypes.create_string_buffer(48 * 15)
    assert lib.wc_table(B.g1_compress(P), out) == 0
    for d in range(1, 16):
        d0, d1, d2, d3 = d & 1, (d >> 1) & 1, (d >> 2) & 1, (d >> 3) & 1
        assert out.raw[48 * (d - 1):48 * d] == C.want([P], [(d0 + (d1 << 16), d2 + (d3 << 16))]), d


def test_chunk_sums(lib):
    """sum (a_i + b_i lambda) P_i through the tables: chunks of 1, 2, 10 and 16 items, the fixed
    pairs, random pairs, (0, 0) on one item, and the degenerate chunks"""
    cases = C.cases()
    assert {len(pts) for pts, _ in cases[:len(C.SIZES) * C.PER_SIZE]} == set(C.SIZES)
    for pts, ab in cases:
        assert _chunk(lib, "wc_chunk_wide", pts, ab) == C.want(pts, ab), (len(pts), ab)


def test_one_item_ladder(lib):
    """k_rlc<1>'s form: one key, the fixed pairs and random ones"""
    rng = random.Random(77)
    pairs = C.FIXED + [(rng.getrandbits(32), rng.getrandbits(32)) for _ in range(10)] + [(0, 0)]
    for P in (C.keys()[4], B.G1_GEN):
        for a, b in pairs:
            out = ctypes.create_string_buffer(48)
            assert lib.wc_item_wide(B.g1_compress(P), a, b, out) == 0
            assert out.raw == C.want([P], [(a, b)]), (a, b)


def test_wide_equals_narrow_random_chunks(lib):
    """200 random chunks: the 16-step ladder through the tables and the 32-step ladder through the
    per-slot table give the same point (and the oracle's, on every tenth)"""
    rng = random.Random(20)
    keys = C.keys()
    for it in range(200):
        k = rng.randrange(1, 17)
        pts = [keys[rng.randrange(len(keys))] for _ in range(k)]
        ab = [(rng.getrandbits(32), rng.getrandbits(32)) for _ in range(k)]
        w = _chunk(lib, "wc_chunk_wide", pts, ab)
        assert w == _chunk(lib, "wc_chunk_narrow", pts, ab), it
        if it % 10 == 0:
            assert w == C.want(pts, ab), it
