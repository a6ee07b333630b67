"""hash_to_curve G2 on the GPU, stage by stage, against the oracle.

Through the C ABI the hashing only ever meets SHA-256 outputs as u0, u1 and effectively random points
in the cofactor clearing, and the suite's messages were 32 bytes long.  Here the test-only harness
tests/native/devblocks_h2c.hip / devblocks_h2c_std.hip (a library of its own, built for gfx950 from
the product headers and the product's hashsplit.hip) runs each stage on chosen inputs: the leaves
(fp_pow_win's four schedules, fp_sqrt, fp_is_square, f2_sqrt, f2_sgn0, f2_is_lex_largest,
fp_from_mont, fp_from_be512, xmd_b0, xmd_bi), hash_to_field over message lengths around every block
boundary, the map on exceptional u, and the cofactor clearing on exceptional points, in the fast
convention (the staged kernels of hashsplit.hip themselves) and in the standard one (as hash.hip is
compiled); hbls_hash_to_g2_device then runs the same messages through every kernel path.  Every
comparison is exact; the reference is the oracle (oracle/bls12381.py), hashlib or Python integers
(tests/blocks_ref.py maps stored words to field and group elements); the host harness and the other
device path are never the reference.

The standard-convention kernels (the harness's std unit and hash.hip's two kernels) need 3.4 - 3.6 KB of
scratch per lane; their calls are made once, in one child process (tests/gpu_helpers/hash_harness.py
says why, fixture `big`), and only their output words come back to be compared here.

Ranges, derived from the code's comments:
  stored words  a field element is its Montgomery representative plus 0 or p, so every input is below
                2p (fp.h "reduce [0,2p) -> [0,p)": the lazily reduced range), and every stored
                output must be below 2p; fp_from_mont returns the canonical residue below p.
  fp_from_be512 16 big-endian words of any value: its comment admits lo >= 2p (the unbounded second
                operand of the Montgomery product); hi is four words.
  messages      any length; every off[i] + len[i] inside the uploaded buffer (checked on the host).
  points        Jacobian (X, Y, Z) in stored words below 2p; infinity is Z == 0 (mod p), whatever X, Y.
"""
import hashlib
import os
import random
import sys

import numpy as np
import pytest

import blocks_ref as R
from oracle import bls12381 as B

pytestmark = pytest.mark.gpu

HELPERS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_helpers")
if HELPERS not in sys.path:
    sys.path.insert(0, HELPERS)

import hash_harness as H  # noqa: E402
from hash_harness import (M_FIELD, M_HASH, MAX_CASES, S_CLEAR, S_MAP, S_PSI, S_PSI2, ST_CLEAR1, ST_CLEAR3,  # noqa: E402
                          ST_FIELD, ST_MAP, U8P, U32P, U64P)

P = B.P
F2 = B._Fp2Ops


def _ok(rc, what):
    """A failed launch or synchronise (devblocks.h DB_E_LAUNCH, DB_E_SYNC) is a GPU error: the run
    ends there, nothing more is started on the card."""
    if rc in H.GPU_ERRORS:
        pytest.exit(f"{what} returned {rc}: the GPU reported an error; no further block test is run", returncode=3)
    assert rc == 0, f"{what} returned {rc}"


@pytest.fixture(scope="module")
def hh():
    """The hash harness, loaded only if it was built from this tree (its embedded id); otherwise built
    now, and a failure of that fails the tests."""
    from gpu_helpers import harness
    return H.Hash(harness.load_devblocks("hash"), _ok)


# ---- stored words -> values ------------------------------------------------------------------
def _fp(w):
    """the stored integer of 12 words, which must be below 2p"""
    v = R.from_words(w)
    assert v < 2 * P, hex(v)
    return v


def _f2val(w):
    """the field element of 24 stored words"""
    return (R.unmont(_fp(w[:12])), R.unmont(_fp(w[12:24])))


def _jac_point(w):
    """the group element of a Jacobian record (72 words, each coordinate below 2p)"""
    for k in range(6):
        _fp(w[12 * k:12 * k + 12])
    return R.entry_affine(2, [int(v) for v in w])


def _hm_point(w):
    """the group element of an HmEntry (52 words): its flag decides, the coordinates below 2p"""
    x, y = _f2val(w[:24]), _f2val(w[24:48])
    assert int(w[48]) in (0, 1) and not any(int(v) for v in w[49:52])
    if int(w[48]):
        assert x == (0, 0) and y == (0, 0)
        return None
    return (x, y)


def _shapes(n_all):
    return [1, 2, 65, n_all]


# ---- leaves ----------------------------------------------------------------------------------
def _pow_inputs():
    vals = list(dict.fromkeys([0, R.RM, P, P + 1, P - 1, 2 * P - 1] + R.EDGES))
    rng = random.Random(61)
    vals += [rng.randrange(2 * P) for _ in range(100)]
    while len(vals) < 133:
        vals.append(rng.randrange(2 * P))
    assert len(vals) == 133 and all(0 <= v < 2 * P for v in vals)
    return vals


@pytest.mark.parametrize("name", sorted(R.POW_EXP))
def test_fp_pow_win(hh, name):
    """each constant schedule: a^e R^(1 - e), e from the schedule's formula; a 133-case launch (three
    workgroups, the last partly filled) and one-case launches"""
    e, vals = R.POW_EXP[name], _pow_inputs()
    out, _ = hh.leaf("pow_" + name, [R.words(a) for a in vals])
    for a, row in zip(vals, out):
        assert _fp(row[:12]) % P == R.pow_expected(a, e), (name, hex(a))
    for a in (vals[-1], 2 * P - 1, 0):
        out, _ = hh.leaf("pow_" + name, [R.words(a)])
        assert _fp(out[0][:12]) % P == R.pow_expected(a, e), (name, hex(a))


def test_fp_sqrt_and_is_square(hh):
    rng = random.Random(62)
    sq, nsq = [], []
    while len(sq) < 64 or len(nsq) < 64:
        v = rng.randrange(1, P)
        side = sq if B.fp_is_square(v) else nsq
        if len(side) < 64:
            side.append(v)
    raws = [R.mont(v, up) for v in sq + nsq for up in (False, True)] + [0, P]
    assert len(raws) == 258
    for part in (raws[:133], raws[133:]):
        rows = [R.words(a) for a in part]
        roots, ok = hh.leaf("fp_sqrt", rows)
        _, issq = hh.leaf("fp_is_square", rows)
        for a, root, f1, f2 in zip(part, roots, ok, issq):
            v = R.unmont(a)
            want = B.fp_sqrt(v) is not None
            assert want == B.fp_is_square(v)
            assert (f1, f2) == (int(want), int(want)), hex(a)
            if want:
                assert pow(R.unmont(_fp(root[:12])), 2, P) == v, hex(a)
    assert ok[-2:] == [1, 1]  # 0 and p: the square zero


def _f2_sqrt_cases():
    rng = random.Random(63)
    cases = []  # (name, raw c0, raw c1)
    count = {True: 0, False: 0}
    while min(count.values()) < 16:  # 16 squares and 16 non-squares, the first four of each in all four forms
        v = (rng.randrange(P), rng.randrange(P))
        kind = B.f2_is_square(v)
        if count[kind] == 16:
            continue
        count[kind] += 1
        cases += [("random", r0, r1) for r0, r1 in R.reps2(v)[:4 if count[kind] <= 4 else 1]]
    cases += [("zero", a0, a1) for a0 in (0, P) for a1 in (0, P)]
    qr = next(v for v in range(2, 100) if B.fp_is_square(v))
    nqr = next(v for v in range(2, 100) if not B.fp_is_square(v))
    for a0 in (qr, nqr, rng.randrange(P), rng.randrange(P), P - qr, P - nqr):
        for up in (False, True):
            cases += [("in_fp", R.mont(a0, up), 0), ("in_fp", R.mont(a0, up), P)]  # a1 = 0 and a1 = p
            cases += [("imaginary", 0, R.mont(a0, up)), ("imaginary", P, R.mont(a0, up))]
    return cases


def test_f2_sqrt(hh):
    """the oracle's verdict, and x^2 == a for the returned value (no particular root): random squares
    and non-squares, zero in its four stored forms, elements of Fp with a residue and a non-residue as
    a0 (both squares in Fp2: one through y^2 == c, the other through (-h, y)), pure imaginary ones"""
    cases = _f2_sqrt_cases()
    assert len(cases) <= MAX_CASES
    out, ok = hh.leaf("f2_sqrt", [R.words(a0) + R.words(a1) for _, a0, a1 in cases])
    seen = set()
    for (name, a0, a1), row, f in zip(cases, out, ok):
        v = (R.unmont(a0), R.unmont(a1))
        want = B.f2_is_square(v)
        assert f == int(want), (name, hex(a0), hex(a1))
        seen.add((name, want))
        if want:
            assert B.f2_sqr(_f2val(row)) == v, (name, hex(a0), hex(a1))
    # an element of Fp and a pure imaginary one have the norms a0^2, a1^2: both are squares in Fp2
    assert seen == {("random", True), ("random", False), ("zero", True), ("in_fp", True), ("imaginary", True)}


def _sign_values():
    h = (P - 1) // 2
    vals = [(0, 1), (0, 2), (0, P - 1), (0, P - 2), (1, 0), (1, 5), (1, 6), (P - 1, 0), (P - 1, 3), (P - 2, 4), (5, 0), (6, 0),
            (7, h), (7, h + 1), (0, h), (0, h + 1), (h, 0), (h + 1, 0), (h, h + 1), (0, 0)]
    rng = random.Random(64)
    return vals + [(rng.randrange(P), rng.randrange(P)) for _ in range(24)]


def test_sgn0_lex_largest_from_mont(hh):
    """every value in its four stored forms (c0 | c0 + p) x (c1 | c1 + p): the signs are the oracle's
    on the field value whichever form came in, fp_from_mont returns the canonical residue"""
    vals = _sign_values()
    cases = [(v, raw) for v in vals for raw in R.reps2(v)]
    assert len(cases) <= MAX_CASES
    rows = [R.fp2_words(raw) for _, raw in cases]
    _, sgn = hh.leaf("f2_sgn0", rows)
    _, lex = hh.leaf("f2_lex", rows)
    c0, _ = hh.leaf("from_mont", rows)
    c1, _ = hh.leaf("from_mont", [r[12:] + r[:12] for r in rows])
    for (v, raw), s, l, o0, o1 in zip(cases, sgn, lex, c0, c1):
        assert s == B.sgn0_fp2(v), (v, raw)
        assert l == int(B._fp2_lex_largest(v)), (v, raw)
        assert (R.from_words(o0[:12]), R.from_words(o1[:12])) == v, (v, raw)
    # the cases the sign turns on are among them
    assert {B.sgn0_fp2(v) for v in vals if v[0] == 0} == {0, 1}
    assert {B._fp2_lex_largest(v) for v in vals if v[1] == 0} == {False, True}


def test_fp_from_be512(hh):
    rng = random.Random(65)
    ones384 = (1 << 384) - 1
    vals = [0, (1 << 512) - 1, P, 2 * P, 2 * P + 1, ones384, rng.randrange(2 * P, 1 << 384), rng.randrange(2 * P, 1 << 384),
            ((1 << 128) - 1) << 384, 1 << 384, P - 1, 2 * P - 1]
    vals += [rng.randrange(1 << 512) for _ in range(64)]
    rows = [[(v >> (32 * (15 - k))) & 0xFFFFFFFF for k in range(16)] for v in vals]  # W[0] the most significant
    out, _ = hh.leaf("from_be512", rows)
    for v, row in zip(vals, out):
        assert R.unmont(_fp(row[:12])) == v % P, hex(v)
    out, _ = hh.leaf("from_be512", rows[1:2])
    assert R.unmont(_fp(out[0][:12])) == vals[1] % P


def test_xmd_bi(hh):
    rng = random.Random(66)
    dst_prime = R.XMD_TAIL[3:]
    cases = [(bytes(32), 1), (b"\xff" * 32, 255)] + [(bytes(rng.randrange(256) for _ in range(32)), i) for i in range(1, 9)]
    rows = [[int.from_bytes(x[4 * k:4 * k + 4], "big") for k in range(8)] + [i] for x, i in cases]
    out, _ = hh.leaf("xmd_bi", rows)
    for (x, i), row in zip(cases, out):
        got = b"".join(int(w).to_bytes(4, "big") for w in row[:8])
        assert got == hashlib.sha256(x + bytes([i]) + dst_prime).digest(), (x.hex(), i)


@pytest.fixture(scope="module")
def messages():
    return R.h2c_messages()


def _orders(messages):
    """the launches of a message test: 1, 2, 65 messages and the whole list, then the list reversed"""
    return [messages[:n] for n in _shapes(len(messages))] + [messages[::-1]]


def test_xmd_b0(hh, messages):
    """SHA-256 of Z_pad || msg || I2OSP(256, 2) || 0 || DST' for every length around the block
    boundaries, the messages back to back in one buffer"""
    for msgs in _orders(messages):
        got = hh.b0(msgs)
        for m, d in zip(msgs, got):
            assert d == hashlib.sha256(bytes(64) + m + R.XMD_TAIL).digest(), len(m)


def test_message_ranges_are_checked(hh):
    """a message that does not lie inside the uploaded buffer is refused on the host (DB_E_ARG)"""
    b = np.zeros(16, dtype=np.uint8)
    out = np.zeros(216, dtype=np.uint32)
    for off, ln in ((0, 17), (16, 1), (17, 0), (1 << 40, 1)):
        o, n = np.array([off], dtype=np.uint64), np.array([ln], dtype=np.uint32)
        args = (b.ctypes.data_as(U8P), 16, o.ctypes.data_as(U64P), n.ctypes.data_as(U32P))
        assert hh.lib.db_h2c_b0(1, *args, out.ctypes.data_as(U32P)) == -1
        assert hh.lib.db_h2c_std_msg(M_FIELD, 1, *args, out.ctypes.data_as(U32P)) == -1
        assert hh.lib.db_h2c_stages(ST_FIELD, ST_FIELD, 0, 1, *args, None, out.ctypes.data_as(U32P),
                                    out.ctypes.data_as(U32P), out.ctypes.data_as(U32P)) == -1
    assert hh.lib.db_h2c_leaf(0, 257, out.ctypes.data_as(U32P), out.ctypes.data_as(U32P), None) == -1


# ---- the scratch-heavy calls, made in one child process ---------------------------------------------
# (knobs, message counts) of hbls_hash_to_g2_device: the staged kernels with lane-pair and with one-lane
# ladders, then hash.hip's two-lane kernel (an odd n and n = 1: the ii = n - 1 partner lanes run) and
# its one-lane kernel
LIBRARY_PATHS = {
    "staged_pair": ({"HBLS_HASH_SPLIT": 1, "HBLS_HASH_PAIR_MAX": 16384}, [1, 2, 65, None, "rev"]),
    "staged_one_lane": ({"HBLS_HASH_SPLIT": 1, "HBLS_HASH_PAIR_MAX": 0}, [1, 2, 65, None, "rev"]),
    "two_lane": ({"HBLS_HASH_SPLIT": 0, "HBLS_HASH_ONE_LANE": 65536}, [65, 1, None, "rev"]),
    "one_lane": ({"HBLS_HASH_SPLIT": 0, "HBLS_HASH_ONE_LANE": 0}, [None, 1, "rev"]),
}
IN_CHILD = ("two_lane", "one_lane")  # hash.hip's kernels: 3.6 KB of scratch per lane


def _launch(msgs, n):
    """the messages of one launch: the first n, all of them (None) or all of them reversed ("rev")"""
    return msgs[::-1] if n == "rev" else msgs[:n] if n else msgs


@pytest.fixture(scope="module")
def big(hh, messages, sswu, clearing):
    """Every standard-convention call of this file, made once in a child process (hash_harness.py says
    why): {name: output rows}.  The tests below compare the rows with the oracle."""
    hexes = [m.hex() for m in messages]
    jobs = {}
    for k, msgs in enumerate(_orders(hexes)):
        jobs["field%d" % k] = {"kind": "std_msg", "op": M_FIELD, "msgs": msgs}
    jobs["hash_all"] = {"kind": "std_msg", "op": M_HASH, "msgs": hexes}
    jobs["hash_one"] = {"kind": "std_msg", "op": M_HASH, "msgs": hexes[-1:]}
    jobs["map"] = {"kind": "std", "op": S_MAP, "rows": [R.fp2_words(raw) for _, _, raw, _ in sswu]}
    rows = [c[1] + c[2] for c in clearing]
    jobs["clear_all"] = {"kind": "std", "op": S_CLEAR, "rows": rows}
    jobs["clear_one"] = {"kind": "std", "op": S_CLEAR, "rows": rows[1:2]}
    jobs["psi"] = {"kind": "std", "op": S_PSI, "rows": _psi_rows(clearing)}
    jobs["psi2"] = {"kind": "std", "op": S_PSI2, "rows": _psi_rows(clearing)}
    for path in IN_CHILD:
        knobs, counts = LIBRARY_PATHS[path]
        for n in counts:
            jobs["%s:%s" % (path, n)] = {"kind": "library", "knobs": knobs, "msgs": _launch(hexes, n)}
    rc, res = H.run_child(jobs)
    if H.gpu_trouble(rc):  # a GPU error, an abort, a segmentation fault or a hang: nothing more on the card
        pytest.exit(f"the child process ended with {rc}: {res}; no further GPU test is run", returncode=3)
    assert rc == 0, res
    assert sorted(res) == sorted(jobs)
    return res


# ---- hash to field ---------------------------------------------------------------------------
def _check_fields(msgs, rows):
    for m, row in zip(msgs, rows):
        want = B.hash_to_field_fp2(m, 2, B.DST_POP)
        assert [_f2val(row[:24]), _f2val(row[24:48])] == want, len(m)
    assert len(rows) == len(msgs)


def test_hash_to_field_fast(hh, messages):
    """k_h2c_field itself: u0, u1 are the oracle's hash_to_field"""
    for msgs in _orders(messages):
        u, _, _ = hh.stages(ST_FIELD, ST_FIELD, 0, msgs=msgs)
        _check_fields(msgs, u)


def test_hash_to_field_std(big, messages):
    """hash_to_field_fp2 in the standard convention"""
    for k, msgs in enumerate(_orders(messages)):
        _check_fields(msgs, big["field%d" % k])


# ---- end to end ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hashed(messages):
    """the oracle's hash_to_g2 of every message, computed once"""
    return {m: B.hash_to_g2(m) for m in messages}


def test_hash_to_g2_std_unit(big, messages, hashed):
    """hash_to_g2 (h2c.h, what k_hash_to_g2_1 calls) in the standard convention"""
    for msgs, rows in ((messages, big["hash_all"]), (messages[-1:], big["hash_one"])):
        assert len(rows) == len(msgs)
        for m, row in zip(msgs, rows):
            assert _jac_point(row) == hashed[m], len(m)


@pytest.fixture(scope="module")
def L():
    return H.load_library()


@pytest.mark.parametrize("path", sorted(LIBRARY_PATHS))
def test_library_hash_paths(request, messages, hashed, path):
    """hbls_hash_to_g2_device: HmEntry (x, y mod p, inf) is the oracle's hash_to_g2 on every kernel
    path, the knobs that choose it set for the call and put back after it"""
    knobs, counts = LIBRARY_PATHS[path]
    for n in counts:
        msgs = _launch(messages, n)
        assert path != "two_lane" or len(msgs) % 2 == 1 or n in (None, "rev")
        if path in IN_CHILD:
            rows = request.getfixturevalue("big")["%s:%s" % (path, n)]
        else:
            rows = H.library_hash(request.getfixturevalue("L"), msgs, knobs)
        assert len(rows) == len(msgs)
        for m, w in zip(msgs, rows):
            assert _hm_point(w) == hashed[m], (path, len(m))


# ---- the map on chosen u -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def sswu():
    """[(name, u, stored form, the oracle's iso3_map(map_to_curve_sswu(u)))], computed once"""
    ref = {}
    out = []
    for name, u, raw in R.sswu_inputs():
        if u not in ref:
            ref[u] = R.sswu_reference(u)
            assert ref[u] is not None and B.ec_is_on_curve(ref[u], F2, B.B_G2)
        out.append((name, u, raw, ref[u]))
    return out


def test_sswu_inputs_cover_both_branches(sswu):
    rnd = [u for name, u, _, _ in sswu if name.startswith("random")]
    squares = sum(R.sswu_gx1_is_square(u) for u in rnd)
    assert len(rnd) == 40 and squares >= 8 and len(rnd) - squares >= 8
    assert sum(1 for name, *_ in sswu if name.startswith("zero")) == 4
    assert any(raw[0] >= P for _, _, raw, _ in sswu) and any(raw[1] >= P for _, _, raw, _ in sswu)


def _map_stage(hh, sswu, n):
    """k_h2c_map over n messages: message i holds inputs 2i and 2i + 1 (cyclically) -> [(input, point)]"""
    k = len(sswu)
    idx = [((2 * i) % k, (2 * i + 1) % k) for i in range(n)]
    _, q, _ = hh.stages(ST_MAP, ST_MAP, 0, inp=[R.fp2_words(sswu[a][2]) + R.fp2_words(sswu[b][2]) for a, b in idx])
    assert not q[:, 144:].any()  # the third record is the clearing's
    return [(j, _jac_point(q[i][72 * h:72 * h + 72])) for i, ab in enumerate(idx) for h, j in enumerate(ab)]


def test_map_chosen_u(hh, big, sswu):
    """k_h2c_map (65 messages: 130 lanes over three workgroups, u0 and u1 of a message in adjacent
    lanes), sswu_iso_map one lane per case, and sswu_map + iso3_map in the standard convention: each
    result is on E2 and is the oracle's point, Q(-u) = -Q(u), and the three agree"""
    rows = [R.fp2_words(raw) for _, _, raw, _ in sswu]
    leaf = [_jac_point(r) for r in hh.leaf("sswu_iso", rows)[0]]
    std = [_jac_point(r) for r in big["map"]]
    assert len(std) == len(sswu)
    staged = dict(_map_stage(hh, sswu, 65))
    assert sorted(staged) == list(range(len(sswu)))
    by_name = {}
    for j, (name, u, raw, want) in enumerate(sswu):
        for got in (leaf[j], std[j], staged[j]):
            assert got is not None and B.ec_is_on_curve(got, F2, B.B_G2), name
            assert got == want, (name, raw)
        assert leaf[j] == std[j] == staged[j]
        by_name[name] = leaf[j]
    for k in range(6):
        assert by_name["neg%d" % k] == B.g2_neg(by_name["random%d" % k])
    assert len({by_name["zero%d" % k] for k in range(4)}) == 1


@pytest.mark.parametrize("n", [1, 2, 33])
def test_map_stage_shapes(hh, sswu, n):
    for j, got in _map_stage(hh, sswu, n):
        assert got == sswu[j][3], sswu[j][0]


# ---- cofactor clearing on chosen points ----------------------------------------------------------
def _raw_jac(X, Y, Z):
    """a Jacobian record from raw (stored) Fp2 coordinates"""
    return [w for c in (X, Y, Z) for v in c for w in R.words(v)]


@pytest.fixture(scope="module")
def clearing(sswu):
    """33 cases (name, Q0 record, Q1 record, Q0, Q1, the oracle's h_eff (Q0 + Q1)), the exceptional
    ones between generic ones; Z = 1 and Z random, both stored forms, by turns"""
    rng = random.Random(67)
    pts = [want for name, _, _, want in sswu if name.startswith("random")]
    one = R.mont(1)
    inf0 = _raw_jac((one, 0), (one, 0), (0, 0))
    infp = _raw_jac((R.mont(5), P), (R.mont(7, True), 0), (P, P))
    torsion = R.load_torsion()[2]
    special = [("double", pts[20], pts[20]), ("opposite", pts[21], B.g2_neg(pts[21])), ("q1_inf_z0", pts[22], None),
               ("q1_inf_zp", pts[23], None), ("double2", pts[24], pts[24]), ("opposite2", B.g2_neg(pts[25]), pts[25])]
    special += [("torsion%d:%s:" % (j, kind), pt, None) for j, (kind, _, _, pt) in enumerate(torsion)]
    special.append(("generator", B.G2_GEN, None))
    cases, g = [], 0
    for k, (name, a, b) in enumerate(special):
        if k < 4 or k % 6 == 0:  # a generic pair in front
            cases.append(("generic%d" % g, pts[2 * g], pts[2 * g + 1]))
            g += 1
        cases.append((name, a, b))
    assert len(cases) == 33 and g == 8
    out = []
    for k, (name, a, b) in enumerate(cases):
        # Q0 with Z = 1 in even cases, Q1 in every other pair of cases; a doubling never with equal Z
        z0 = F2.one if k % 2 == 0 else R.frand(2, rng)
        z1 = F2.one if k % 4 >= 2 and not name.startswith("double") else R.frand(2, rng)
        up = bool((k >> 1) & 1)
        q0 = R.jac_entry(2, a, z0, upper=up)
        if b is None:
            q1 = {"q1_inf_z0": inf0, "q1_inf_zp": infp}.get(name, infp if k % 2 else inf0)
        else:
            q1 = R.jac_entry(2, b, z1, upper=not up)
        want = B.g2_clear_cofactor(B.g2_add(a, b))
        assert want is None or B.g2_in_subgroup(want), name
        out.append((name, q0, q1, a, b, want))
    names = {c[0]: c[5] for c in out}
    assert names["opposite"] is None and names["opposite2"] is None and names["double"] is not None
    assert all((w is None) == (":G+T:" not in n) for n, w in names.items() if n.startswith("torsion"))
    return out


def _x_mul(pt):
    return B.g2_neg(B.g2_mul(pt, -B.X_PARAM))  # [x] pt, x < 0


@pytest.mark.parametrize("n", [1, 2, 33])
def test_clear_cofactor_staged(hh, clearing, n):
    """k_h2c_clear1 -> 1b -> 2 -> 3 and the same chain with the lane-pair ladders (clear1h / clear2h):
    the HmEntry is the oracle's h_eff (Q0 + Q1) (infinity: inf == 1, later lanes unaffected), the
    parked points P, t1, u, v are the oracle's, and both chains leave the same words"""
    cases = clearing[:n]
    inp = [c[1] + c[2] for c in cases]
    parked = []  # the oracle's P, t1 = [x] P, u = t1 + psi(P), v = psi^2(2P) - psi(P) - P - t1
    for _, _, _, a, b, _ in cases:
        p = B.g2_add(a, b)
        t1, psi_p = _x_mul(p), B.g2_psi(p)
        v = B.g2_add(B.g2_psi(B.g2_psi(B.g2_add(p, p))), B.g2_neg(B.g2_add(B.g2_add(psi_p, p), t1)))
        parked.append((p, t1, B.g2_add(t1, psi_p), v))
    res = {}
    for pair in (0, 1):
        _, qa, _ = hh.stages(ST_CLEAR1, ST_CLEAR1, pair, inp=inp)
        _, q, h = hh.stages(ST_CLEAR1, ST_CLEAR3, pair, inp=inp)
        res[pair] = (qa, q, h)
        for i, (name, *_, want) in enumerate(cases):
            p, t1, u, v = parked[i]
            assert _jac_point(qa[i][:72]) == p, (name, pair)
            assert _jac_point(qa[i][72:144]) == t1, (name, pair)
            assert _jac_point(q[i][72:144]) == u, (name, pair)
            assert _jac_point(q[i][144:216]) == v, (name, pair)
            assert _jac_point(q[i][:72]) == want, (name, pair)
            assert _hm_point(h[i]) == want, (name, pair)
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)  # the same formulas and values, products split or not


def test_clear_cofactor_std(big, clearing):
    """g2_clear_cofactor(jac_add(Q0, Q1)) in the standard convention, 33 cases and one"""
    for cases, got in ((clearing, big["clear_all"]), (clearing[1:2], big["clear_one"])):
        assert len(got) == len(cases)
        for (name, *_, want), row in zip(cases, got):
            assert _jac_point(row) == want, name


def _psi_points(clearing):
    """(name, Jacobian record, group element): Q0 and Q1 of the first twelve clearing cases"""
    return [(c[0], c[1], c[3]) for c in clearing[:12]] + [(c[0] + ":q1", c[2], c[4]) for c in clearing[:12]]


def _psi_rows(clearing):
    return [r[1] for r in _psi_points(clearing)]


def test_psi(big, clearing):
    """g2_psi, g2_psi2 against the oracle's psi applied once and twice, infinity included"""
    pts = _psi_points(clearing)
    assert any(pt is None for _, _, pt in pts) and len(big["psi"]) == len(big["psi2"]) == len(pts)
    for (name, _, pt), r1, r2 in zip(pts, big["psi"], big["psi2"]):
        assert _jac_point(r1) == B.g2_psi(pt), name
        assert _jac_point(r2) == B.g2_psi(B.g2_psi(pt)), name
