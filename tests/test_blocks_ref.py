"""tests/blocks_ref.py, the Python side of tests/test_gpu_blocks.py, checked on the CPU: the map
between the oracle's Fp12 and pair3.h's lane form against hc_pairing (so that a wrong map cannot
pass for a kernel bug), the conjugation shortcut against the power, and the lazy-limb case
generators against lazy28.py's model and the host build of the same products."""
import ctypes
import random

import pytest

import blocks_ref as R
from charon_amd.tools import lazy28
from oracle import bls12381 as B


@pytest.fixture(scope="module")
def hc():
    from gpu_helpers import harness
    return harness.load("hostcheck")


def test_lane_map_matches_hc_pairing(hc):
    """e(P, Q)^3 of the oracle, taken through poly_to_lanes, is what hc_pairing returns in tower
    order; the map inverts; raw lanes carry the Montgomery factor"""
    rng = random.Random(5)
    a, b = rng.randrange(1, B.R), rng.randrange(1, B.R)
    Pt, Q = B.g1_mul(B.G1_GEN, a), B.g2_mul(B.G2_GEN, b)
    o = ctypes.create_string_buffer(576)
    assert hc.hc_pairing(B.g1_compress(Pt), B.g2_compress(Q), o) == 0
    ours = [int.from_bytes(o.raw[48 * i:48 * i + 48], "big") for i in range(12)]
    e = B.pairing(Pt, Q)
    e3 = B._p12_mul(B._p12_mul(e, e), e)
    lanes = R.poly_to_lanes(e3)
    assert R.lanes_tower_order(lanes) == ours
    assert R.lanes_to_poly(lanes) == e3
    assert R.raw_to_poly(R.poly_to_raw(e3)) == e3 and R.raw_to_poly(R.poly_to_raw(e3, upper=True)) == e3
    # the exponents of the GPU test: f^CYC_EXP lies in the cyclotomic subgroup (order p^4 - p^2 + 1),
    # and FEXP3 is the cube of the oracle's final exponentiation
    f = [rng.randrange(B.P) for _ in range(12)]
    assert B._p12_pow(B._p12_pow(f, R.CYC_EXP), B.P ** 4 - B.P ** 2 + 1) == B.P12_ONE
    assert B._p12_pow(f, R.FEXP3) == B._p12_pow(B.final_exponentiation(f), 3)


def test_lane_form_of_one_line_and_conjugate():
    rng = random.Random(6)
    assert R.poly_to_lanes(B.P12_ONE) == [(1, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)]
    assert R.poly_to_raw(B.P12_ONE, upper=True)[0] == (R.RM + B.P, B.P, B.P, B.P)
    f = [rng.randrange(B.P) for _ in range(12)]
    assert R.p12_conj(f) == B._p12_pow(f, B.P ** 6)
    # a0 + a1 v + b1 v w with v = w^2: the oracle's own embedding of Fp2 times powers of w
    a0, a1, b1 = [(rng.randrange(B.P), rng.randrange(B.P)) for _ in range(3)]
    w = [0, 1] + [0] * 10
    w2 = B._p12_mul(w, w)
    w3 = B._p12_mul(w2, w)
    want = B._p12_add(B._fp2_to_p12(a0), B._p12_add(B._p12_mul(B._fp2_to_p12(a1), w2), B._p12_mul(B._fp2_to_p12(b1), w3)))
    assert R.line_poly(a0, a1, b1) == want
    # every is-one case but the first three differs from one
    for name, raw, one in R.is_one_values():
        assert (R.raw_to_poly(raw) == B.P12_ONE) == one, name
        assert all(v < 2 * B.P for lane in raw for v in lane)


def test_stored_edge_values():
    assert all(v < 2 * B.P for v in R.EDGES)
    for want in (0, 1, 2, B.P - 2, B.P - 1, B.P, B.P + 1, 2 * B.P - 1, 2 * B.P - 2, (1 << 381) - 1, 1 << 380,
                 2 * B.P - (1 << 200), R.RM, R.RM * R.RM % B.P):
        assert want in R.EDGES
    assert any(R.words(v)[:11] == [0xFFFFFFFF] * 11 for v in R.EDGES)
    assert any(R.limbs(v)[:13] == [R.M28] * 13 for v in R.EDGES)
    q = R.fp2_quads()
    for c in ((0, R.TOP, 0, R.TOP), (R.TOP, 0, R.TOP, 0), (R.TOP, 0, 0, R.TOP), (0, R.TOP, R.TOP, 0), (R.P,) * 4):
        assert c in q
    assert len(set(R.inv_values())) == 64 and {0, B.P, B.P + 1, R.TOP, (B.P + 1) // 2} <= set(R.inv_values())
    assert R.from_words(R.words(R.TOP)) == R.TOP and R.lvalue(R.limbs(20 * B.P - 1)) == 20 * B.P - 1


def test_lazy_generators_are_admitted():
    """Every generated operand set passes lazy28.py's model (the generators assert it; a rejected
    one raises here), covers normalised values up to VMAX - 1 multiples of p and un-normalised
    patterns, and starts with an admitted worst case above 3/4 of the 64-bit accumulator;
    check_lazy accepts Python's own Montgomery product of such operands."""
    mul, sqr = R.mul_cases("Fp"), R.sqr_cases("Fp")
    assert R.col_max(*mul[0]) > 3 << 62 and R.col_max(sqr[0], sqr[0]) > 3 << 62
    assert any(R.lvalue(a) >= 19 * B.P and max(a) <= R.M28 for a, _ in mul)
    assert any(max(a) > R.M28 for a, _ in mul) and any(max(a) > R.M28 for a in sqr)
    with pytest.raises(AssertionError):  # the model does reject: two operands shifted by 3
        big = R.l_shl(R.all_ones(19), 3)
        lazy28.mul(R.bound(big), R.bound(big))
    f2m = R.f2mul_cases()
    assert any(R.lvalue(c[0]) >= 15 * B.P for c in f2m)
    for st in R.SQR_SITES:
        assert len(R.f2sqr_cases(st)) > 40
    assert len(R.dot_cases()) == 2 * len(f2m)
    for a, b in mul[:50]:
        va, vb = R.lvalue(a), R.lvalue(b)
        m = (-va * vb * pow(B.P, -1, 1 << 392)) % (1 << 392)
        R.check_lazy(R.limbs((va * vb + m * B.P) >> 392), va * vb, va * vb)


@pytest.mark.parametrize("field", [1, 2])
def test_curve_point_formats(field):
    """the raw point formats of the curve harness: every representative of a group element (any Z,
    any admitted multiple of p on top, lazy limbs or stored words) decodes to that element, the
    product records have layout.h's sizes, and infinity is Z = 0 mod p or the flag"""
    rng = random.Random(70 + field)
    g = B.G1_GEN if field == 1 else B.G2_GEN
    pt = R.ec_mul(field, g, 0xABCDEF)
    vmax = lazy28.VMAX["Fp" if field == 1 else "Fp2"]
    for lazy, kmax in ((True, vmax - 1), (False, 1)):
        for _ in range(4):
            lam = R.frand(field, rng)
            slots = R.raw_slots(field, R.jac_coords(field, pt, lam), [rng.randrange(kmax + 1) for _ in range(6)])
            assert all(v < (kmax + 1) * B.P for v in slots)
            got, inf, normalised = R.unpack_point(R.pack_point(slots, False, lazy), lazy)
            assert got == slots and not inf and normalised and R.affine_of(field, got) == pt
    for k in (0, 1):
        assert R.affine_of(field, R.raw_slots(field, R.jac_coords(field, None, None), k)) is None
    assert R.affine_of(field, R.raw_slots(field, R.jac_coords(field, pt, R.FIELD_OPS[field].one)), inf=True) is None
    assert len(R.affine_entry(field, pt)) == (28, 52)[field - 1] and R.affine_entry(field, None)[-4] == 1
    assert len(R.jac_entry(field, pt)) == 36 * field
    assert R.entry_affine(field, R.jac_entry(field, pt, R.frand(field, rng), upper=True)) == pt
    assert R.entry_affine(field, R.jac_entry(field, None, upper=True)) is None


def test_msm_reference_is_linear():
    """-psi^2 is an endomorphism: the term-by-term MSM reference equals the sum taken in scalars over
    a base point (what tests/test_gpu_curve.py uses for its larger inputs)"""
    q = B.g2_mul(B.G2_GEN, 987654321)
    img = B.g2_neg(B.g2_psi(B.g2_psi(q)))
    ms, coefs = [3, 5, 3, 70000], [(0x10001, 0xFFFF0000), (7, 0), (0, 9), (0xFFFFFFFF, 0x80000001)]
    want = B.g2_add(B.g2_mul(q, sum(m * a for m, (a, _) in zip(ms, coefs))),
                    B.g2_mul(img, sum(m * b for m, (_, b) in zip(ms, coefs))))
    assert R.msm_reference([B.g2_mul(q, m) for m in ms], coefs) == want
    assert R.msm_reference([q, None], [(0, 0), (5, 5)]) is None


def test_torsion_fixture_loads():
    t = R.load_torsion()
    assert {q for _, q, _, _ in t[1]} >= {3, 11} and {q for _, q, _, _ in t[2]} >= {13, 23}
    for field in (1, 2):
        for kind, q, order, pt in t[field]:
            assert B.ec_is_on_curve(pt, R.FIELD_OPS[field], R.CURVE_B[field])
            if kind in ("T", "-T"):
                assert order == q


def test_hash_helpers():
    """the generators of tests/test_gpu_hash.py: the message list (every length, neighbours of
    different block counts, enough for a 65-message launch), the exponents and expected value of
    fp_pow_win, the four stored forms, and the map's inputs on both branches"""
    msgs = R.h2c_messages()
    assert len(msgs) == len(set(msgs)) >= 65 and {len(m) for m in msgs} == set(R.H2C_LENGTHS)
    assert [R.xmd_b0_blocks(n) for n in (8, 9, 72, 73, 136, 137)] == [1, 2, 2, 3, 3, 4]
    assert len(R.XMD_TAIL) == 47 and (16 + 47 + 1) % 64 == 0 and (80 + 47 + 1) % 64 == 0  # 0x80 ends a block
    for name, e in R.POW_EXP.items():
        for a in (R.mont(12345), R.mont(12345, True), 0):
            assert R.unmont(R.pow_expected(a, e)) == pow(R.unmont(a), e, R.P), name
    assert 4 * R.POW_EXP["SQRT"] - 1 == R.P == 4 * R.POW_EXP["P_M3_4"] + 3 == 2 * R.POW_EXP["LEGENDRE"] + 1
    v = (5, R.P - 7)
    assert len(set(R.reps2(v))) == 4 and all((R.unmont(a), R.unmont(b)) == v for a, b in R.reps2(v))
    inputs = R.sswu_inputs()
    rnd = [u for name, u, _ in inputs if name.startswith("random")]
    squares = sum(R.sswu_gx1_is_square(u) for u in rnd)
    assert len(rnd) == 40 and squares >= 8 and len(rnd) - squares >= 8
    assert all((R.unmont(raw[0]), R.unmont(raw[1])) == u and max(raw) < 2 * R.P for _, u, raw in inputs)
    assert B.ec_is_on_curve(R.sswu_reference((0, 0)), B._Fp2Ops, B.B_G2)


def _be(v):
    return b"".join(int(c).to_bytes(48, "big") for c in v)


def _hc_lines(hc, Q, ev):
    """hc_line_chain28's 68 lines of Q (pair28.h's lazy-limb chain), as field elements"""
    stored, lazy = ctypes.create_string_buffer(288 * R.N_LINES), ctypes.create_string_buffer(288 * R.N_LINES)
    cnt = (ctypes.c_ulonglong * 2)()
    assert hc.hc_line_chain28(_be(Q[0] + Q[1]), ev, stored, lazy, cnt) == 0
    out = []
    for buf in (stored.raw, lazy.raw):
        v = [int.from_bytes(buf[48 * i:48 * i + 48], "big") for i in range(6 * R.N_LINES)]
        out.append([((v[6 * j], v[6 * j + 1]), (v[6 * j + 2], v[6 * j + 3]), (v[6 * j + 4], v[6 * j + 5]))
                    for j in range(R.N_LINES)])
    return out


def test_miller_reference_matches_host_lines(hc):
    """tests/test_gpu_pairing.py's reference against the g++ build: the chain has X_PARAM's 68 steps;
    every line of both host chains satisfies line_matches against it, unevaluated and evaluated at
    -g1, and a changed line does not; the Python schedule over the host's evaluated lines, and the
    oracle's own Miller value, give hc_pairing's e(-g1, Q)^3 after exponentiation."""
    rng = random.Random(8)
    Q = B.g2_mul(B.G2_GEN, rng.randrange(1, B.R))
    chain = R.miller_chain(Q)
    assert R.N_LINES == 68 and [s[0] for s in chain].count("dbl") == 63 and chain[0][2:] == Q
    assert [s[0] for s in chain[:6]] == ["dbl", "add", "dbl", "dbl", "add", "dbl"]  # |x| = 0b1101...
    neg = R.G1_NEG
    for ev, at in ((0, None), (1, neg)):
        for lines in _hc_lines(hc, Q, ev):
            assert all(R.line_matches(l, s, at) for l, s in zip(lines, chain))
            assert not R.line_matches(lines[1], chain[2], at)
            a0, c1, c2 = lines[5]
            assert not R.line_matches((a0, B.f2_add(c1, (1, 0)), c2), chain[5], at)
            assert not R.line_matches(((0, 0), (0, 0), (0, 0)), chain[5], at)  # c2 = 0 matches nothing
    stored, lazy = _hc_lines(hc, Q, 1)
    unev = _hc_lines(hc, Q, 0)[1]
    assert [R.eval_line(l, neg) for l in unev] == lazy
    f = R.miller_from_lines(lazy)
    want = R.pairing3(neg, Q)
    assert f != B.miller_loop(neg, Q)  # the raw values differ by the lines' Fp4 factors
    assert R.pow3(f) == want == R.pow3(R.miller_from_lines(stored))
    o = ctypes.create_string_buffer(576)
    assert hc.hc_pairing(B.g1_compress(neg), B.g2_compress(Q), o) == 0
    assert R.lanes_tower_order(R.poly_to_lanes(want)) == [int.from_bytes(o.raw[48 * i:48 * i + 48], "big") for i in range(12)]
    # several chains share the squarings: the product of the single loops
    Q2 = B.g2_mul(B.G2_GEN, 77)
    l2 = [R.eval_line(l, B.G1_GEN) for l in _hc_lines(hc, Q2, 0)[0]]
    assert R.miller_from_lines(lazy, l2) == B._p12_mul(f, R.miller_from_lines(l2))
    # the stored-word formats round-trip
    w = R.f12_words(f, upper=True)
    assert len(w) == R.F12_WORDS and R.f12_of_words(w)[0] == f and min(R.f12_of_words(w)[1]) >= B.P
    lw = [x for c in lazy[3] for v in c for x in R.words(R.mont(v))]
    assert len(lw) == R.LINE_WORDS and R.line_of_words(lw)[0] == lazy[3]


def test_fixed_base_matches_the_oracle():
    """blocks_ref.FixedBase (the expectations of tests/test_gpu_vbatch.py) against the oracle's
    scalar multiplication on both curves: edge scalars, random ones, and a base that is a multiple"""
    rng = random.Random(3101)
    for field, gen, mul in ((1, B.G1_GEN, B.g1_mul), (2, B.g2_mul(B.G2_GEN, 77), B.g2_mul)):
        fb = R.FixedBase(field, gen)
        for k in [0, 1, 2, 15, 16, 17, B.R - 1, B.R, B.R + 5, R.LAMBDA, (1 << 255) % B.R] + \
                [rng.randrange(B.R) for _ in range(4)]:
            assert fb.mul(k) == mul(gen, k % B.R), (field, k)


def test_rlc_restatements_match_host_check(hc):
    """The restated coefficients (hashlib), the eigenvalue and the sparse digit table against the host
    check: hc_rlc_coeffs word for word; the dense and sparse chunk sums (hc_rlc_sum_g1, _g1_sparse,
    _g2_sparse, _g2_lazy) equal ONE scalar multiplication [sum r_i k_i] of the base, with keys k_i G1
    and signatures k_i Q -- how tests/test_gpu_vbatch.py computes every expectation."""
    rng = random.Random(3102)
    key = [rng.getrandbits(32) for _ in range(8)]
    ab = (ctypes.c_uint32 * 2)()
    for item in [0, 1, 2, 63, 64, 65, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF] + [rng.getrandbits(32) for _ in range(20)]:
        hc.hc_rlc_coeffs((ctypes.c_uint32 * 8)(*key), item, ab)
        assert (ab[0], ab[1]) == R.rlc_coeffs(key, item), item
        rec = R.rlc_record(key, item)
        assert rec[0] == ab[0] & 0x3FFFFFFF and rec[1] == ab[1] & 0x3FFFFFFF and rec[2] < 64 and rec[3] == 1
    assert R.rlc_coeffs(key, 1) != R.rlc_coeffs(key, 2) and R.rlc_coeffs(key[::-1], 1) != R.rlc_coeffs(key, 1)
    # the digit table: every three-bit digit at every position of a record
    for j in range(R.SPARSE_DIGITS):
        for d in range(8):
            rec = [0, 0, 0, 1]
            rec[j // 10] = d << (3 * (j % 10))
            u, v = R.SPARSE_PAIRS[d & 3]
            sgn = -1 if d & 4 else 1
            # the other positions hold digit 0 = (1, 0)
            rest = sum(4 ** i for i in range(R.SPARSE_DIGITS) if i != j)
            assert R.sparse_ab(rec) == (sgn * u * 4 ** j + rest, sgn * v * 4 ** j)
    Q = B.g2_mul(B.G2_GEN, 0x1234567)
    f1, f2 = R.FixedBase(1, B.G1_GEN), R.FixedBase(2, Q)
    for fn in ("hc_rlc_sum_g1", "hc_rlc_sum_g1_sparse", "hc_rlc_sum_g2_sparse", "hc_rlc_sum_g2_lazy"):
        getattr(hc, fn).argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_char_p]
    for k in (1, 5, 16):
        ks = [rng.randrange(1, B.R) for _ in range(k)]
        pks = b"".join(B.g1_compress(f1.mul(s)) for s in ks)
        sigs = b"".join(B.g2_compress(f2.mul(s)) for s in ks)
        dense = [R.rlc_coeffs(key, 100 + i) for i in range(k)]
        recs = [R.rlc_record(key, 100 + i) for i in range(k)]
        s_dense = sum(R.rlc_scalar(a, b) * s for (a, b), s in zip(dense, ks)) % B.R
        s_sparse = sum(R.rlc_scalar(*R.sparse_ab(r)) * s for r, s in zip(recs, ks)) % B.R
        flat2 = (ctypes.c_uint32 * (2 * k))(*[x for p in dense for x in p])
        flat4 = (ctypes.c_uint32 * (4 * k))(*[x for r in recs for x in r])
        o48, o96 = ctypes.create_string_buffer(48), ctypes.create_string_buffer(96)
        assert hc.hc_rlc_sum_g1(k, pks, flat2, o48) == 0 and o48.raw == B.g1_compress(f1.mul(s_dense))
        assert hc.hc_rlc_sum_g2_lazy(k, sigs, flat2, o96) == 0 and o96.raw == B.g2_compress(f2.mul(s_dense))
        assert hc.hc_rlc_sum_g1_sparse(k, pks, flat4, o48) == 0 and o48.raw == B.g1_compress(f1.mul(s_sparse))
        assert hc.hc_rlc_sum_g2_sparse(k, sigs, flat4, o96) == 0 and o96.raw == B.g2_compress(f2.mul(s_sparse))


def test_plan_restatement_properties():
    """blocks_ref.plan_chunks: the chunks of a group partition its items in order, sizes differ by at
    most one and none exceeds cmax, bit 31 exactly for groups of one, the total within n // cmax + ng"""
    rng = random.Random(3103)
    for cmax in (1, 2, 3, 16):
        sizes = [rng.choice([0, 1, 2, 15, 16, 17, 31, 32, 33, 100]) for _ in range(40)]
        off = [0]
        for s in sizes:
            off.append(off[-1] + s)
        cnt, coff, cfirst, ccount = R.plan_chunks(off, cmax)
        assert coff[-1] == len(cfirst) <= off[-1] // cmax + len(sizes)
        for g, s in enumerate(sizes):
            cs = [(cfirst[c], ccount[c] & 0x7FFFFFFF, ccount[c] >> 31) for c in range(coff[g], coff[g + 1])]
            assert sum(c[1] for c in cs) == s and all(c[2] == (s == 1) for c in cs)
            assert not cs or (max(c[1] for c in cs) - min(c[1] for c in cs) <= 1 and max(c[1] for c in cs) <= cmax)
            pos = off[g]
            for f, n, _ in cs:
                assert f == pos and n >= 1
                pos += n


# ---- the threshold aggregation's references (tests/test_gpu_threshold.py) ----
def test_ta_lambda_matches_the_oracle():
    """blocks_ref.ta_lambda against oracle.bls12381.lagrange_coeffs_at_zero wherever that is defined,
    and None entries exactly where a member sees the combine failure; ta_digits recomposes"""
    import itertools
    rng = random.Random(3104)
    sets = [list(c) for t in range(1, 6) for c in itertools.combinations(range(1, 8), t)]
    sets += [[3, 1, 2], [-1, 5, 2], [1, 64, 65, 130], [2 ** 62 - 1, 1, 2], [-(2 ** 62 - 1), 2 ** 62, 7],
             [2 ** 63 - 1, -2 ** 63, 1], [2 ** 63 - 1, -2 ** 63, 2 ** 62, -3]]
    sets += [[rng.randrange(-2 ** 63, 2 ** 63) for _ in range(rng.randrange(1, 18))] for _ in range(40)]
    for ids in sets:
        want = B.lagrange_coeffs_at_zero(ids)
        assert want is not None and R.ta_lambda(ids) == want, ids
        for lam in want:
            a = R.ta_digits(lam)
            assert len(a) == 4 and R.ta_digit_scalar(a) == lam
    assert R.TA_Z == -B.X_PARAM == 0xd201000000010000 and B.R < R.TA_Z ** 4
    for ids, none_at in (([0, 1, 2], [1, 2]), ([1, 1, 2], [0, 1]), ([0, 0, 3], [0, 1, 2]), ([4, 5, 4, 0], [0, 1, 2]),
                         ([5, 7, 5 + B.R], None)):
        assert B.lagrange_coeffs_at_zero(ids) is None
        if none_at is not None:  # the last set is no set of 64-bit indices: the oracle's rule is mod r
            assert [j for j, lam in enumerate(R.ta_lambda(ids)) if lam is None] == none_at, ids
    assert R.ta_lambda([0]) == [1] == B.lagrange_coeffs_at_zero([0])


def test_ta_small_split_matches_the_host_check(hc):
    """blocks_ref.ta_small_split against hc_ta_small (ta_small.h compiled for the CPU) over every 2- to
    7-subset of 1..10 -- c_j and s equal, and lambda_j = s c_j -- and over the refusal list of
    tests/test_hostcheck.py::test_ta_small_split, with the other refusals the header names"""
    import itertools
    c, s = (ctypes.c_int64 * 16)(), ctypes.create_string_buffer(32)

    def host(ids):
        if not hc.hc_ta_small((ctypes.c_int64 * len(ids))(*ids), len(ids), c, s):
            return None
        return [int(c[j]) for j in range(len(ids))], int.from_bytes(s.raw, "big")
    n = 0
    for t in range(2, 8):
        for ids in itertools.combinations(range(1, 11), t):
            got = R.ta_small_split(list(ids))
            assert got is not None and got == host(ids), ids
            assert [got[1] * cj % B.R for cj in got[0]] == R.ta_lambda(list(ids)), ids
            n += 1
    assert n == sum(len(list(itertools.combinations(range(10), t))) for t in range(2, 8))
    edge = [-2 ** 30, 2 ** 30, -2 ** 30 + 1, -2 ** 30 + 4]  # E_0 = -2^63 exactly
    for bad in ([0, 1, 2], [1, 1, 2], [5], list(range(1, 18)), edge, [1, 2 ** 31], [1, -2 ** 31], [2 ** 31 - 1, -2 ** 31 + 1, 5, 9],
                list(range(1, 65, 4))):
        assert R.ta_small_split(bad) is None and host(bad) is None, bad
    rng = random.Random(3105)
    seen = set()
    for _ in range(300):  # shuffled, signed and wide sets: the two agree on taking or refusing, and on the values
        ids = rng.sample(range(-40, 41), rng.randrange(2, 17)) if rng.random() < 0.7 else \
            [rng.randrange(-2 ** 31 + 1, 2 ** 31) for _ in range(rng.randrange(2, 5))]
        got = R.ta_small_split(ids)
        assert got == host(ids), ids
        seen.add(got is None)
        if got:
            assert [got[1] * cj % B.R for cj in got[0]] == R.ta_lambda(ids), ids
    assert seen == {True, False}
    assert R.ta_small_split([1, 2 ** 31 - 1]) == host([1, 2 ** 31 - 1]) is not None


def test_ta_digit_sum_is_one_fixed_base_multiplication():
    """sum_i a_i (-1)^i psi^i(sigma) = [(sum_i a_i z^i) k mod r] Q for sigma = [k] Q, against the oracle's
    g2_psi, for digit vectors that are no digits of a reduced scalar too (z - 1 in every position)"""
    rng = random.Random(3106)
    Q = B.g2_mul(B.G2_GEN, rng.randrange(1, B.R))
    fb = R.FixedBase(2, Q)
    z = R.TA_Z
    for a in ([1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [z - 1] * 4, [0, 0, 0, 0],
              [rng.randrange(z) for _ in range(4)], R.ta_digits(rng.randrange(B.R))):
        k = rng.randrange(1, B.R)
        sigma, acc = fb.mul(k), None
        w = sigma
        for i in range(4):
            term = B.g2_mul(w, a[i])
            acc = B.g2_add(acc, B.g2_neg(term) if i & 1 else term)
            w = B.g2_psi(w)
        assert acc == fb.mul(R.ta_digit_scalar(a) * k), a
