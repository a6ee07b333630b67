"""The curve layer on the GPU against the oracle's group law: exceptional additions, small-torsion
points and the slot-wide bucket MSM.

Through the C ABI the curve code (ec28.h lazy-limb points, ec.h stored-word Jacobian arithmetic, the
endomorphism subgroup tests, the chunk ladders, msm.hip) only ever meets effectively random points,
which never take the branches where such code goes wrong: H == 0 (a multiple k p in lazy limbs,
decided by l_is_zero_n's double-precision estimate), rr == 0, doubling, infinity.  Here the test-only
harness tests/native/devblocks_curve.hip / devblocks_msm.hip (a library of its own, built for gfx950
from the product headers and the product's msm.hip) runs each function on chosen raw inputs.  Every
comparison is exact; the oracle (oracle/bls12381.py) or Python integers are the only reference (tests/blocks_ref.py
maps raw limbs to group elements); the host harness is never the reference.

Ranges, derived from ec28.h's comments and charon_amd/tools/lazy28.py:
  l_is_zero_n  a normalised value below 2^392 (14 x 28 bits), so k = a / p up to (2^392 - 1) // p;
               l_is_zero carries first (lazy28.norm: no limb passes 2^32 on the way).  The formulas
               test H = U2 + S p - X1 and rr = 2 S2 + S' p - 2 Y1 with S, S' from lazy28.KSITE
               (*_H, *_R: at most 41) and products below 2p, so k <= 45 occurs; every k <= 64 is
               tried, as tests/test_lazy28.py does for the g++ build.
  l_red        limbs below 2^32, not necessarily carried, value below 2^390 (lazy28.red).
  points       coordinates normalised and below VMAX p (lazy28.VMAX: 20 for G1, 16 for G2), an
               affine operand of a mixed addition below 2p; stored words below 2p.
"""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

import blocks_ref as R
from charon_amd.tools import lazy28
from oracle import bls12381 as B

pytestmark = pytest.mark.gpu

P = B.P
U32P = ctypes.POINTER(ctypes.c_uint32)
U8P = ctypes.POINTER(ctypes.c_uint8)
I32P = ctypes.POINTER(ctypes.c_int)
VP = ctypes.c_void_p

ONE, HALF = 0, 1
P_OPS = {n: i for i, n in enumerate("l_dbl l_madd l_add l_tojac l_fromjac j_dbl j_add j_add_aff j_eq".split())}
S_OPS = {n: i for i, n in enumerate("is_zero f2_is_zero norm red".split())}
LD_MUL, LD_SUB = 0, 1
MAX_LANES = 256  # cases per launch
X_ABS = -B.X_PARAM
LAMBDA = (-B.X_PARAM ** 2) % B.R


def _ok(rc, what):
    """A failed launch or synchronise (devblocks.h DB_E_LAUNCH, DB_E_SYNC) is a GPU error: the run
    ends there, nothing more is started on the card."""
    if rc in (-5, -6):
        pytest.exit(f"{what} returned {rc}: the GPU reported an error; no further block test is run", returncode=3)
    assert rc == 0, f"{what} returned {rc}"


def _u32(a):
    return np.ascontiguousarray(np.array(a, dtype=np.uint64).astype(np.uint32))


class Curve:
    def __init__(self, lib):
        self.lib = lib
        lib.db_build_id.restype = ctypes.c_char_p
        for f in (1, 2):
            getattr(lib, "db_point_g%d" % f).argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, U32P, U32P, I32P]
        lib.db_lazy_scalar.argtypes = [ctypes.c_int, ctypes.c_int, U32P, U32P, I32P]
        lib.db_ladder.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, VP, VP, I32P]
        lib.db_chunk_ladder.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, VP, U32P, U32P, U32P, VP]
        lib.db_msm.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, U32P, U8P, U32P, U8P, U32P, U32P, U8P, U32P]
        self.g_ready = lib.db_g_ready()
        self.msm_chunk = lib.db_msm_chunk()
        assert lib.db_msm_keys() == 2 << 16

    def scalar(self, op, cases):
        """cases: [(limbs a, limbs b)] -> ([14 limbs], [flag])"""
        outs, flags = [], []
        for s in range(0, len(cases), MAX_LANES):
            part = cases[s:s + MAX_LANES]
            n = len(part)
            inp = _u32([list(a) + list(b) for a, b in part])
            out, fl = np.zeros((n, 14), dtype=np.uint32), np.zeros(n, dtype=np.int32)
            _ok(self.lib.db_lazy_scalar(S_OPS[op], n, inp.ctypes.data_as(U32P), out.ctypes.data_as(U32P),
                                        fl.ctypes.data_as(I32P)), f"db_lazy_scalar({op})")
            outs += [[int(v) for v in row] for row in out]
            flags += [int(v) for v in fl]
        return outs, flags

    def point(self, field, mode, op, cases):
        """cases: [(record P, record Q)] -> per case the lanes' (record, flag): one lane, or the two
        lanes of its pair"""
        per = 2 if mode == HALF else 1
        res = []
        for s in range(0, len(cases), MAX_LANES // per):
            part = cases[s:s + MAX_LANES // per]
            n = len(part)
            inp = _u32([p + q for p, q in part])
            threads = self.lib.db_curve_threads(mode, n)
            assert threads >= per * n
            out, fl = np.zeros((threads, R.PT_WORDS), dtype=np.uint32), np.zeros(threads, dtype=np.int32)
            rc = getattr(self.lib, "db_point_g%d" % field)(mode, P_OPS[op], n, inp.ctypes.data_as(U32P),
                                                          out.ctypes.data_as(U32P), fl.ctypes.data_as(I32P))
            _ok(rc, f"db_point_g{field}({mode}, {op})")
            assert not out[per * n:].any()  # lanes without a case store nothing
            res += [[(out[per * i + h], int(fl[per * i + h])) for h in range(per)] for i in range(n)]
        return res

    def ladder(self, field, mode, op, entries):
        """entries: [record words] -> per case the lanes' (Jacobian record words, flag)"""
        per = 2 if mode == HALF else 1
        n = len(entries)
        assert per * n <= MAX_LANES
        inp = _u32(entries)
        threads = self.lib.db_curve_threads(mode, n)
        rec = 36 * field
        out, fl = np.zeros((threads, rec), dtype=np.uint32), np.zeros(threads, dtype=np.int32)
        _ok(self.lib.db_ladder(field, mode, op, n, inp.ctypes.data, out.ctypes.data, fl.ctypes.data_as(I32P)),
            f"db_ladder({field}, {mode}, {op})")
        return [[([int(v) for v in out[per * i + h]], int(fl[per * i + h])) for h in range(per)] for i in range(n)]

    def chunk(self, field, sparse, tab, coef, ranges):
        """tab: per item its 3 (4) affine group elements; coef: per item 2 (4) words; ranges:
        [(first, cnt)] one lane each -> [group element]"""
        items, n = len(tab), len(ranges)
        assert n <= MAX_LANES
        t = _u32([R.jac_entry(field, pt) for row in tab for pt in row])
        c = _u32(coef)
        first, cnt = _u32([r[0] for r in ranges]), _u32([r[1] for r in ranges])
        out = np.zeros((n, 36 * field), dtype=np.uint32)
        _ok(self.lib.db_chunk_ladder(field, 1 if sparse else 0, n, items, t.ctypes.data, c.ctypes.data_as(U32P),
                                     first.ctypes.data_as(U32P), cnt.ctypes.data_as(U32P), out.ctypes.data),
            f"db_chunk_ladder({field}, {sparse})")
        return [R.entry_affine(field, [int(v) for v in row]) for row in out]

    def msm(self, sig, coef, igrp, gst, sig_st=None, agg=(), agg_st=None, sig_inf=None, upper=False):
        """sig: n group elements (sig_inf: flags set on otherwise finite records), agg: n_agg;
        coef: n + n_agg pairs -> total[0] as a group element"""
        n, n_agg = len(sig), len(agg)
        assert n + n_agg <= 96
        inf = sig_inf or [0] * n

        def rec(pt, flag):
            w = R.affine_entry(2, pt, upper=upper)
            if flag:
                w[48] = 1
            return w
        s = _u32([rec(p, f) for p, f in zip(sig, inf)] or [[0] * 52])
        a = _u32([rec(p, 0) for p in agg] or [[0] * 52])
        sst = np.array(list(sig_st if sig_st is not None else [0] * n) or [0], dtype=np.uint8)
        ast = np.array(list(agg_st if agg_st is not None else [0] * n_agg) or [0], dtype=np.uint8)
        c = _u32([list(ab) for ab in coef])
        ig = _u32(list(igrp) or [0])
        g = np.array(gst, dtype=np.uint8)
        out = np.zeros(72, dtype=np.uint32)
        _ok(self.lib.db_msm(n, n_agg, len(gst), s.ctypes.data_as(U32P), sst.ctypes.data_as(U8P), a.ctypes.data_as(U32P),
                            ast.ctypes.data_as(U8P), c.ctypes.data_as(U32P), ig.ctypes.data_as(U32P),
                            g.ctypes.data_as(U8P), out.ctypes.data_as(U32P)), "db_msm")
        return R.entry_affine(2, [int(v) for v in out])


@pytest.fixture(scope="module")
def cv():
    """The curve harness, loaded only if it was built from this tree (its embedded id); otherwise
    built now, and a failure of that fails the tests."""
    from gpu_helpers import harness
    return Curve(harness.load_devblocks("curve"))


@pytest.fixture(scope="module")
def torsion():
    return R.load_torsion()


def _subgroup_point(field, k):
    return R.ec_mul(field, B.G1_GEN if field == 1 else B.G2_GEN, k)


# ---- zero test and reductions ----------------------------------------------------------------
KMAX = ((1 << 392) - 1) // P


def _borrowed(rng, l):
    """the same value with limb j + 2^28 and limb j + 1 less one (what a limb-wise sum leaves)"""
    j = rng.randrange(13)
    if l[j + 1] == 0:
        return None
    l2 = list(l)
    l2[j] += 1 << 28
    l2[j + 1] -= 1
    return l2


def _zero_test_values():
    rng = random.Random(3901)
    ks = list(range(65)) + [100, 1000, 1 << 11, KMAX // 2, KMAX - 1, KMAX]
    vals = []
    for k in ks:
        ds = [0, 1, -1, 1 << 336, -(1 << 336), 1 << 200, rng.randrange(1, 1 << 300)]
        ds += [1 << (28 * j) for j in (3, 7, 12, 13)] + [-(1 << (28 * j)) for j in (5, 13)]  # one limb changed
        vals += [k * P + d for d in ds]
        # next to (k + 1/2) p: the estimate rounds to k or to k + 1, the value is no multiple either way
        vals += [k * P + P // 2 + d for d in (0, 1, -1, 1 << 336, -(1 << 336))]
    vals += [rng.randrange(1 << 392) for _ in range(100)]
    return [v for v in vals if 0 <= v < (1 << 392)]


def test_zero_test_on_device(cv):
    """l_is_zero (l_norm + l_is_zero_n) on k p for every k <= 64 and up to the largest k p below
    2^392, each +- 1, with one limb changed, next to (k + 1/2) p, in carried and uncarried layouts,
    and on the very limbs the formulas test: H = U2 + K - X1 of two representatives of one x."""
    rng = random.Random(3902)
    cases, want = [], []
    for v in _zero_test_values():
        l = R.limbs(v)
        for lay in (l, _borrowed(rng, l)):
            if lay is not None:
                cases.append((lay, [0] * 14))
                want.append(v % P == 0)
    for site, vmax in (("1A_H", lazy28.VMAX["Fp"]), ("2A_H", lazy28.VMAX["Fp2"]), ("2J_H", 2)):
        kdom = R.sub_kmax(site, vmax)  # the subtrahends x + j p that the site's K dominates
        for j in range(0 if kdom is None else kdom + 1):
            x = rng.randrange(P)
            for d in (0, 1):
                cases.append((R.l_sub(R.limbs(x + d), R.limbs(x + j * P), site), [0] * 14))
                want.append(d == 0)
    assert sum(want) > 120 and len(want) - sum(want) > 1000
    _, flags = cv.scalar("is_zero", cases)
    bad = [(i, R.lvalue(cases[i][0]) // P) for i in range(len(cases)) if bool(flags[i]) != want[i]]
    assert not bad, f"l_is_zero wrong on {len(bad)} of {len(cases)} inputs, (case, k): {bad[:8]}"


def test_f2_zero_test_on_device(cv):
    rng = random.Random(3903)
    zs = [R.limbs(k * P) for k in (0, 1, 2, 19, 37, KMAX)]
    nz = [R.limbs(k * P + d) for k in (0, 1, 36) for d in (1, P - 1, 1 << 364)]
    cases = [(a, b) for a in zs for b in zs] + [(a, b) for a in zs for b in nz] + [(b, a) for a in zs for b in nz] + \
        [(a, b) for a in nz[:3] for b in nz[:3]]
    cases.append((R.limbs(rng.randrange(1 << 392)), R.limbs(0)))
    _, flags = cv.scalar("f2_is_zero", cases)
    for (a, b), f in zip(cases, flags):
        assert bool(f) == (R.lvalue(a) % P == 0 and R.lvalue(b) % P == 0), (a, b)


def test_red_and_norm_on_device(cv):
    """l_red: the same residue, normalised, below 2p, for values on both sides of q p and (q + 1) p,
    the extremes of its range (0, 2^390 - 1, every limb 2^32 - 1) and uncarried layouts; l_norm: the
    same VALUE with limbs 0..12 below 2^28 -- so both return the same residue."""
    rng = random.Random(3904)
    top = 1 << 390
    qmax = (top - 1) // P
    vals = [0, 1, top - 1, top - 2, qmax * P, qmax * P - 1, qmax * P + 1]
    for q in (0, 1, 2, 3, 17, 36, 113, 500, qmax - 1):
        vals += [q * P + d for d in (-1, 0, 1, P // 2, P - 1, P, P + 1) if 0 <= q * P + d < top]
    vals += [rng.randrange(top) for _ in range(60)]
    lays = []
    for v in vals:
        l = R.limbs(v)
        lays.append(l)
        b = _borrowed(rng, l)
        if b:
            lays.append(b)
    full = [0xFFFFFFFF] * 13
    low = R.lvalue(full + [0])
    lays.append(full + [(top - 1 - low) >> 364])      # l_red's extreme: every limb 2^32 - 1
    red_in = list(lays)
    near = [0xFFFFFFEF] * 13                           # l_norm's: the carries reach 2^32 - 2, no further
    lazy28.norm(lazy28.Bound(near + [0], R.lvalue(near + [0]) + 1))
    norm_in = [l for l in lays if all(x < (1 << 32) - 16 for x in l)] + [near + [0]]
    assert all(R.lvalue(l) < top and max(l) < (1 << 32) for l in red_in)
    out, _ = cv.scalar("red", [(l, [0] * 14) for l in red_in])
    for l, r in zip(red_in, out):
        v, w = R.lvalue(l), R.lvalue(r)
        assert all(x <= R.M28 for x in r[:13]) and w < 2 * P and w % P == v % P, (l, r)
    out, _ = cv.scalar("norm", [(l, [0] * 14) for l in norm_in])
    for l, r in zip(norm_in, out):
        assert all(x <= R.M28 for x in r[:13]) and r[13] < (1 << 32) and R.lvalue(r) == R.lvalue(l), (l, r)


# ---- point operations --------------------------------------------------------------------------
def _point_cases(field, torsion):
    """[(name, P, Q)] group elements: generic, doubling, inverse, infinity on either side, and a
    torsion point of order 3 (G1) / 13 (G2) whose multiples meet each other"""
    q = 3 if field == 1 else 13
    T = next(pt for kind, qq, _, pt in torsion[field] if kind == "T" and qq == q)
    A, Bp = _subgroup_point(field, 0x1234567), _subgroup_point(field, 0x7654321)
    neg = lambda a: R.ec_neg(field, a)  # noqa: E731
    mul = lambda a, k: R.ec_mul(field, a, k)  # noqa: E731
    cases = [("generic", A, Bp), ("same", A, A), ("inverse", A, neg(A)), ("inf+P", None, A), ("P+inf", A, None),
             ("inf+inf", None, None), ("T+T", T, T), ("T+(-T)", T, neg(T)), ("T+2T", T, mul(T, 2)),
             ("2T+2T", mul(T, 2), mul(T, 2)), ("T+(q-1)T", T, mul(T, q - 1)), ("(q-1)/2 T + (q+1)/2 T", mul(T, q // 2), mul(T, q // 2 + 1)),
             ("A+T", A, T), ("(A+T)+(A+T)", R.ec_add(field, A, T), R.ec_add(field, A, T)),
             ("(A+T)+(-A)", R.ec_add(field, A, T), neg(A))]
    assert mul(T, q) is None
    return cases


def _reps(field, rng, pt, lazy, affine=False):
    """raw representatives of one group element: Z = 1 and Z random, at the low and the high end of
    the admitted range (lazy: + k p up to VMAX - 1, an affine operand + p; stored: + p), and mixed"""
    F = R.FIELD_OPS[field]
    kmax = (lazy28.VMAX["Fp" if field == 1 else "Fp2"] - 1) if lazy and not affine else 1
    out = []
    for lam in ([F.one] if affine or pt is None else [F.one, R.frand(field, rng), R.frand(field, rng)]):
        co = R.jac_coords(field, pt, lam)
        for ks in (0, kmax, [rng.randrange(kmax + 1) for _ in range(6)]):
            out.append((R.raw_slots(field, co, ks), pt is None))
    return out


def _check_lanes(field, lanes, lazy, want, what, vmax=None):
    first = lanes[0][0]
    for rec, _ in lanes:
        assert (rec == first).all(), f"{what}: the lanes of a pair hold different words"
    slots, inf, normalised = R.unpack_point(first, lazy)
    got = R.affine_of(field, slots, inf)
    assert got == want, f"{what}: got {got}, want {want}"
    if lazy and not inf:
        assert normalised and all(v < vmax * P for v in slots), f"{what}: result outside the ladders' invariant"
    if got is not None:
        assert B.ec_is_on_curve(got, R.FIELD_OPS[field], R.CURVE_B[field])


@pytest.mark.parametrize("field", [1, 2])
@pytest.mark.parametrize("mode", [ONE, HALF], ids=["one", "half"])
def test_lazy_point_ops(cv, torsion, field, mode):
    """g?l_dbl, g?l_madd, g?l_add on every case of _point_cases in several representatives each
    (so that H and rr are nonzero multiples of p in limbs, never equal words), one lane per case
    and one lane pair per case (G1Half / F2Half): the oracle's sum, inside the ladders' invariant."""
    rng = random.Random(3910 + 10 * field + mode)
    vmax = lazy28.VMAX["Fp" if field == 1 else "Fp2"]
    for op in ("l_dbl", "l_madd", "l_add"):
        cases, wants, names = [], [], []
        for name, a, b in _point_cases(field, torsion):
            if op == "l_madd" and b is None:
                continue  # the affine operand of a mixed addition is finite
            ra, rb = _reps(field, rng, a, True), _reps(field, rng, b, True, affine=op == "l_madd")
            n = max(len(ra), len(rb)) if op != "l_dbl" else len(ra)
            for i in range(n):
                pa, pb = ra[i % len(ra)], rb[(i * 2 + 1) % len(rb)]
                cases.append((R.pack_point(pa[0], pa[1], True), R.pack_point(pb[0], pb[1], True)))
                wants.append(R.ec_add(field, a, a if op == "l_dbl" else b))
                names.append(f"{op}/{name}#{i}")
        for lanes, want, name in zip(cv.point(field, mode, op, cases), wants, names):
            _check_lanes(field, lanes, True, want, name, vmax)


@pytest.mark.parametrize("field", [1, 2])
def test_stored_point_ops(cv, torsion, field):
    """jac_dbl, jac_add, jac_add_aff and jac_eq on the same cases, operands at both ends of the
    stored range (below p, and p and above), infinity as Z = 0 and as Z = p"""
    rng = random.Random(3930 + field)
    F = R.FIELD_OPS[field]
    for op in ("j_dbl", "j_add", "j_add_aff"):
        cases, wants, names = [], [], []
        for name, a, b in _point_cases(field, torsion):
            ra, rb = _reps(field, rng, a, False), _reps(field, rng, b, False, affine=op == "j_add_aff")
            for i in range(max(len(ra), len(rb))):
                pa, pb = ra[i % len(ra)], rb[(i * 2 + 1) % len(rb)]
                cases.append((R.pack_point(pa[0], False, False), R.pack_point(pb[0], pb[1] and op == "j_add_aff", False)))
                wants.append(R.ec_add(field, a, a if op == "j_dbl" else b))
                names.append(f"{op}/{name}#{i}")
        for lanes, want, name in zip(cv.point(field, ONE, op, cases), wants, names):
            _check_lanes(field, lanes, False, want, name)
    A, Bp = _subgroup_point(field, 99), _subgroup_point(field, 100)
    T = torsion[field][0][3]
    eq = [(A, A, True), (A, R.ec_neg(field, A), False), (A, Bp, False), (None, A, False), (A, None, False),
          (None, None, True), (T, T, True), (T, R.ec_neg(field, T), False)]
    cases, wants = [], []
    for a, b, w in eq:
        ra, rb = _reps(field, rng, a, False), _reps(field, rng, b, False)
        for i in range(max(len(ra), len(rb))):
            pa, pb = ra[i % len(ra)], rb[(i * 4 + 1) % len(rb)]
            cases.append((R.pack_point(pa[0], False, False), R.pack_point(pb[0], False, False)))
            wants.append(w)
    for lanes, w, c in zip(cv.point(field, ONE, "j_eq", cases), wants, range(len(cases))):
        assert bool(lanes[0][1]) == w, c


@pytest.mark.parametrize("field", [1, 2])
def test_lazy_stored_round_trips(cv, torsion, field):
    """g?l_to_jac returns the same group element in stored words below 2p (infinity for the flag,
    whatever the limbs hold); g2l_from_jac returns it in limbs, flagged exactly when Z = 0 mod p"""
    rng = random.Random(3940 + field)
    pts = [_subgroup_point(field, 5), torsion[field][0][3], torsion[field][5][3], None]
    cases, wants = [], []
    for pt in pts:
        for sl, inf in _reps(field, rng, pt, True):
            cases.append((R.pack_point(sl, inf, True), R.pack_point([0] * 6, True, True)))
            wants.append(pt)
    junk = R.raw_slots(field, R.jac_coords(field, pts[0], R.FIELD_OPS[field].one), 3)
    cases.append((R.pack_point(junk, True, True), R.pack_point([0] * 6, True, True)))  # flagged: infinity
    wants.append(None)
    for lanes, want in zip(cv.point(field, ONE, "l_tojac", cases), wants):
        slots, _, _ = R.unpack_point(lanes[0][0], False)
        assert all(v < 2 * P for v in slots) and R.affine_of(field, slots) == want
    if field == 2:
        cases, wants = [], []
        for pt in pts:
            for sl, _ in _reps(field, rng, pt, False):
                cases.append((R.pack_point(sl, False, False), R.pack_point([0] * 6, False, False)))
                wants.append(pt)
        for lanes, want in zip(cv.point(2, ONE, "l_fromjac", cases), wants):
            slots, inf, normalised = R.unpack_point(lanes[0][0], True)
            assert normalised and inf == (want is None) and R.affine_of(2, slots, inf) == want


# ---- ladders and subgroup tests ------------------------------------------------------------------
@pytest.fixture(scope="module")
def ladder_points(torsion):
    """{field: [(name, group element, oracle's in_subgroup)]}: every fixture point, the generator,
    a random subgroup point, infinity -- the oracle's verdicts computed once"""
    out = {}
    for field, insub, gen in ((1, B.g1_in_subgroup, B.G1_GEN), (2, B.g2_in_subgroup, B.G2_GEN)):
        pts = [(f"{kind}/q={str(q)[:8]}", pt) for kind, q, _, pt in torsion[field]]
        pts += [("generator", gen), ("subgroup", _subgroup_point(field, random.Random(3950).randrange(1, B.R))), ("infinity", None)]
        out[field] = [(name, pt, insub(pt)) for name, pt in pts]
        assert sum(1 for _, _, v in out[field] if v) == 3
    return out


@pytest.mark.parametrize("field,mode", [(1, ONE), (1, HALF), (2, ONE), (2, HALF)], ids=["g1", "g1-half", "g2", "g2-half"])
def test_subgroup_verdicts(cv, ladder_points, field, mode):
    """g1_in_subgroup28 / g2_in_subgroup28_l, one lane and one lane pair per point, equal the
    oracle's [r] P == O on points of every small order (where the ladder meets R = +-T and R = O)"""
    pts = ladder_points[field]
    ent = [R.affine_entry(field, pt, upper=(i % 3 == 1)) for i, (_, pt, _) in enumerate(pts)]
    for (name, _, want), lanes in zip(pts, cv.ladder(field, mode, LD_SUB, ent)):
        assert [bool(f) for _, f in lanes] == [want] * len(lanes), name


@pytest.mark.parametrize("mode", [ONE, HALF], ids=["one", "half"])
def test_g2_xabs_ladder(cv, ladder_points, mode):
    """g2l_mul_by_xabs_l returns [|x|] P as a group element, infinity included, for P in Jacobian
    form with Z = 1 and Z random"""
    rng = random.Random(3960 + mode)
    pts = ladder_points[2]
    ent = [R.jac_entry(2, pt, None if i % 2 else R.frand(2, rng), upper=(i % 3 == 0)) for i, (_, pt, _) in enumerate(pts)]
    for (name, pt, _), lanes in zip(pts, cv.ladder(2, mode, LD_MUL, ent)):
        assert lanes[0][0] == lanes[-1][0], name
        assert R.entry_affine(2, lanes[0][0]) == B.g2_mul(pt, X_ABS), name


def test_g1_x2_ladder(cv, ladder_points):
    """[x^2] P from ec.h's stored-word ladders (jac_mul_by_xabs_aff, jac_mul_by_xabs), infinity included"""
    pts = ladder_points[1]
    ent = [R.affine_entry(1, pt, upper=(i % 2 == 1)) for i, (_, pt, _) in enumerate(pts)]
    for (name, pt, _), lanes in zip(pts, cv.ladder(1, ONE, LD_MUL, ent)):
        assert R.entry_affine(1, lanes[0][0]) == B.g1_mul(pt, X_ABS * X_ABS), name


_LAM = {}


def _lam_image(field, p):
    """[lambda] p, what the product's tables hold as T2 (the endomorphism's image), by the oracle"""
    if (field, p) not in _LAM:
        _LAM[(field, p)] = R.ec_mul(field, p, LAMBDA)
        _LAM[(field, R.ec_neg(field, p))] = R.ec_neg(field, _LAM[(field, p)])
    return _LAM[(field, p)]


def _chunk_plan(field, torsion):
    """[(name, [(T1, T2)], [(a, b)])]: the exceptional chunks tests/test_lazy28.py lists for the g++
    build (the ladder meets T, a sum at infinity, all-ones and zero coefficients), a chunk of one
    point only, and one holding a torsion point and its negative"""
    rng = random.Random(3970 + field)
    K = [_subgroup_point(field, rng.randrange(1, B.R)) for _ in range(3)]
    q = 3 if field == 1 else 13
    T = next(pt for kind, qq, _, pt in torsion[field] if kind == "T" and qq == q)
    lam = lambda p: _lam_image(field, p)  # noqa: E731
    neg = lambda p: R.ec_neg(field, p)  # noqa: E731
    r32 = lambda: (rng.getrandbits(32), rng.getrandbits(32))  # noqa: E731
    return [
        ("random", [(K[0], lam(K[0])), (K[1], lam(K[1])), (K[2], lam(K[2]))], [r32(), r32(), r32()]),
        ("meets T", [(K[0], lam(K[0]))] * 4, [(1, 0), (1, 0), (0xFFFFFFFF, 0), (0, 1)]),
        ("infinity", [(K[1], lam(K[1])), (neg(K[1]), lam(neg(K[1])))], [(5, 0), (5, 0)]),
        ("all ones", [(K[2], lam(K[2]))] * 3, [(0xFFFFFFFF, 0xFFFFFFFF)] * 3),
        ("zero coefficient", [(K[0], lam(K[0])), (K[1], lam(K[1])), (K[2], lam(K[2]))], [r32(), (0, 0), r32()]),
        ("one point", [(K[1], lam(K[1]))] * 5, [r32() for _ in range(5)]),
        ("T and -T", [(T, K[0]), (neg(T), K[1]), (T, K[2])], [r32(), r32(), (3, 1)]),
        ("T and -T cancel", [(T, K[0]), (neg(T), neg(K[0]))], [(7, 9), (7, 9)]),
    ]


@pytest.mark.parametrize("field", [1, 2])
def test_dense_chunk_ladders(cv, torsion, field):
    """g1l_msm_ladder / g2l_msm_ladder on explicit tables (T1, T2, T1 + T2) and coefficients: the
    sum [a_i] T_i1 + [b_i] T_i2 of every chunk, one lane each, as a group element"""
    tab, coef, ranges, wants, names = [], [], [], [], []
    for name, pairs, ab in _chunk_plan(field, torsion):
        ranges.append((len(tab), len(pairs)))
        want = None
        for (t1, t2), (a, b) in zip(pairs, ab):
            tab.append((t1, t2, R.ec_add(field, t1, t2)))
            assert tab[-1][2] is not None  # a table holds finite points only
            coef.append((a, b))
            want = R.ec_add(field, want, R.ec_add(field, R.ec_mul(field, t1, a), R.ec_mul(field, t2, b)))
        wants.append(want)
        names.append(name)
    ranges.append((0, len(tab)))  # and one lane over the whole table
    total = None
    for (first, cnt), w in zip(ranges[:-1], wants):
        total = R.ec_add(field, total, w)
    wants.append(total)
    names.append("everything")
    assert None in wants
    for got, want, name in zip(cv.chunk(field, False, tab, coef, ranges), wants, names):
        assert got == want, name


def _sparse_record(digits, usable=True):
    w = [0, 0, 0, 1 if usable else 0]
    for j, v in enumerate(digits):
        w[j // 10] |= v << (3 * (j % 10))
    A = Bv = 0
    for j, v in enumerate(digits):
        u, x = [(1, 0), (0, 1), (1, 1), (1, -1)][v & 3]
        if v & 4:
            u, x = -u, -x
        A, Bv = A + u * 4 ** j, Bv + x * 4 ** j
    return w, ((A, Bv) if usable else (0, 0))


@pytest.mark.parametrize("field", [1, 2])
def test_sparse_chunk_ladders(cv, torsion, field):
    """g1l/g2l_msm_ladder_sparse on explicit tables (T1, T2, T1 + T2, T1 - T2) and digit records
    (ec28.h RLC_DIGITS): random digits, the extreme strings, a skipped item, one point repeated
    (the ladder meets T: a doubling; and T then -T: infinity), and a torsion point with its negative"""
    rng = random.Random(3980 + field)
    K = [_subgroup_point(field, rng.randrange(1, B.R)) for _ in range(3)]
    T = next(pt for kind, qq, _, pt in torsion[field] if kind == "T" and qq == (3 if field == 1 else 13))
    lam = lambda p: _lam_image(field, p)  # noqa: E731
    neg = lambda p: R.ec_neg(field, p)  # noqa: E731
    rd = lambda: [rng.randrange(8) for _ in range(22)]  # noqa: E731
    plan = [("random", [(K[0], lam(K[0])), (K[1], lam(K[1])), (K[2], lam(K[2]))], [rd(), rd(), rd()], [1, 1, 1]),
            ("extremes", [(K[0], lam(K[0])), (K[1], lam(K[1])), (K[2], lam(K[2]))], [[2] * 22, [7] * 22, rd()], [1, 1, 0]),
            ("one point", [(K[1], lam(K[1]))] * 4, [rd(), rd(), [0] * 22, [4] * 22], [1] * 4),
            ("meets T", [(K[0], lam(K[0]))] * 2, [[0] * 22, [0] * 22], [1, 1]),  # top digit: K + K, a doubling
            ("cancels", [(K[2], lam(K[2]))] * 2, [[0] * 22, [4] * 22], [1, 1]),
            ("T and -T", [(T, K[0]), (neg(T), K[1]), (T, K[2])], [rd(), rd(), [0] * 22], [1, 1, 1])]
    tab, coef, ranges, wants, names = [], [], [], [], []
    for name, pairs, digits, usable in plan:
        ranges.append((len(tab), len(pairs)))
        want = None
        for (t1, t2), d, u in zip(pairs, digits, usable):
            tab.append((t1, t2, R.ec_add(field, t1, t2), R.ec_add(field, t1, neg(t2))))
            assert tab[-1][2] is not None and tab[-1][3] is not None
            w, (a, b) = _sparse_record(d, bool(u))
            coef.append(w)
            want = R.ec_add(field, want, R.ec_add(field, R.ec_mul(field, t1, a), R.ec_mul(field, t2, b)))
        wants.append(want)
        names.append(name)
    assert None in wants
    for got, want, name in zip(cv.chunk(field, True, tab, coef, ranges), wants, names):
        assert got == want, name


# ---- the slot-wide bucket MSM ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def msm_pool():
    """signatures s_i = [m_i] Q_j for small m_i over two base points of G2, and the base points'
    -psi^2 images: by linearity S = sum_j [sum a_i m_i] Q_j + [sum b_i m_i] (-psi^2 Q_j), two
    oracle multiplications per base point (test_msm_random checks that against the term-by-term sum)"""
    rng = random.Random(3990)
    bases = [B.g2_mul(B.G2_GEN, rng.randrange(1, B.R)) for _ in range(2)]
    images = [B.g2_neg(B.g2_psi(B.g2_psi(q))) for q in bases]
    return bases, images


class _Msm:
    """one MSM input under construction: items as (base index, multiplier), the sum kept in scalars"""

    def __init__(self, pool, g_ready):
        self.bases, self.images = pool
        self.ready = g_ready
        self.sig, self.coef, self.igrp, self.sig_st, self.sig_inf = [], [], [], [], []
        self.agg, self.agg_coef, self.agg_st, self.gst = [], [], [], []
        self.sa, self.sb = [0, 0], [0, 0]
        self._g, self._cache = [], {}

    def pt(self, j, m):
        if m < 0:
            return B.g2_neg(self.pt(j, -m))
        if (j, m) not in self._cache:
            self._cache[(j, m)] = B.g2_mul(self.bases[j], m)
        return self._cache[(j, m)]

    def add(self, j, m, a, b, st=0, inf=0, gst=None, agg=False, counted=True):
        """item [m] Q_j with coefficients (a, b) in a group of its own (state gst, default READY)"""
        g = self.ready if gst is None else gst
        if agg:
            self.agg.append(self.pt(j, m))
            self.agg_coef.append((a, b))
            self.agg_st.append(st)
        else:
            self.sig.append(self.pt(j, m))
            self.coef.append((a, b))
            self.sig_st.append(st)
            self.sig_inf.append(inf)
        self._g.append((agg, g))
        if counted:
            assert st == 0 and inf == 0 and g == self.ready and (a | b)
            self.sa[j] = (self.sa[j] + a * m) % B.R
            self.sb[j] = (self.sb[j] + b * m) % B.R

    def run(self, cv, upper=False):
        # groups: the folded aggregates are groups 0 .. n_agg - 1, every item a group after them
        agg_g = [g for is_agg, g in self._g if is_agg]
        item_g = [g for is_agg, g in self._g if not is_agg]
        gst = agg_g + item_g
        igrp = [len(agg_g) + i for i in range(len(item_g))]
        return cv.msm(self.sig, self.coef + self.agg_coef, igrp, gst, self.sig_st, self.agg, self.agg_st, self.sig_inf,
                      upper=upper)

    def want(self):
        total = None
        for j in range(2):
            total = B.g2_add(total, B.g2_add(B.g2_mul(self.bases[j], self.sa[j]), B.g2_mul(self.images[j], self.sb[j])))
        return total


def _w(d1, d0):
    return (d1 << 16) | d0


def test_msm_random(cv, msm_pool):
    """1. random 32-bit coefficients; the linear reference equals the oracle's term-by-term sum"""
    rng = random.Random(4001)
    m = _Msm(msm_pool, cv.g_ready)
    for i in range(10):
        m.add(i & 1, rng.randrange(1, 1 << 16), rng.getrandbits(32), rng.getrandbits(32))
    want = m.want()
    assert want == R.msm_reference(m.sig, m.coef)
    assert m.run(cv) == want
    assert m.run(cv, upper=True) == want


def test_msm_one_bucket(cv, msm_pool):
    """2. every item with the same digit in both windows: the bucket's sum passes through a
    doubling (one point three times) and through infinity (a point and its negative) and goes on"""
    for d in (0x0001, 0x5A5A, 0xFFFF):
        m = _Msm(msm_pool, cv.g_ready)
        for j, mult in ((0, 7), (0, 7), (0, 7), (1, 11), (1, -11), (1, 5), (0, 7), (0, -7), (1, 123)):
            m.add(j, mult, _w(d, d), 0)
        assert m.run(cv) == m.want(), hex(d)
    m = _Msm(msm_pool, cv.g_ready)  # the same in half 1: the images double and cancel
    for j, mult in ((0, 7), (0, 7), (0, -7), (0, -7), (0, 7), (1, 3)):
        m.add(j, mult, 0, _w(9, 9))
    assert m.run(cv) == m.want()
    m = _Msm(msm_pool, cv.g_ready)  # a bucket that ends at infinity beside one that does not
    for j, mult, a in ((0, 7, _w(9, 9)), (0, -7, _w(9, 9)), (1, 3, _w(9, 10))):
        m.add(j, mult, a, 0)
    assert m.run(cv) == m.want()


def test_msm_digit_extremes(cv, msm_pool):
    """3. digits exactly 1 and 0xFFFF in each window, in each half"""
    m = _Msm(msm_pool, cv.g_ready)
    k = 0
    for a in (_w(0, 1), _w(1, 0), _w(0, 0xFFFF), _w(0xFFFF, 0), _w(1, 1), _w(0xFFFF, 0xFFFF), _w(1, 0xFFFF), _w(0xFFFF, 1)):
        k += 1
        m.add(k & 1, 100 + k, a, 0)
        m.add(k & 1, 200 + k, 0, a)
        m.add(k & 1, 300 + k, a, a ^ 0xFFFFFFFF if a ^ 0xFFFFFFFF else 1)
    assert m.run(cv) == m.want()


@pytest.mark.parametrize("where", ["first", "last", "straddle", "mul16"])
def test_msm_chunk_extremes(cv, msm_pool, where):
    """4. k_msm_reduce's chunks of MSM_CHUNK buckets: only the first chunk (lo == 0, W = T - R), only
    the last, a chunk boundary, and the 16-bit multiples lo - 1 at their extremes and bit patterns"""
    c = cv.msm_chunk
    assert c >= 2
    digits = {"first": list(range(1, c)),
              "last": list(range(0x10000 - c, 0x10000)),
              "straddle": [c - 1, c, 0x8000 - 1, 0x8000, 0x10000 - c - 1, 0x10000 - c],
              "mul16": [c, c + 1, 2 * c, 0x5555, 0xAAAA, 0x8000 + c, 0xFF00, 0x00FF + c]}[where]
    for window in (0, 1, 2):  # 2: both
        m = _Msm(msm_pool, cv.g_ready)
        for i, d in enumerate(digits):
            a = _w(d, 0) if window == 1 else _w(0, d) if window == 0 else _w(d, d)
            m.add(i & 1, 40 + i, a, 0)
            if i % 2:
                m.add(i & 1, 90 + i, 0, a)
        assert m.run(cv) == m.want(), (where, window)


def test_msm_windows_and_halves(cv, msm_pool):
    """5. only window 0 populated, only window 1; 6. only b coefficients (the -psi^2 image), a == b"""
    rng = random.Random(4005)
    for kind in ("w0", "w1", "b only", "a == b"):
        m = _Msm(msm_pool, cv.g_ready)
        for i in range(8):
            d = rng.randrange(1, 1 << 16)
            full = rng.getrandbits(32) | 1
            a, b = {"w0": (d, d ^ 0x1), "w1": (d << 16, (d ^ 0x3) << 16), "b only": (0, full), "a == b": (full, full)}[kind]
            m.add(i & 1, rng.randrange(1, 1 << 12), a, b)
        assert m.run(cv) == m.want(), kind


def test_msm_filters(cv, msm_pool):
    """7. what must not enter: a (0, 0) coefficient, a nonzero sig_st / agg_st, a set inf flag, a
    group that is not G_READY (the value read from layout.h through the harness); 8. nothing left"""
    rng = random.Random(4007)
    not_ready = [v for v in range(3) if v != cv.g_ready]
    for keep in (True, False):
        m = _Msm(msm_pool, cv.g_ready)
        r32 = lambda: rng.getrandbits(32) | 1  # noqa: E731
        for rep in range(2):
            if keep:
                m.add(0, 3 + rep, r32(), r32())
            m.add(1, 5, 0, 0, counted=False)
            m.add(0, 6, r32(), r32(), st=1 + rep, counted=False)
            m.add(1, 7, r32(), r32(), inf=1, counted=False)
            m.add(0, 8, r32(), r32(), gst=not_ready[rep], counted=False)
            m.add(1, 9, r32(), r32(), st=2, agg=True, counted=False)
            m.add(0, 10, r32(), r32(), gst=not_ready[rep], agg=True, counted=False)
            m.add(1, 11, 0, 0, agg=True, counted=False)
            if keep:
                m.add(1, 12 + rep, r32(), r32(), agg=True)
        want = m.want()
        assert (want is None) == (not keep)
        assert m.run(cv) == want, keep


def test_msm_with_aggregates(cv, msm_pool):
    """9. folded aggregates (n_agg > 0) mixed with items, sharing buckets with them"""
    rng = random.Random(4009)
    m = _Msm(msm_pool, cv.g_ready)
    for i in range(12):
        a = rng.getrandbits(32) if i % 3 else _w(0x77, 0x77)
        m.add(i & 1, rng.randrange(1, 1 << 12), a, rng.getrandbits(32), agg=(i % 2 == 0))
    assert m.run(cv) == m.want()


def test_msm_total_is_infinity(cv, msm_pool):
    """10. a set whose total is infinity: inside one bucket, and across different buckets"""
    m = _Msm(msm_pool, cv.g_ready)
    m.add(0, 5, _w(3, 10), _w(7, 0))
    m.add(0, -5, _w(3, 10), _w(7, 0))
    m.add(1, 6, 2 * 0x1234, 0)      # [2 c] (6 Q) - [c] (12 Q) = O across different buckets
    m.add(1, -12, 0x1234, 0)
    assert m.want() is None
    assert m.run(cv) is None


# ---- the same points through the C ABI ----------------------------------------------------------------
# Expected statuses and bytes come from the oracle (verify, aggregate, threshold_aggregate,
# verify_aggregate, the decompressors); its decompressions are memoised for the module, so that each
# fixture point's [r] P is computed once.
from charon_amd import _lib  # noqa: E402

HELPERS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_helpers")


@pytest.fixture(scope="module")
def L(hipbls):
    return _lib.load_library()


@pytest.fixture(scope="module")
def oracle_memo():
    """oracle.bls12381 with g1_decompress / g2_decompress memoised (results and DecodeErrors)"""
    saved = B.g1_decompress, B.g2_decompress

    def memo(fn):
        seen = {}

        def wrapped(b, subgroup_check=True):
            key = (bytes(b), subgroup_check)
            if key not in seen:
                try:
                    seen[key] = (fn(b, subgroup_check), None)
                except B.DecodeError as e:
                    seen[key] = (None, e)
            val, err = seen[key]
            if err is not None:
                raise B.DecodeError(str(err))
            return val
        return wrapped
    B.g1_decompress, B.g2_decompress = memo(saved[0]), memo(saved[1])
    yield B
    B.g1_decompress, B.g2_decompress = saved


@pytest.fixture(scope="module")
def fixture_bytes():
    import json
    doc = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "torsion_points.json")))
    return {g: [bytes.fromhex(e["point"]) for e in doc[g]["points"]] for g in ("g1", "g2")}


@pytest.fixture(scope="module")
def valid(hipbls, kats):
    """valid (pk, msg, sig) triples: the reference's KATs"""
    vecs = [kats["registration"]] + kats["deposit"]
    return [(hipbls.secret_to_public_key(bytes.fromhex(v["sk"])), bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"]))
            for v in vecs]


def _interleave(valid, bad_items):
    """valid and bad items alternating (so that waves are mixed), valid ones first and last"""
    items, kinds = [], []
    for i, b in enumerate(bad_items):
        items += [valid[i % len(valid)], b]
        kinds += [True, False]
    return items + [valid[0]], kinds + [True]


@pytest.mark.parametrize("pair_max", [0, 1 << 30], ids=["one-lane", "lane-pair"])
def test_abi_torsion_keys_and_signatures_verify(L, hipbls, oracle_memo, fixture_bytes, valid, pair_max):
    """hbls_verify_batch: every G1 fixture point as a public key is BAD_PUBKEY, every G2 fixture
    point as a signature BAD_SIGNATURE (the oracle's statuses), between valid items, with the
    subgroup ladders one lane per item (k_g1_subgroup, k_g2_subgroup) and split over lane pairs
    (k_g1_subgroup_h, k_g2_subgroup_h: hbls_dec_pair_max raised)"""
    pk0, m0, s0 = valid[0]
    bad = [(k, m0, s0) for k in fixture_bytes["g1"]] + [(pk0, m0, s) for s in fixture_bytes["g2"]]
    items, kinds = _interleave(valid, bad)
    want = [B.ST_OK if ok else oracle_memo.verify(*it) for it, ok in zip(items, kinds)]
    n1 = len(fixture_bytes["g1"])
    assert want.count(B.ST_BAD_PUBKEY) == n1 and want.count(B.ST_BAD_SIGNATURE) == len(fixture_bytes["g2"])
    prev = L.hbls_dec_pair_max(pair_max)
    try:
        got = hipbls.verify_batch(*zip(*items))
    finally:
        L.hbls_dec_pair_max(prev)
    assert got == want


def test_abi_torsion_keys_decompress_device(L, hipbls, oracle_memo, fixture_bytes, valid):
    """hbls_decompress_pubkeys_device: the table's status is BAD_PUBKEY for every G1 fixture point"""
    import torch
    keys, kinds = _interleave([v[0] for v in valid], fixture_bytes["g1"])
    want = []
    for k, ok in zip(keys, kinds):
        try:
            oracle_memo.g1_decompress(k)
            want.append(B.ST_OK)
        except B.DecodeError:
            want.append(B.ST_BAD_PUBKEY)
    assert [w == B.ST_OK for w in want] == kinds
    dev = torch.device("cuda", 0)
    n = len(keys)
    src = torch.from_numpy(np.frombuffer(b"".join(keys), dtype=np.uint8).copy()).to(dev)
    tab = torch.zeros(n * L.hbls_pk_entry_bytes(), dtype=torch.uint8, device=dev)
    st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(device=dev)
    rc = L.hbls_decompress_pubkeys_device(ctypes.c_void_p(src.data_ptr()), n, ctypes.c_void_p(tab.data_ptr()),
                                          ctypes.c_void_p(st.data_ptr()), ctypes.c_void_p(s.cuda_stream))
    assert rc == 0, L.hbls_last_error().decode()
    s.synchronize()
    assert list(st.cpu().numpy()) == want


@pytest.mark.parametrize("cap", [0, 64], ids=["learn-off", "learn-64"])
def test_abi_torsion_keys_slot_device(L, oracle_memo, fixture_bytes, cap):
    """hbls_slot_device on a small cluster with every G1 fixture point among the pubshares and the
    DV keys: BAD_PUBKEY for each (and a failed aggregate verification), with the learned key cache
    off, and cold and warm with a table smaller than the key set (the counters show which)"""
    if HELPERS not in sys.path:
        sys.path.insert(0, HELPERS)
    import key_learn_slot as ks
    d = ks.make_inputs(L)
    pks = d["pks"].reshape(-1, 48).copy()
    dv = d["dv_pks"].reshape(-1, 48).copy()
    bad = fixture_bytes["g1"]
    ndv = min(len(bad), d["V"] // 2)
    assert 5 * len(bad) < d["NP"]
    for j, kb in enumerate(bad):
        with pytest.raises(B.DecodeError):
            oracle_memo.g1_decompress(kb)
        pks[5 * j + 1] = np.frombuffer(kb, dtype=np.uint8)
        if j < ndv:
            dv[2 * j + 1] = np.frombuffer(kb, dtype=np.uint8)
    occurrences = d["NP"] + d["V"]
    prev = ks.tune(L, "HBLS_KEY_LEARN", cap)
    try:
        s0 = ks.stats(L)
        cold = ks.run_slots(L, d, pks=pks, dv_pks=dv)[0]
        s1 = ks.stats(L)
        warm = ks.run_slots(L, d, pks=pks, dv_pks=dv)[0]
        s2 = ks.stats(L)
    finally:
        ks.tune(L, "HBLS_KEY_LEARN", prev)
    for out in (cold, warm):
        vst, ast = np.frombuffer(out[0], dtype=np.uint8), np.frombuffer(out[2], dtype=np.uint8)
        badpos = {5 * j + 1 for j in range(len(bad))}
        assert all((vst[i] == _lib.BAD_PUBKEY) == (i in badpos) for i in range(d["NP"]))
        assert all(vst[i] == _lib.OK for i in range(d["NP"]) if i not in badpos)
        assert all((ast[v] == _lib.BAD_PUBKEY) == (v % 2 == 1 and v // 2 < ndv) for v in range(d["V"]))
    assert cold == warm
    if cap == 0:
        assert (s1["hits"], s1["misses"], s1["size"]) == (s0["hits"], s0["misses"], 0) and s2 == s1
    else:
        assert (s1["hits"] - s0["hits"], s1["misses"] - s0["misses"], s1["size"]) == (0, occurrences, cap)
        hits, misses = s2["hits"] - s1["hits"], s2["misses"] - s1["misses"]
        assert hits + misses == occurrences and hits >= 1 and s2["size"] == cap


def test_abi_torsion_signatures_in_aggregations(L, hipbls, oracle_memo, fixture_bytes, valid):
    """every G2 fixture point as a member of hbls_threshold_aggregate_batch and hbls_aggregate_batch
    groups: the oracle's group status, without the signature cache, and after a Verify put the
    points into it with their rejection status"""
    good = [v[2] for v in valid]
    bad = fixture_bytes["g2"]
    ta_groups, ag_groups = [{1: good[0], 2: good[1]}], [[good[0], good[1]]]
    for i, t in enumerate(bad):  # first, and for a few last (the oracle stops at the first bad member)
        ta_groups.append({1: t, 2: good[i % len(good)]} if i % 6 else {1: good[0], 2: good[1], 3: t})
        ag_groups.append([t, good[i % len(good)]] if i % 6 else [good[0], good[1], t])
    want_ta = [oracle_memo.threshold_aggregate(g) for g in ta_groups]
    want_ag = [oracle_memo.aggregate(g) for g in ag_groups]
    assert [w[0] for w in want_ta] == [B.ST_OK] + [B.ST_BAD_SIGNATURE] * len(bad)
    assert [w[0] for w in want_ag] == [B.ST_OK] + [B.ST_BAD_SIGNATURE] * len(bad)
    pk0, m0, _ = valid[0]

    def run():
        outs, sts = hipbls.threshold_aggregate_batch(ta_groups)
        assert sts == [w[0] for w in want_ta] and outs[0] == want_ta[0][1]
        outs, sts = hipbls.aggregate_batch(ag_groups)
        assert sts == [w[0] for w in want_ag] and outs[0] == want_ag[0][1]
    prev = L.hbls_sig_cache(0)
    try:
        run()
        L.hbls_sig_cache(1 << 12)
        st = hipbls.verify_batch([pk0] * len(bad) + [v[0] for v in valid], [m0] * len(bad) + [v[1] for v in valid],
                                 bad + good)
        assert st == [B.ST_BAD_SIGNATURE] * len(bad) + [B.ST_OK] * len(valid)
        run()
        run()
    finally:
        L.hbls_sig_cache(prev)


def _neg_sig(s):
    """the compressed negative of a finite point: the sign flag flipped"""
    assert s[0] & 0x80 and not s[0] & 0x40
    return bytes([s[0] ^ 0x20]) + s[1:]


@pytest.fixture(scope="module")
def degenerate(hipbls):
    """S = sign(k, m), [2] S, [3] S, another signature, and keys pk, -pk, pk2 -- inputs only (the
    oracle decodes the same bytes)"""
    m = b"degenerate sums"
    k = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA998877665544332211000123 % B.R
    sk = [B.sk_to_bytes(j * k) for j in (1, 2, 3)]
    S, S2, S3 = hipbls.sign_batch(sk, [m] * 3)
    k2 = B.sk_to_bytes(0x2468ACE)
    return dict(m=m, S=S, S2=S2, S3=S3, T=hipbls.sign(k2, b"another"), pk=hipbls.secret_to_public_key(sk[0]),
                pk2=hipbls.secret_to_public_key(k2), S_k2=hipbls.sign(k2, m))


def test_abi_degenerate_aggregates(hipbls, oracle_memo, degenerate, valid):
    """Aggregate of {s, s} (a doubling), {s, -s} (infinity), {s, s, -s}, {s, -s, t}: byte-exact
    with the oracle (the infinity encoding where the sum vanishes), alone and in a batch"""
    d = degenerate
    S, nS, T = d["S"], _neg_sig(d["S"]), d["T"]
    groups = [[S, S], [S, nS], [S, S, nS], [S, nS, T], [nS, S], [S, S, S, S]]
    want = [oracle_memo.aggregate(g) for g in groups]
    assert want[1] == (B.ST_OK, B.g2_compress(None)) and want[2] == (B.ST_OK, S) and want[3] == (B.ST_OK, T)
    for g, w in zip(groups, want):
        outs, sts = hipbls.aggregate_batch([g])
        assert (sts[0], outs[0]) == w
    ordinary = [[v[2] for v in valid[:k]] for k in (2, 3, 4)]
    mixed = [ordinary[0]] + groups[:3] + [ordinary[1]] + groups[3:] + [ordinary[2]]
    outs, sts = hipbls.aggregate_batch(mixed)
    assert list(zip(sts, outs)) == [oracle_memo.aggregate(g) for g in mixed]


def test_abi_degenerate_threshold_aggregates(hipbls, oracle_memo, degenerate, valid):
    """ThresholdAggregate over indices (1, 2) (coefficients 2, -1) of (S, S) -> S, (S, 2S) ->
    infinity, (S, -S) -> 3S, and 3-of-n sets over (1, 2, 3) (coefficients 3, -3, 1) that vanish:
    byte-exact with the oracle, alone and in a batch of ordinary groups"""
    d = degenerate
    S, S2, S3, nS = d["S"], d["S2"], d["S3"], _neg_sig(d["S"])
    groups = [{1: S, 2: S}, {1: S, 2: S2}, {1: S, 2: nS}, {1: S, 2: S2, 3: S3}, {1: S, 2: S, 3: S3},
              {1: S, 2: S, 3: S}, {2: S2, 1: S}]
    want = [oracle_memo.threshold_aggregate(g) for g in groups]
    inf = (B.ST_OK, B.g2_compress(None))
    assert want[0] == (B.ST_OK, S) and want[1] == inf and want[2] == (B.ST_OK, S3) and want[3] == inf
    assert want[5] == (B.ST_OK, S) and want[6] == inf
    for g, w in zip(groups, want):
        outs, sts = hipbls.threshold_aggregate_batch([g])
        assert (sts[0], outs[0]) == w, g.keys()
    good = [v[2] for v in valid]
    ordinary = [{1: good[0], 2: good[1]}, {2: good[1], 3: good[2], 5: good[3]}, {1: good[2], 4: good[0]}]
    mixed = [ordinary[0]] + groups[:4] + [ordinary[1]] + groups[4:] + [ordinary[2]]
    outs, sts = hipbls.threshold_aggregate_batch(mixed)
    assert list(zip(sts, outs)) == [oracle_memo.threshold_aggregate(g) for g in mixed]


def test_abi_verify_aggregate_cancelling_keys(hipbls, oracle_memo, degenerate, valid):
    """VerifyAggregate with keys {pk, -pk, pk2}: the key sum passes through infinity and is pk2
    (verified by pk2's signature); {pk, -pk} alone sums to the identity key, which never verifies"""
    d = degenerate
    npk = bytes([d["pk"][0] ^ 0x20]) + d["pk"][1:]
    cases = [([d["pk"], npk, d["pk2"]], d["S_k2"], d["m"]), ([d["pk"], npk], d["S_k2"], d["m"]),
             ([d["pk"], d["pk"], npk], d["S"], d["m"]), ([npk, d["pk2"], d["pk"]], d["S"], d["m"])]
    want = [oracle_memo.verify_aggregate(*c) for c in cases]
    assert want == [B.ST_OK, B.ST_NOT_VERIFIED, B.ST_OK, B.ST_NOT_VERIFIED]
    for c, w in zip(cases, want):
        assert hipbls.verify_aggregate_batch([c[0]], [c[1]], [c[2]]) == [w]
    ordinary = ([valid[0][0]], valid[0][2], valid[0][1])
    batch = [ordinary] + cases + [ordinary]
    assert hipbls.verify_aggregate_batch(*[list(x) for x in zip(*batch)]) == [B.ST_OK] + want + [B.ST_OK]
