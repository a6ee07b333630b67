"""Python-integer side of tests/test_gpu_blocks.py: the raw-limb formats of the device block harness
(tests/native/devblocks*.hip), the map between the oracle's Fp12 (oracle/bls12381.py: polynomials in
w) and pair3.h's lane form, and the case generators.  No GPU here: tests/test_blocks_ref.py checks
this module on the CPU (the map against hc_pairing, the generators against lazy28.py's model), so
that a wrong map or an inadmissible input cannot pass for a kernel bug."""
import itertools
import random

from charon_amd.tools import lazy28
from oracle import bls12381 as B

P = B.P
RBITS = 392
RM = (1 << RBITS) % P          # the Montgomery representative of 1 (R = 2^392)
RINV = pow(RM, -1, P)          # a Montgomery product is a b RINV
M28 = (1 << 28) - 1
TOP = 2 * P - 1


# ---- raw limbs ------------------------------------------------------------------------------
def words(x):
    """12 little-endian uint32 of a stored value (< 2^384)"""
    assert 0 <= x < (1 << 384)
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(12)]


def from_words(w):
    return sum(int(v) << (32 * i) for i, v in enumerate(w))


def limbs(x):
    """the normalised 14 x 28-bit limbs of a lazy value (< 2^392; limb 13 takes what is left)"""
    assert 0 <= x < (1 << 392)
    return [(x >> (28 * i)) & M28 for i in range(13)] + [x >> 364]


def lvalue(l):
    return sum(int(v) << (28 * i) for i, v in enumerate(l))


def mont(x, upper=False):
    """the stored representative of the field element x: x R mod p, or that plus p"""
    return x * RM % P + (P if upper else 0)


def unmont(raw):
    return raw * RINV % P


# ---- stored-word edge values (all below 2p) --------------------------------------------------
def _runs():
    ones32 = sum(0xFFFFFFFF << (32 * i) for i in range(11))
    mid32 = sum(0xFFFFFFFF << (32 * i) for i in range(3, 9))
    ones28 = (1 << 364) - 1
    top_word, top_limb = (2 * P) >> 352, (2 * P) >> 364
    return [((top_word - 1) << 352) | ones32,            # words 0..10 all ones
            ones32,                                       # the same below p, top word 0
            (0x1234 << 352) | mid32 | 0x89ABCDEF,         # a run of all-ones words in the middle
            ((top_limb - 1) << 364) | ones28,             # 28-bit limbs 0..12 all ones
            ones28,
            (1 << 364) | (ones28 ^ M28)]                  # limb 0 zero below a run of all-ones limbs


EDGES = [0, 1, 2, P - 2, P - 1, P, P + 1, TOP, TOP - 1, (1 << 381) - 1, 1 << 380, 2 * P - (1 << 200),
         RM, RM * RM % P] + _runs()
assert all(0 <= v < 2 * P for v in EDGES) and len(set(EDGES)) == len(EDGES)


def fp_pairs(seed=11, n_random=300):
    """(a, b) for the one- and two-operand Fp operations: every pair of edge values, then random"""
    rng = random.Random(seed)
    return [(a, b) for a in EDGES for b in EDGES] + \
        [(rng.randrange(2 * P), rng.randrange(2 * P)) for _ in range(n_random)]


def fp2_quads(seed=12, n_random=300):
    """(a0, a1, b0, b1) for the Fp2 product / square and fp_dot2 (a0 b0 +- a1 b1): the operand
    list of tests/test_hostcheck.py::test_fp2_mul_lazy_bounds over the longer edge list, the
    combinations that decide the sign correction of the real part -- (x, x, x, x): exactly 0;
    every choice of 0 / 2p - 1 for the four operands, among them (0, 2p-1, 0, 2p-1), the most
    negative, and (2p-1, 0, 2p-1, 0), the most positive, and both with the operand pairs
    swapped -- and random values below 2p"""
    rng = random.Random(seed)
    q = [(x, y, u, v) for x in EDGES[::2] for y in EDGES[1::2] for u in (TOP, 0, P) for v in (TOP, 1, P - 1)]
    q += [(x, x, x, x) for x in EDGES]
    q += list(itertools.product((0, TOP), repeat=4))
    q += [(x, P - 1, P - 1, x) for x in EDGES] + [(x, 1, 1, x + 1 if x + 1 < 2 * P else x) for x in EDGES]
    q += [tuple(rng.randrange(2 * P) for _ in range(4)) for _ in range(n_random)]
    return q


def inv_values(seed=30):
    """fp_inv wave 1: 64 distinct raw values"""
    rng = random.Random(seed)
    v = [0, 1, 2, 3, P - 2, P - 1, (P + 1) // 2, P, P + 1, TOP] + [1 << k for k in range(0, 381, 17)]
    v += [(1 << 380) - 1, (1 << 380) + 1]
    v = list(dict.fromkeys(v))
    while len(v) < 64:
        x = rng.randrange(2 * P)
        if x not in v:
            v.append(x)
    assert len(v) == 64
    return v


# ---- Fp12: the oracle's polynomial basis <-> pair3.h's lanes ----------------------------------
# oracle: f = sum_k c_k w^k, k < 12, with w^12 = 2 w^6 - 2, i.e. u = w^6 - 1.  tower.h / pair3.h:
# f = sum_i z_i w^i, i < 6, z_i = a_i + b_i u in Fp2, so c_i = a_i - b_i and c_{i+6} = b_i (the map of
# tests/test_hostcheck.py::test_pairing_matches_oracle), and lane k of a group holds
# A_k = (z_k, z_{k+3}) as the Fp4 x + y s.
def poly_to_lanes(c):
    z = [((c[i] + c[i + 6]) % P, c[i + 6] % P) for i in range(6)]
    return [(z[k][0], z[k][1], z[k + 3][0], z[k + 3][1]) for k in range(3)]


def lanes_to_poly(lanes):
    z = [None] * 6
    for k in range(3):
        x0, x1, y0, y1 = lanes[k]
        z[k], z[k + 3] = (x0, x1), (y0, y1)
    c = [0] * 12
    for i in range(6):
        c[i], c[i + 6] = (z[i][0] - z[i][1]) % P, z[i][1] % P
    return c


def lanes_tower_order(lanes):
    """the twelve Fp in hc_pairing's order: c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2 = z0, z2, z4, z1, z3, z5"""
    z = {k: lanes[k][:2] for k in range(3)}
    z.update({k + 3: lanes[k][2:] for k in range(3)})
    return [v for i in (0, 2, 4, 1, 3, 5) for v in z[i]]


def raw_to_poly(raw_lanes):
    """the Fp12 element whose stored lane form is raw_lanes (3 x 4 raw values below 2p)"""
    return lanes_to_poly([tuple(unmont(v) for v in lane) for lane in raw_lanes])


def poly_to_raw(c, upper=False):
    return [tuple(mont(v, upper) for v in lane) for lane in poly_to_lanes(c)]


def line_poly(a0, a1, b1):
    """a0 + a1 v + b1 v w (v = w^2) for Fp2 values: z0 = a0, z2 = a1, z3 = b1"""
    return lanes_to_poly([(a0[0], a0[1], b1[0], b1[1]), (0, 0, 0, 0), (a1[0], a1[1], 0, 0)])


def p12_conj(c):
    """f^(p^6): the automorphism of order two, w -> -w (tests/test_blocks_ref.py compares it with
    the power)"""
    return [(-v) % P if k & 1 else v % P for k, v in enumerate(c)]


FEXP3 = 3 * B.FINAL_EXP                       # the device chain computes f^(3 (p^12 - 1) / r)
CYC_EXP = (P ** 6 - 1) * (P ** 2 + 1)         # into the cyclotomic subgroup


def group_values(seed=21, n_random=3):
    """[(name, raw lanes)]: random values, one in both representatives, all coordinates p - 1 and
    all 2p - 1"""
    rng = random.Random(seed)
    out = [("random%d" % i, [tuple(rng.randrange(2 * P) for _ in range(4)) for _ in range(3)]) for i in range(n_random)]
    out.append(("one", poly_to_raw(B.P12_ONE)))
    out.append(("one_upper", poly_to_raw(B.P12_ONE, upper=True)))
    out.append(("all_p-1", [(P - 1,) * 4] * 3))
    out.append(("all_2p-1", [(TOP,) * 4] * 3))
    return out


def is_one_values():
    """one in both representatives, and one changed in a single coordinate of a single role (the
    coordinate 1 changed to 0 and to 2, the others from 0 to 1 and to their upper representative's
    neighbour p + 1), for each of the six Fp2 coordinates (both halves)"""
    out = [("one", poly_to_raw(B.P12_ONE), True), ("one_upper", poly_to_raw(B.P12_ONE, upper=True), True),
           ("one_mixed", [(RM + P, 0, P, 0), (P, 0, 0, P), (0, P, P, 0)], True)]
    for k in range(3):
        for j in range(4):
            for delta, upper in ((1, False), (1, True), (P - 1, False)):
                lanes = [list(l) for l in poly_to_lanes(B.P12_ONE)]
                lanes[k][j] = (lanes[k][j] + delta) % P
                raw = [tuple(mont(v, upper) for v in lane) for lane in lanes]
                out.append(("one+%d@%d.%d%s" % (delta if delta == 1 else -1, k, j, "u" if upper else ""), raw, False))
    return out


# ---- lazy limbs -------------------------------------------------------------------------------
# Patterns are built the way ec28.h / pair28.h build them, and every operand set is passed through
# lazy28.py's model as a degenerate Bound (the concrete limbs, value + 1) before it may be used.
LAZY_X = [0, 1, 2, P - 2, P - 1, RM, 1 << 380, (1 << 364) - 1, ((P >> 364) << 364) - 1]


def bound(l):
    return lazy28.Bound(l, lvalue(l) + 1)


def l_add(a, b):
    return [x + y for x, y in zip(a, b)]


def l_shl(a, s):
    return [x << s for x in a]


def l_sub(a, b, site):
    """ec28.h l_sub<S, T>: a + (K - b) limb by limb, (S, T) = lazy28.KSITE[site]"""
    k = lazy28.kconst(*lazy28.KSITE[site])
    lazy28.sub(bound(a), bound(b), site)  # asserts that K dominates b
    return [x + (kk - y) for x, kk, y in zip(a, k, b)]


def sub_kmax(site, vmax):
    """the largest k < vmax for which K of `site` dominates every normalised value below (k + 1) p"""
    k13 = lazy28.kconst(*lazy28.KSITE[site])[13]
    ks = [k for k in range(vmax) if ((k + 1) * P) >> 364 <= k13]
    return max(ks) if ks else None


def all_ones(k):
    """the normalised value below (k + 1) p with limbs 0..12 all ones"""
    return limbs(((((k + 1) * P) >> 364) << 364) - 1)


def _sites(prefixes):
    """one site per distinct constant (S, T) among KSITE's sites of these prefixes"""
    seen = {}
    for s, st in lazy28.KSITE.items():
        if s[0] in prefixes and s != "2N":
            seen.setdefault(st, s)
    return list(seen.values())


FIELD_SITES = {"Fp": _sites("1"), "Fp2": _sites("234")}


def kinds(field):
    return ["N", "ADD", "SHL1", "SHL2"] + ["SUB:" + s for s in FIELD_SITES[field] if sub_kmax(s, lazy28.VMAX[field]) is not None]


def operand(kind, field, pick, pick_sub=None):
    """one operand of `kind`; pick(kmax) returns the normalised limbs of some x + k p, k <= kmax
    (pick_sub: the same for a subtrahend)"""
    vmax = lazy28.VMAX[field]
    if kind == "N":
        return pick(vmax - 1)
    if kind == "ADD":
        return l_add(pick(vmax - 1), pick(vmax - 1))
    if kind in ("SHL1", "SHL2"):
        return l_shl(pick(vmax - 1), int(kind[3]))
    site = kind[4:]
    return l_sub(pick(vmax - 1), (pick_sub or pick)(sub_kmax(site, vmax)), site)


def worst(kind, field):
    """the pattern's largest limbs: all-ones operands, a subtrahend of zero"""
    return operand(kind, field, all_ones, lambda kmax: [0] * 14)


def col_max(a, b):
    """the largest column sum of a_j b_(k-j) (the products' own terms), for ranking patterns"""
    return max(sum(a[j] * b[k - j] for j in range(max(0, k - 13), min(k, 13) + 1)) for k in range(27))


def admits(fn, *args):
    """does lazy28's model admit this operand set?  Used ONLY to choose which pattern kinds the
    generators combine (on their worst cases) -- a generated case is never dropped: it is asserted."""
    try:
        fn(*args)
        return True
    except AssertionError:
        return False


def _picker(rng):
    def pick(kmax):
        x = rng.choice(LAZY_X) if rng.random() < 0.4 else rng.randrange(P)
        k = rng.choice((0, kmax)) if rng.random() < 0.5 else rng.randrange(kmax + 1)
        return limbs(x + k * P)
    return pick


def _model_f2mul(a0, a1, b0, b1):
    lazy28.f2_mul((bound(a0), bound(a1)), (bound(b0), bound(b1)), "2N")


def _model_f2sqr(site):
    return lambda a0, a1: lazy28.f2_sqr((bound(a0), bound(a1)), site)


def mul_cases(field="Fp", seed=41, per_pair=2):
    """(a, b) for l_mul / l_mul2 / p_mul2: every pair of pattern kinds whose worst case the model
    admits, random and edge values in them; first the admitted worst-case pair with the largest
    column sum"""
    rng = random.Random(seed)
    ks = kinds(field)
    ok = [(ka, kb) for ka in ks for kb in ks if admits(lazy28.mul, bound(worst(ka, field)), bound(worst(kb, field)))]
    best = max(ok, key=lambda p: col_max(worst(p[0], field), worst(p[1], field)))
    cases = [(worst(best[0], field), worst(best[1], field))]
    pick = _picker(rng)
    for ka, kb in ok:
        cases.append((worst(ka, field), worst(kb, field)))
        cases += [(operand(ka, field, pick), operand(kb, field, pick)) for _ in range(per_pair)]
    for a, b in cases:
        lazy28.mul(bound(a), bound(b))
    return cases


def sqr_cases(field="Fp", seed=42, per_kind=8):
    rng = random.Random(seed)
    ok = [k for k in kinds(field) if admits(lazy28.sqr, bound(worst(k, field)))]
    best = max(ok, key=lambda k: col_max(worst(k, field), worst(k, field)))
    cases = [worst(best, field)]
    pick = _picker(rng)
    for k in ok:
        cases.append(worst(k, field))
        cases += [operand(k, field, pick) for _ in range(per_kind)]
    for a in cases:
        lazy28.sqr(bound(a))
    return cases


def f2mul_cases(seed=43, per_pair=3):
    """(a0, a1, b0, b1) for f2l_mul / fm / fm3 / fm2 (real = a0 b0 + (K - a1) b1, K = KSITE["2N"]):
    pattern kinds per operand (both coefficients of an operand the same kind, as the formulas
    produce them), chosen and checked as mul_cases"""
    rng = random.Random(seed)
    ks = kinds("Fp2")
    w = {k: worst(k, "Fp2") for k in ks}
    ok = [(ka, kb) for ka in ks for kb in ks if admits(_model_f2mul, w[ka], w[ka], w[kb], w[kb])]
    k2n = lazy28.kconst(*lazy28.KSITE["2N"])

    def cmax(p):
        a, b = w[p[0]], w[p[1]]
        na = [kk - x for kk, x in zip(k2n, a)]
        return max(sum(a[j] * b[k - j] + na[j] * b[k - j] for j in range(max(0, k - 13), min(k, 13) + 1)) for k in range(27))
    best = max(ok, key=cmax)
    cases = [(w[best[0]], w[best[0]], w[best[1]], w[best[1]])]
    pick = _picker(rng)
    for ka, kb in ok:
        cases.append((w[ka], w[ka], w[kb], w[kb]))
        cases += [(operand(ka, "Fp2", pick), operand(ka, "Fp2", pick), operand(kb, "Fp2", pick), operand(kb, "Fp2", pick))
                  for _ in range(per_pair)]
    zero = [0] * 14
    cases += [(w["N"], zero, w["N"], zero), (zero, w["N"], zero, w["N"]), (zero, zero, w["N"], w["N"])]
    for c in cases:
        _model_f2mul(*c)
    return cases


SQR_SITES = {(36, 1): "2Q", (78, 1): "3Q", (9, 2): "4Q"}  # the instantiations of f2l_sqr_k / fs / fs3
assert all(lazy28.KSITE[s] == st for st, s in SQR_SITES.items())


def f2sqr_cases(st, seed=44, per_kind=40):
    """(a0, a1) for f2l_sqr_k<S, T> / fs<S, T> / fs3<S, T>: (a0 + a1)(a0 + K - a1), (2 a0) a1"""
    site = SQR_SITES[st]
    model = _model_f2sqr(site)
    rng = random.Random(seed + st[0])
    # a1 is a subtrahend of the site's K: operands x + k p only up to the k that K dominates
    kcap = sub_kmax(site, lazy28.VMAX["Fp2"])
    ks = kinds("Fp2")
    zero = [0] * 14
    w = {k: operand(k, "Fp2", lambda kmax: all_ones(min(kmax, kcap)), lambda kmax: zero) for k in ks}
    ok = [k for k in ks if admits(model, w[k], w[k])]
    kk = lazy28.kconst(*st)
    best = max(ok, key=lambda k: col_max(l_add(w[k], w[k]), [x + (c - y) for x, c, y in zip(w[k], kk, w[k])]))
    cases = [(w[best], w[best])]
    rpick = _picker(rng)

    def pick(kmax):
        return rpick(min(kmax, kcap))
    for k in ok:
        cases.append((w[k], w[k]))
        cases += [(operand(k, "Fp2", pick), operand(k, "Fp2", pick)) for _ in range(per_kind)]
    cases += [(w["N"], zero), (zero, w["N"]), (zero, zero)]
    for c in cases:
        model(*c)
    return cases


def dot_cases(seed=45):
    """(x0, x1, y0, y1) for l_dot = x0 y0 + x1 y1, as fm(F2Half) / F2Hex feed it from an admitted
    Fp2 product: (a0, K - a1, b0, b1) for the real part and (a0, a1, b1, b0) for the other"""
    k2n = lazy28.kconst(*lazy28.KSITE["2N"])
    out = []
    for a0, a1, b0, b1 in f2mul_cases(seed):
        out.append((a0, [k - x for k, x in zip(k2n, a1)], b0, b1))
        out.append((a0, a1, b1, b0))
    return out


R392_INV = pow(1 << RBITS, -1, P)


def check_lazy(r, want_num, cap):
    """a product's output r (14 limbs): normalised, congruent to want_num / R, and below the bound
    lazy28.py's model gives it (cap = the operands' integer numerator: r <= cap / R + p)"""
    assert len(r) == 14 and all(0 <= int(v) < (1 << 28) for v in r[:13]), r
    v = lvalue(r)
    assert v % P == want_num * R392_INV % P
    assert v < cap // (1 << RBITS) + P + 1


# ---- curve layer (tests/native/devblocks_curve.hip, devblocks_msm.hip; tests/test_gpu_curve.py) ----
# A group element is the oracle's: an affine tuple (x, y) of field elements (Fp: int, Fp2: (c0, c1))
# or None.  A raw point is (slots, inf): six raw integers X.c0, X.c1, Y.c0, Y.c1, Z.c0, Z.c1 (G1 fills
# the c0 slots), each the Montgomery representative plus a multiple of p, and the `inf` flag.
FIELD_OPS = {1: B._FpOps, 2: B._Fp2Ops}
CURVE_B = {1: B.B_G1, 2: B.B_G2}
PT_WORDS, PT_INF = 88, 84


def fcoords(field, v):
    """the Fp coordinates of a field element, as a pair (c0, c1)"""
    return (v, 0) if field == 1 else tuple(v)


def felem(field, c0, c1):
    return c0 % P if field == 1 else (c0 % P, c1 % P)


def frand(field, rng, nonzero=True):
    while True:
        v = rng.randrange(P) if field == 1 else (rng.randrange(P), rng.randrange(P))
        if not nonzero or v not in (0, (0, 0)):
            return v


def jac_coords(field, pt, lam):
    """the Jacobian representative (X, Y, Z) = (x lam^2, y lam^3, lam) of an affine point; infinity
    as (1, 1, 0), what ec.h jac_infinity holds"""
    F = FIELD_OPS[field]
    if pt is None:
        return F.one, F.one, F.zero
    l2 = F.mul(lam, lam)
    return F.mul(pt[0], l2), F.mul(pt[1], F.mul(l2, lam)), lam


def raw_slots(field, coords, ks=0):
    """raw integers of three field elements: mont(c) + k p, k from ks (an int, or six of them)"""
    ks = [ks] * 6 if isinstance(ks, int) else list(ks)
    flat = [c for v in coords for c in fcoords(field, v)]
    return [mont(c) + k * P for c, k in zip(flat, ks)]


def affine_of(field, slots, inf=False):
    """the group element of raw Jacobian slots (any multiples of p on top): None if flagged or Z = 0"""
    F = FIELD_OPS[field]
    X, Y, Z = (felem(field, unmont(slots[2 * k]), unmont(slots[2 * k + 1])) for k in range(3))
    if inf or Z == F.zero:
        return None
    zi = F.inv(Z)
    zi2 = F.mul(zi, zi)
    return F.mul(X, zi2), F.mul(Y, F.mul(zi2, zi))


def pack_point(slots, inf, lazy):
    """one 88-word point record: 14 limbs (lazy) or 12 words per slot"""
    rec = [0] * PT_WORDS
    for k, v in enumerate(slots):
        w = limbs(v) if lazy else words(v)
        rec[14 * k:14 * k + len(w)] = w
    rec[PT_INF] = 1 if inf else 0
    return rec


def unpack_point(rec, lazy):
    """(slots, inf, normalised) of an output record"""
    rec = [int(v) for v in rec]
    if lazy:
        sl = [lvalue(rec[14 * k:14 * k + 14]) for k in range(6)]
        normalised = all(v <= M28 for k in range(6) for v in rec[14 * k:14 * k + 13])
    else:
        sl = [from_words(rec[14 * k:14 * k + 12]) for k in range(6)]
        normalised = True
    return sl, rec[PT_INF] != 0, normalised


def entry_words(field, coords, inf=None, upper=False):
    """the stored words of a product record (layout.h): the field elements' Montgomery words in
    order, then -- for the affine records G1AEntry / HmEntry -- the inf flag and three words of padding"""
    out = []
    for v in coords:
        for c in fcoords(field, v)[:field]:
            out += words(mont(c, upper))
    if inf is not None:
        out += [1 if inf else 0, 0, 0, 0]
    return out


def affine_entry(field, pt, upper=False):
    """G1AEntry (28 words) / HmEntry (52 words) of a group element"""
    F = FIELD_OPS[field]
    return entry_words(field, (F.zero, F.zero) if pt is None else pt, inf=pt is None, upper=upper)


def jac_entry(field, pt, lam=None, upper=False):
    """G1JEntry (36 words) / G2JEntry (72 words): the representative with Z = lam (default 1)"""
    return entry_words(field, jac_coords(field, pt, FIELD_OPS[field].one if lam is None else lam), upper=upper)


def entry_affine(field, w):
    """the group element of a Jacobian record's words"""
    vals = [from_words(w[12 * k:12 * k + 12]) for k in range(3 * field)]
    slots = vals if field == 2 else [vals[0], 0, vals[1], 0, vals[2], 0]
    return affine_of(field, slots)


def load_torsion():
    """tests/golden/torsion_points.json as {1: [...], 2: [...]} of (kind, q, order, group element)"""
    import json
    import os
    doc = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "torsion_points.json")))
    out = {}
    for field, g, dec in ((1, "g1", B.g1_decompress), (2, "g2", B.g2_decompress)):
        out[field] = [(e["kind"], int(e["q"]), int(e["order"]), dec(bytes.fromhex(e["point"]), subgroup_check=False))
                      for e in doc[g]["points"]]
    return out


def ec_add(field, a, b):
    return B.ec_add(a, b, FIELD_OPS[field])


def ec_mul(field, a, k):
    return B.ec_mul(a, k, FIELD_OPS[field])


def ec_neg(field, a):
    return B.ec_neg(a, FIELD_OPS[field])


# ---- hash-to-curve (tests/native/devblocks_h2c.hip, devblocks_h2c_std.hip; tests/test_gpu_hash.py) ----
# the exponents of fp.h's four window schedules, from the formulas of their comments
# (charon_amd/tools/gen_consts.py writes the tables from the same four) -- never decoded from the tables
POW_EXP = {"P_MINUS_2": P - 2, "SQRT": (P + 1) // 4, "P_M3_4": (P - 3) // 4, "LEGENDRE": (P - 1) // 2}


def pow_expected(a, e):
    """the value fp_pow_win's stored result must be congruent to: (a / R)^e R = a^e R^(1 - e)"""
    return pow(a, e, P) * pow(RINV, e - 1, P) % P


def reps2(v):
    """the four stored forms (c0 | c0 + p, c1 | c1 + p) of the Fp2 element v"""
    return [(mont(v[0], k0), mont(v[1], k1)) for k0 in (False, True) for k1 in (False, True)]


def fp2_words(raw):
    return words(raw[0]) + words(raw[1])


# message lengths: the block count of xmd_b0 (1 + (len + 47 + 8) // 64 after Z_pad) changes between
# 8 / 9, 72 / 73, 136 / 137 and 200 / 201; 0x80 is the last byte of a block at 16 and 80
H2C_LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 72, 73, 80, 81, 136, 137, 200, 300]
XMD_TAIL = (256).to_bytes(2, "big") + b"\x00" + B.DST_POP + bytes([len(B.DST_POP)])


def xmd_b0_blocks(n):
    return (n + len(XMD_TAIL) + 8) // 64 + 1


def h2c_messages(seed=5, per_length=3, extra=(9, 73, 137, 16, 80)):
    """66 distinct messages, every length of H2C_LENGTHS three times (the empty one once, five lengths
    once more), ordered so that neighbours -- neighbouring lanes of a wave -- differ in xmd_b0's
    block count"""
    rng = random.Random(seed)
    pool = [bytes(rng.randrange(256) for _ in range(n)) if n else b"" for n in H2C_LENGTHS for _ in range(per_length)]
    pool += [bytes(rng.randrange(256) for _ in range(n)) for n in extra]
    pool = list(dict.fromkeys(pool))  # the empty message once
    by = {}
    for m in pool:
        by.setdefault(xmd_b0_blocks(len(m)), []).append(m)
    out, prev = [], None
    while any(by.values()):  # the fullest class that differs from the previous message's
        k = max((c for c in by if by[c] and c != prev), key=lambda c: len(by[c]))
        out.append(by[k].pop())
        prev = k
    assert all(xmd_b0_blocks(len(a)) != xmd_b0_blocks(len(b)) for a, b in zip(out, out[1:]))
    assert {len(m) for m in out} == set(H2C_LENGTHS) and len(out) >= 65
    return out


def sswu_gx1_is_square(u):
    """whether g(x1) of RFC 9380's simplified SWU on E2' is a square at u (the map then takes x1)"""
    A, Bc, Z = B.SSWU_A, B.SSWU_B, B.SSWU_Z
    zu2 = B.f2_mul(Z, B.f2_sqr(u))
    tv1 = B.f2_add(B.f2_sqr(zu2), zu2)
    if B.f2_is_zero(tv1):
        x1 = B.f2_mul(Bc, B.f2_inv(B.f2_mul(Z, A)))
    else:
        x1 = B.f2_mul(B.f2_mul(B.f2_neg(Bc), B.f2_inv(A)), B.f2_add(B.F2_ONE, B.f2_inv(tv1)))
    return B.f2_is_square(B.f2_add(B.f2_add(B.f2_mul(B.f2_sqr(x1), x1), B.f2_mul(A, x1)), Bc))


def sswu_inputs(seed=1, n_random=40):
    """[(name, u, stored form (raw c0, raw c1))] for the map: u = 0 in its four stored forms, small
    and extreme values, u and -u, each coordinate in [p, 2p), random u"""
    rng = random.Random(seed)
    out = [("zero%d" % k, (0, 0), r) for k, r in enumerate(reps2((0, 0)))]
    small = [(1, 0), (0, 1), (1, 1), (P - 1, 0), (0, P - 1), (2, 0)]
    out += [("small%d" % k, u, reps2(u)[0]) for k, u in enumerate(small)]
    rnd = [(rng.randrange(P), rng.randrange(P)) for _ in range(n_random)]
    for k, u in enumerate(rnd):
        out.append(("random%d" % k, u, reps2(u)[0]))
    for k, u in enumerate(rnd[:6]):
        out.append(("neg%d" % k, B.f2_neg(u), reps2(B.f2_neg(u))[0]))
    for k, u in enumerate(rnd[6:9] + small[:3]):
        out += [("upper%d.%d" % (k, j), u, r) for j, r in enumerate(reps2(u)[1:], 1)]
    return out


def sswu_reference(u):
    return B.iso3_map(B.map_to_curve_sswu(u))


def msm_reference(points, coefs):
    """sum_i [a_i] s_i + [b_i] (-psi^2 s_i) with the oracle's group law, term by term"""
    total = None
    for pt, (a, b) in zip(points, coefs):
        if pt is None:
            continue
        total = B.g2_add(total, B.g2_mul(pt, a))
        total = B.g2_add(total, B.g2_mul(B.g2_neg(B.g2_psi(B.g2_psi(pt))), b))
    return total


# ---- Miller loops (tests/native/devblocks_pair.hip, devblocks_vgroup.hip; tests/test_gpu_pairing.py) ----
# The loop order comes from X_PARAM alone: bit 62 .. 0 of |x| below its top bit, a doubling per bit
# and an addition after each set one.
X_ABS = -B.X_PARAM
MILLER_BITS = bin(X_ABS)[3:]
N_LINES = len(MILLER_BITS) + MILLER_BITS.count("1")
G1_NEG = B.g1_neg(B.G1_GEN)
_CHAINS, _PAIRINGS, _POWS, _ATINV = {}, {}, {}, {}


def miller_chain(Q):
    """The affine chain of the oracle's miller_loop over Q: per line (kind, lambda, x_T, y_T), T the
    point the line is taken at (the formulas are miller_loop's own), memoised"""
    if Q in _CHAINS:
        return _CHAINS[Q]
    out, T = [], Q
    for bit in MILLER_BITS:
        xt, yt = T
        lam = B.f2_mul(B.f2_mul(B.f2(3), B.f2_sqr(xt)), B.f2_inv(B.f2_mul(B.f2(2), yt)))
        out.append(("dbl", lam, xt, yt))
        x3 = B.f2_sub(B.f2_sub(B.f2_sqr(lam), xt), xt)
        T = (x3, B.f2_sub(B.f2_mul(lam, B.f2_sub(xt, x3)), yt))
        if bit == "1":
            xt, yt = T
            lam = B.f2_mul(B.f2_sub(Q[1], yt), B.f2_inv(B.f2_sub(Q[0], xt)))
            out.append(("add", lam, xt, yt))
            x3 = B.f2_sub(B.f2_sub(B.f2_sqr(lam), xt), Q[0])
            T = (x3, B.f2_sub(B.f2_mul(lam, B.f2_sub(xt, x3)), yt))
    assert len(out) == N_LINES
    _CHAINS[Q] = out
    return out


def line_matches(line, step, at=None):
    """Is the device line (a0, c1, c2) -- Fp2 field elements -- the oracle's line of `step` up to the
    factor w^3 c2 (in Fp4: the final exponentiation removes it)?  c2 != 0, a0 = c2 (lambda x_T - y_T),
    c1 = -c2 lambda.  at = (x_P, y_P): the line came evaluated, (a0, c1 x_P, c2 y_P)."""
    a0, c1, c2 = line
    if at is not None:
        if at not in _ATINV:
            _ATINV[at] = (B.fp_inv(at[0]), B.fp_inv(at[1]))
        c1 = B.f2_mul(c1, (_ATINV[at][0], 0))
        c2 = B.f2_mul(c2, (_ATINV[at][1], 0))
    _, lam, xt, yt = step
    if B.f2_is_zero(c2):
        return False
    return tuple(a0) == B.f2_mul(c2, B.f2_sub(B.f2_mul(lam, xt), yt)) and tuple(c1) == B.f2_neg(B.f2_mul(c2, lam))


def miller_from_lines(*chains):
    """The Miller value of evaluated lines (a0, a1, b1), N_LINES per chain, in the schedule X_PARAM
    gives: f^2 in front of every doubling line but the first, then the line of every chain -- one
    chain, or several sharing the squarings (a multi-Miller loop)"""
    assert chains and all(len(c) == N_LINES for c in chains)
    f, i = B.P12_ONE, 0

    def step(f, i):
        for c in chains:
            f = B._p12_mul(f, line_poly(*c[i]))
        return f
    for k, bit in enumerate(MILLER_BITS):
        if k:
            f = B._p12_mul(f, f)
        f, i = step(f, i), i + 1
        if bit == "1":
            f, i = step(f, i), i + 1
    assert i == N_LINES
    return f


def pow3(f):
    """f^FEXP3, memoised by value"""
    key = tuple(f)
    if key not in _POWS:
        _POWS[key] = B._p12_pow(list(f), FEXP3)
    return _POWS[key]


def pairing3(Pt, Q):
    """e(P, Q)^3 as the device computes it: the oracle's Miller value to the power FEXP3, memoised"""
    if (Pt, Q) not in _PAIRINGS:
        _PAIRINGS[(Pt, Q)] = pow3(B.miller_loop(Pt, Q))
    return _PAIRINGS[(Pt, Q)]


def eval_line(line, Pt):
    """(a0, c1, c2) at P: (a0, c1 x_P, c2 y_P)"""
    return line[0], B.f2_mul(line[1], (Pt[0], 0)), B.f2_mul(line[2], (Pt[1], 0))


LINE_WORDS, F12_WORDS, HM_WORDS, MSG_WORDS = 72, 144, 52, 52 + 72 * N_LINES


def line_of_words(w):
    """(a0, a1, b1) as field elements and the six raw values of a LineEntry's 72 words"""
    raw = [from_words(w[12 * k:12 * k + 12]) for k in range(6)]
    v = [unmont(r) for r in raw]
    return ((v[0], v[1]), (v[2], v[3]), (v[4], v[5])), raw


def f12_of_words(w):
    """the Fp12 element (oracle polynomial) and the twelve raw values of a stored value's 144 words
    (three Fp4Entry: role k holds x.c0, x.c1, y.c0, y.c1)"""
    raw = [from_words(w[12 * k:12 * k + 12]) for k in range(12)]
    return raw_to_poly([tuple(raw[4 * k:4 * k + 4]) for k in range(3)]), raw


def f12_words(c, upper=False):
    return [x for lane in poly_to_raw(c, upper) for v in lane for x in words(v)]


# ---- the batched verification's combination (vbatch.hip; tests/native/devblocks_vbatch.hip,
# tests/test_gpu_vbatch.py) ----
# Coefficients: the digest is hashlib's SHA-256 over the 8 key words and the stream position, big-endian.
# r = a + b lambda with lambda = -x^2 mod r (rlc.h), the eigenvalue of phi on G1 and of -psi^2 on G2.
LAMBDA = (-B.X_PARAM ** 2) % B.R
SPARSE_DIGITS = 22
SPARSE_PAIRS = [(1, 0), (0, 1), (1, 1), (1, -1)]  # entry d & 3, negated when d & 4 (ec28.h RLC_DIGITS)


def rlc_hash_words(key, item):
    """the eight big-endian words of SHA-256(key words || item)"""
    import hashlib
    d = hashlib.sha256(b"".join(int(w).to_bytes(4, "big") for w in key) + int(item).to_bytes(4, "big")).digest()
    return [int.from_bytes(d[4 * k:4 * k + 4], "big") for k in range(8)]


def rlc_coeffs(key, item):
    """the dense pair (a, b) of stream position `item`.  (A digest whose first 64 bits are zero
    would give (1, 0) on the device; reaching that line takes a hash preimage, so it is not restated.)"""
    h = rlc_hash_words(key, item)
    assert h[0] | h[1]
    return h[0], h[1]


def rlc_record(key, item):
    """the sparse record of stream position `item`: 10 + 10 + 2 three-bit digits, word 3 = usable"""
    h = rlc_hash_words(key, item)
    return h[0] & 0x3FFFFFFF, h[1] & 0x3FFFFFFF, h[2] & 0x3F, 1


def sparse_ab(rec):
    """(A, B) of a sparse record: A = sum u_j 4^j, B = sum v_j 4^j; digit j is bits 3 (j mod 10) .. + 2
    of word j // 10"""
    A = Bv = 0
    for j in range(SPARSE_DIGITS):
        d = (rec[j // 10] >> (3 * (j % 10))) & 7
        u, v = SPARSE_PAIRS[d & 3]
        if d & 4:
            u, v = -u, -v
        A += u * 4 ** j
        Bv += v * 4 ** j
    return A, Bv


def rlc_scalar(a, b):
    return (a + b * LAMBDA) % B.R


class FixedBase:
    """[k] base for many k: a table of d 16^w base (oracle additions), summed with mixed Jacobian
    additions in Python integers and one inversion.  test_blocks_ref.py holds it against the oracle."""

    def __init__(self, field, base):
        self.field, self.F, self.base = field, FIELD_OPS[field], base
        self.tab, self._memo = [], {}
        w = base
        for _ in range(64):
            row, acc = [None], None
            for _ in range(15):
                acc = ec_add(field, acc, w)
                row.append(acc)
            self.tab.append(row)
            w = ec_add(field, row[15], w)

    def _madd(self, J, q):
        F = self.F
        if J is None:
            return q[0], q[1], F.one
        X, Y, Z = J
        zz = F.mul(Z, Z)
        h, r = F.sub(F.mul(q[0], zz), X), F.sub(F.mul(q[1], F.mul(zz, Z)), Y)
        if h == F.zero:  # the same x: fall back to the oracle's law
            zi = F.inv(Z)
            zi2 = F.mul(zi, zi)
            s = ec_add(self.field, (F.mul(X, zi2), F.mul(Y, F.mul(zi2, zi))), q)
            return None if s is None else (s[0], s[1], F.one)
        hh = F.mul(h, h)
        hhh, v = F.mul(h, hh), F.mul(X, hh)
        x3 = F.sub(F.sub(F.mul(r, r), hhh), F.add(v, v))
        return x3, F.sub(F.mul(r, F.sub(v, x3)), F.mul(Y, hhh)), F.mul(Z, h)

    def mul(self, k):
        k %= B.R
        if k not in self._memo:
            J, F = None, self.F
            for w in range(64):
                d = (k >> (4 * w)) & 15
                if d:
                    J = self._madd(J, self.tab[w][d])
            if J is not None:
                zi = F.inv(J[2])
                zi2 = F.mul(zi, zi)
                J = (F.mul(J[0], zi2), F.mul(J[1], F.mul(zi2, zi)))
            self._memo[k] = J
        return self._memo[k]


def plan_chunks(grp_off, cmax):
    """The chunk plan of the comment above vbatch.hip k_plan_count: group g's items cut into
    ceil(size / cmax) nearly equal chunks of consecutive items -> (cnt, coff, cfirst, ccount); chunk k
    of nc covers [k size // nc, (k + 1) size // nc); bit 31 of ccount marks a group of ONE item"""
    ng = len(grp_off) - 1
    cnt = [(grp_off[g + 1] - grp_off[g] + cmax - 1) // cmax for g in range(ng)]
    coff = [0]
    for c in cnt:
        coff.append(coff[-1] + c)
    cfirst, ccount = [], []
    for g in range(ng):
        b, sz = grp_off[g], grp_off[g + 1] - grp_off[g]
        for k in range(cnt[g]):
            lo, hi = k * sz // cnt[g], (k + 1) * sz // cnt[g]
            cfirst.append(b + lo)
            ccount.append((hi - lo) | (0x80000000 if sz == 1 else 0))
    return cnt, coff, cfirst, ccount


# ---- the threshold aggregation (threshold.hip; tests/native/devblocks_threshold.hip,
# tests/test_gpu_threshold.py) ----
# z = |x|: psi acts on G2 as multiplication by x = -z, so sum_i a_i (-1)^i psi^i(sigma) = [sum_i a_i z^i] sigma.
TA_Z = X_ABS
TA_SMALL_T = range(2, 17)  # ta_small.h: the member counts the small-scalar split takes


def ta_lambda(ids):
    """lambda_j(0) = prod_{m != j} x_m / (x_m - x_j) per member, the numerator and the denominator as
    exact Python integers (any signed 64-bit indices) and only their quotient reduced mod r.  A group of
    one has lambda = 1.  An entry is None where member j itself shows the combine failure: ANOTHER
    member's index is 0 mod r (the numerator vanishes) or equals x_j mod r (the denominator does)."""
    if len(ids) == 1:
        return [1]
    out = []
    for j, xj in enumerate(ids):
        num = den = 1
        for m, xm in enumerate(ids):
            if m != j:
                num *= xm
                den *= xm - xj
        out.append(None if num % B.R == 0 or den % B.R == 0 else num * pow(den, -1, B.R) % B.R)
    return out


def ta_digits(v):
    """the four base-z digits of 0 <= v < z^4, least significant first"""
    assert 0 <= v < TA_Z ** 4
    a = [v // TA_Z ** i % TA_Z for i in range(4)]
    assert sum(d * TA_Z ** i for i, d in enumerate(a)) == v and all(d < TA_Z for d in a)
    return a


def ta_digit_scalar(a):
    """the scalar of arbitrary digits: sum_i a_i (-1)^i psi^i(sigma) = [sum_i a_i z^i mod r] sigma"""
    return sum(d * TA_Z ** i for i, d in enumerate(a)) % B.R


def ta_small_split(ids):
    """ta_small.h's form of the coefficients from Python integers: with P = prod x_m, E_j = x_j prod_{m
    != j} (x_m - x_j) and L = lcm |E_j|: c_j = L / E_j and s = P / L mod r, so lambda_j = s c_j.
    -> (c, s), or None where the header refuses: t outside 2..16, an index 0, duplicates, |x| >= 2^31, any
    intermediate beyond 63 bits (the products to E_j and the running lcm only grow in magnitude, so it is
    the final E_j and L that decide), E_j = -2^63."""
    import math
    t = len(ids)
    if t not in TA_SMALL_T or any(x == 0 or abs(x) >= 1 << 31 for x in ids) or len(set(ids)) != t:
        return None
    E = []
    for j, xj in enumerate(ids):
        e = xj
        for m, xm in enumerate(ids):
            if m != j:
                e *= xm - xj
        if not -(1 << 63) < e < (1 << 63):
            return None
        E.append(e)
    L = 1
    for e in E:
        L = L * abs(e) // math.gcd(L, abs(e))
        if L >= 1 << 63:
            return None
    Pm = 1
    for x in ids:
        Pm *= x
    return [L // e for e in E], Pm * pow(L, -1, B.R) % B.R
