"""The device-only arithmetic blocks on the GPU against Python integers and the oracle's Fp12.

Every other GPU test goes through the C ABI, where the field values that reach the kernels are
effectively random; the block tests of tests/test_hostcheck.py and tests/test_lazy28.py run the g++
build, which shares none of fp.h's carry builtins, out-of-line leaves and LDS argument slots, nor
any lane exchange.  Here the test-only harness tests/native/devblocks*.hip (built for gfx950 from
the product headers, once with fp.h's default HB_ARG_LANES and once with pipeline.hip's 128) runs
one block per kernel on chosen raw limbs: stored words (12 x uint32 of the Montgomery
representative itself, R = 2^392, any value below 2p), lazy limbs (14 x 28 bits) and lane-group
values (three Fp4Entry).  Every comparison is exact, against Python integers (tests/blocks_ref.py);
the host harness is never the reference."""
import ctypes
import random

import numpy as np
import pytest

import blocks_ref as R
from oracle import bls12381 as B

pytestmark = pytest.mark.gpu

P = B.P
U32P = ctypes.POINTER(ctypes.c_uint32)
I32P = ctypes.POINTER(ctypes.c_int)

A_OPS = {n: i for i, n in enumerate(
    "add sub neg mul sqr f2mul f2sqr dot2 mul28 sqr28 inv invct".split())}
B_OPS = {n: i for i, n in enumerate(
    "lmul lsqr lmul2 lsqr2 f2mul f2sqr36 f2sqr78 f2sqr9 ldot h_fm h_fs36 h_fs78 h_pmul2 h_psqr2 x_fm3 x_fm2 x_fs3".split())}
C_OPS = {n: i for i, n in enumerate(
    "sqr mul mul_line cyc conj frob1 frob2 fexp is_one s_mul s_inv s_is_one".split())}
GROUPS = {"Grp": (0, 3, 21), "Grp6": (1, 6, 10), "Grp18": (2, 18, 3)}  # kind, lanes per value, values per wave


def _ok(rc, what):
    """A failed launch or synchronise (devblocks.h DB_E_LAUNCH, DB_E_SYNC) is a GPU error: the run
    ends there, nothing more is started on the card."""
    if rc in (-5, -6):
        pytest.exit(f"{what} returned {rc}: the GPU reported an error; no further block test is run", returncode=3)
    assert rc == 0, f"{what} returned {rc}"


class Harness:
    def __init__(self, lib, arg_lanes):
        self.lib, self.arg_lanes = lib, arg_lanes
        lib.db_build_id.restype = ctypes.c_char_p
        lib.db_fp.argtypes = [ctypes.c_int, ctypes.c_int, U32P, I32P, U32P, I32P]
        lib.db_lazy.argtypes = [ctypes.c_int, ctypes.c_int, U32P, U32P]
        for k in range(3):
            getattr(lib, "db_grp%d" % k).argtypes = [ctypes.c_int, ctypes.c_int, U32P, U32P, U32P, I32P]

    @staticmethod
    def _pack(values):
        """stored words of a flat list of integers"""
        return np.frombuffer(b"".join(v.to_bytes(48, "little") for v in values), dtype=np.uint32).copy()

    @staticmethod
    def _unpack(arr):
        raw = arr.tobytes()
        return [int.from_bytes(raw[i:i + 48], "little") for i in range(0, len(raw), 48)]

    def fp(self, op, cases, flags=None):
        """cases: [(a0, a1, b0, b1)] -> ([(r0, r1)], [aux])"""
        n = len(cases)
        inp = self._pack([v for c in cases for v in c])
        fl = np.array(flags if flags is not None else [0] * n, dtype=np.int32)
        out, aux = np.zeros(24 * n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
        rc = self.lib.db_fp(A_OPS[op], n, inp.ctypes.data_as(U32P), fl.ctypes.data_as(I32P),
                            out.ctypes.data_as(U32P), aux.ctypes.data_as(I32P))
        _ok(rc, f"db_fp({op})")
        v = self._unpack(out)
        return list(zip(v[::2], v[1::2])), [int(x) for x in aux]

    def lazy(self, op, cases):
        """cases: [up to twelve limb lists] -> array [thread][6][14] of what every lane holds"""
        n = len(cases)
        inp = np.zeros((n, 12, 14), dtype=np.uint32)
        for i, c in enumerate(cases):
            inp[i, :len(c)] = np.array(c, dtype=np.uint64).astype(np.uint32)
        threads = self.lib.db_lazy_threads(B_OPS[op], n)
        assert threads > 0
        out = np.zeros((threads, 6, 14), dtype=np.uint32)
        rc = self.lib.db_lazy(B_OPS[op], n, inp.ctypes.data_as(U32P), out.ctypes.data_as(U32P))
        _ok(rc, f"db_lazy({op})")
        return out

    def grp(self, group, op, A, Bv=None):
        """A, Bv: [raw lanes (3 x 4 integers)] -> ([per lane: 4 integers], [per lane: flag])"""
        kind = GROUPS[group][0]
        n = len(A)
        Bv = Bv if Bv is not None else A
        a = self._pack([v for val in A for lane in val for v in lane])
        b = self._pack([v for val in Bv for lane in val for v in lane])
        lanes = getattr(self.lib, "db_grp%d_lanes" % kind)(n)
        assert lanes > 0
        out, flag = np.zeros(48 * lanes, dtype=np.uint32), np.zeros(lanes, dtype=np.int32)
        rc = getattr(self.lib, "db_grp%d" % kind)(C_OPS[op], n, a.ctypes.data_as(U32P), b.ctypes.data_as(U32P),
                                                  out.ctypes.data_as(U32P), flag.ctypes.data_as(I32P))
        _ok(rc, f"db_grp{kind}({op})")
        v = self._unpack(out)
        return [tuple(v[4 * t:4 * t + 4]) for t in range(lanes)], [int(x) for x in flag]


@pytest.fixture(scope="module", params=["64", "128"])
def db(request):
    """The harness of one build, loaded only if it was built from this tree (its embedded id);
    otherwise built now, and a failure of that fails the tests."""
    from gpu_helpers import harness
    which = request.param
    lib = harness.load_devblocks(which)
    h = Harness(lib, int(which))
    assert lib.db_arg_lanes() == int(which)
    return h


@pytest.fixture(scope="module")
def hc():
    from gpu_helpers import harness
    return harness.load("hostcheck")


def _launches(cases, size, extra=(1,)):
    """The case list cut into launches of `size` (the last one filled up from the front of the list),
    then one launch of each extra shape on a slice that moves through the list; yields
    (indices into cases)."""
    n = len(cases)
    for start in range(0, n, size):
        yield [(start + i) % n for i in range(size)]
    for j, shape in enumerate(extra):
        start = (n // 2 + 7 * j) % n
        yield [(start + i) % n for i in range(shape)]


# ---- A. stored words ---------------------------------------------------------------------------
def _want_fp(op, c):
    a0, a1, b0, b1 = c
    return {"add": (a0 + b0, 0), "sub": (a0 - b0, 0), "neg": (-a0, 0),
            "mul": (a0 * b0 * R.R392_INV, 0), "sqr": (a0 * a0 * R.R392_INV, 0),
            "mul28": (a0 * b0 * R.R392_INV, 0), "sqr28": (a0 * a0 * R.R392_INV, 0),
            "f2mul": ((a0 * b0 - a1 * b1) * R.R392_INV, (a0 * b1 + a1 * b0) * R.R392_INV),
            "f2sqr": ((a0 * a0 - a1 * a1) * R.R392_INV, 2 * a0 * a1 * R.R392_INV)}[op]


def _run_fp(db, op, cases, want, flags=None):
    compared = set()
    for idx in _launches(cases, 133):
        out, _ = db.fp(op, [cases[i] for i in idx], [flags[i] for i in idx] if flags else None)
        for i, (r0, r1) in zip(idx, out):
            w0, w1 = want(cases[i], i)
            assert r0 < 2 * P and r1 < 2 * P, (op, i, cases[i])
            assert r0 % P == w0 % P and r1 % P == w1 % P, (op, i, cases[i], r0, r1)
            compared.add(i)
    assert len(compared) == len(cases)


@pytest.mark.parametrize("op", ["add", "sub", "neg", "mul", "sqr", "mul28", "sqr28"])
def test_fp_ops(db, op):
    """fp.h's carry chains (__builtin_addc / __builtin_subc) and the out-of-line Fp leaves
    (fp_mul_leaf, fp_sqr_leaf, fp_mul28_leaf, fp_sqr28_leaf) on every pair of edge values and 300
    random pairs below 2p: exact residue, result below 2p; 133-case launches (two waves and five
    lanes; in the 128 build one 128-thread workgroup and five lanes) and a one-case launch"""
    cases = [(a, 0, b, 0) for a, b in R.fp_pairs()]
    _run_fp(db, op, cases, lambda c, i: _want_fp(op, c))


@pytest.mark.parametrize("op", ["f2mul", "f2sqr"])
def test_fp2_products(db, op):
    """fp2_mul_pair / fp2_sqr_pair (fp2_mul_leaf's second operand through the per-lane LDS slot,
    the signed real part and its (int64_t)acc < 0 correction) on test_fp2_mul_lazy_bounds's
    operands, the sign-deciding combinations and random values"""
    _run_fp(db, op, R.fp2_quads(), lambda c, i: _want_fp(op, c))


@pytest.mark.parametrize("mode", ["pos", "neg", "alt", "alt_inv"])
def test_fp_dot2(db, mode):
    """pair6.h fp_dot2 = a0 b0 +- a1 b1 with the sign a per-lane operand: every lane adding, every
    lane subtracting, and neighbouring lanes differing (as the two halves of a Grp6 role do)"""
    cases = R.fp2_quads()
    flags = [{"pos": 0, "neg": 1, "alt": i & 1, "alt_inv": (i & 1) ^ 1}[mode] for i in range(len(cases))]

    def want(c, i):
        a0, a1, b0, b1 = c
        return ((a0 * b0 - a1 * b1 if flags[i] else a0 * b0 + a1 * b1) * R.R392_INV, 0)
    _run_fp(db, "dot2", cases, want, flags)


def _hc_batches(hc, raw):
    """the batches the host build of fp_inv runs for this raw (Montgomery) value"""
    hc.hc_fp_inv.argtypes = [ctypes.c_char_p, ctypes.c_char_p, I32P, I32P]
    out, nb, nct = ctypes.create_string_buffer(144), ctypes.c_int(0), ctypes.c_int(0)
    hc.hc_fp_inv(R.unmont(raw).to_bytes(48, "big"), out, ctypes.byref(nb), ctypes.byref(nct))
    return nb.value


@pytest.fixture(scope="module")
def inv_waves(hc):
    """[(name, 64 raw values)]: fp_inv's divstep loop ends for the whole wave at once"""
    rng = random.Random(31)
    rnd = [rng.randrange(P) for _ in range(2000)]
    nb = [_hc_batches(hc, x) for x in rnd]
    slow, fast = rnd[nb.index(max(nb))], rnd[nb.index(min(nb))]
    assert max(nb) > min(nb)
    fill = [rng.randrange(2 * P) for _ in range(64)]
    waves = [("distinct", R.inv_values()), ("all_zero", [0] * 64),
             ("one_value_among_zeros", [0] * 37 + [rnd[0]] + [0] * 26),
             ("one_zero_among_values", fill[:22] + [0] + fill[23:]),
             ("one_p_among_values", fill[:63] + [P])]
    w = list(fill)
    w[30], w[31] = slow, fast
    waves.append(("slow_next_to_fast", w))
    w = list(fill)
    w[0], w[63] = slow, fast
    waves.append(("slow_0_fast_63", w))
    w = [fast] * 64
    w[63], w[0] = slow, fast
    waves.append(("fast_wave_slow_63", w))
    return waves


def test_fp_inv_waves(db, hc, inv_waves):
    """fp_inv / fp_inv_ct on whole waves of chosen values: the raw result is R^2 / a (0 and p map
    to 0) below 2p, both versions agree, a lane that is done is not disturbed by the batches it runs
    until the slowest lane finishes, every lane reports the wave's batch count (at most 40; the
    host build's largest count of the wave's values), fp_inv_ct always 40"""
    compared = 0
    for name, wave in inv_waves:
        cases = [(a, 0, 0, 0) for a in wave]
        out, nb = db.fp("inv", cases)
        out_ct, nb_ct = db.fp("invct", cases)
        for a, (r, _), (rc, _) in zip(wave, out, out_ct):
            want = pow(a, -1, P) * R.RM * R.RM % P if a % P else 0
            assert r % P == want and rc % P == want, (name, a)
            assert r < 2 * P and rc < 2 * P
            compared += 1
        assert len(set(nb)) == 1 and nb[0] <= 40, (name, nb)
        assert nb[0] == max(_hc_batches(hc, a) for a in wave), name
        assert nb_ct == [40] * 64, name
    assert compared == 64 * len(inv_waves)


# ---- B. lazy limbs -----------------------------------------------------------------------------
ZERO = [0] * 14


def _lazy_want(op, c):
    """[(numerator of the result times R, integer cap of that numerator)] for the outputs r0, r1, ..."""
    v = [R.lvalue(x) for x in c] + [0] * (12 - len(c))
    k2n = 33 * P

    def f2m(a0, a1, b0, b1):
        return [(a0 * b0 - a1 * b1, a0 * b0 + (k2n - a1) * b1), (a0 * b1 + a1 * b0,) * 2]

    def f2s(a0, a1, s):
        return [(a0 * a0 - a1 * a1, (a0 + a1) * (a0 + s * P - a1)), (2 * a0 * a1,) * 2]
    if op in ("lmul",):
        return [(v[0] * v[1],) * 2]
    if op == "lsqr":
        return [(v[0] * v[0],) * 2]
    if op in ("lmul2", "h_pmul2"):
        return [(v[0] * v[1],) * 2, (v[2] * v[3],) * 2]
    if op in ("lsqr2", "h_psqr2"):
        return [(v[0] * v[0],) * 2, (v[1] * v[1],) * 2]
    if op == "ldot":
        return [(v[0] * v[2] + v[1] * v[3],) * 2]
    if op in ("f2mul", "h_fm"):
        return f2m(*v[:4])
    if op in ("f2sqr36", "h_fs36"):
        return f2s(v[0], v[1], 36)
    if op in ("f2sqr78", "h_fs78"):
        return f2s(v[0], v[1], 78)
    if op == "f2sqr9":
        return f2s(v[0], v[1], 9)
    if op == "x_fm3":
        return f2m(*v[0:4]) + f2m(*v[4:8]) + f2m(*v[8:12])
    if op == "x_fm2":
        return f2m(*v[0:4]) + f2m(*v[4:8])
    if op == "x_fs3":
        return f2s(v[0], v[1], 9) + f2s(v[2], v[3], 9) + f2s(v[4], v[5], 9)
    raise KeyError(op)


def _group_of(cases, k, seed):
    """cases of k operand sets each: case i joined with k - 1 others (a fixed shuffle)"""
    rng = random.Random(seed)
    others = [rng.sample(range(len(cases)), len(cases)) for _ in range(k - 1)]
    return [sum((list(cases[o[i]]) for o in others), list(cases[i])) for i in range(len(cases))]


@pytest.fixture(scope="module")
def lazy_cases():
    """{operation: operand sets}, each set already admitted by lazy28.py's model (blocks_ref)"""
    mul, sqr = R.mul_cases("Fp"), [(a,) for a in R.sqr_cases("Fp")]
    f2m = R.f2mul_cases()
    sq = {st: R.f2sqr_cases(st) for st in R.SQR_SITES}
    return {"lmul": mul, "lsqr": sqr, "lmul2": _group_of(mul, 2, 1), "lsqr2": _group_of(sqr, 2, 2),
            "f2mul": f2m, "f2sqr36": sq[(36, 1)], "f2sqr78": sq[(78, 1)], "f2sqr9": sq[(9, 2)],
            "ldot": R.dot_cases(),
            "h_fm": f2m, "h_fs36": sq[(36, 1)], "h_fs78": sq[(78, 1)],
            "h_pmul2": _group_of(mul, 2, 3), "h_psqr2": _group_of(sqr, 2, 4),
            "x_fm3": _group_of(f2m, 3, 5), "x_fm2": _group_of(f2m, 2, 6), "x_fs3": _group_of(sq[(9, 2)], 3, 7)}


def _lanes_of(op, j):
    """the threads that hold case j of a launch"""
    if op.startswith("h_"):
        return [2 * j, 2 * j + 1]
    if op.startswith("x_"):
        return [64 * (j // 9) + 6 * (j % 9) + s for s in range(6)]
    return [j]


LAZY_SHAPES = {"": (133, (1,)), "h": (33, (1,)), "x": (19, (10, 9, 1))}


@pytest.mark.parametrize("op", list(B_OPS))
def test_lazy_products(db, lazy_cases, op):
    """ec28.h's lazy-limb products on admitted normalised and un-normalised patterns (l_add, l_shl,
    l_sub<S, T>; the worst-case pattern with the largest column sum first): the one-lane leaves
    (l_mul, l_sqr, the dual-chain l_mul2 / l_sqr2, f2l_mul, f2l_sqr_k, l_dot), the lane-pair
    policies F2Half / G1Half (h_*: 33-pair and one-pair launches) and the six-lane F2Hex (x_*: 19,
    10, 9 and 1 role).  Every lane of a pair / role must hold the same normalised result, congruent
    to the integer result and below the model's bound."""
    cases = lazy_cases[op]
    size, extra = LAZY_SHAPES[op[0] if op[1] == "_" else ""]
    compared = set()
    for idx in _launches(cases, size, extra):
        out = db.lazy(op, [cases[i] for i in idx])
        for j, i in enumerate(idx):
            want = _lazy_want(op, cases[i])
            held = [out[t].tolist() for t in _lanes_of(op, j)]
            assert all(h == held[0] for h in held), (op, i, "the lanes of a pair / role differ")
            for r, (num, cap) in zip(held[0], want):
                R.check_lazy(r, num, cap)
            assert all(r == ZERO for r in held[0][len(want):])
            compared.add(i)
    assert len(compared) == len(cases)


# ---- C. lane groups ----------------------------------------------------------------------------
GROUP_SHAPES = {"Grp": (1, 21, 22, 43), "Grp6": (1, 10, 11, 21), "Grp18": (1, 3, 4, 7)}


@pytest.fixture(scope="module")
def group_ref():
    """The case lists of the lane-group tests and the oracle's result for each, computed once."""
    rng = random.Random(22)
    vals = R.group_values()
    polys = [R.raw_to_poly(raw) for _, raw in vals]
    ref = {"vals": vals, "polys": polys}
    ref["sqr"] = [B._p12_mul(f, f) for f in polys]
    partners = polys[1:] + polys[:1]
    ref["mul_b"] = [raw for _, raw in vals[1:] + vals[:1]]
    ref["mul"] = [B._p12_mul(f, g) for f, g in zip(polys, partners)]
    ref["conj"] = [R.p12_conj(f) for f in polys]
    ref["frob1"] = [B._p12_pow(f, P) for f in polys]
    ref["frob2"] = [B._p12_pow(f, P * P) for f in polys]
    # lines (a0, a1, b1): the unit line, a1 = b1 = 0, random ones, in both representatives
    def f2r():
        return (rng.randrange(2 * P), rng.randrange(2 * P))
    lines = [((R.RM, 0), (0, 0), (0, 0)), ((R.RM + P, P), (P, P), (P, P)), (f2r(), (0, 0), (0, 0)),
             (f2r(), (P, 0), (0, P)), (f2r(), f2r(), f2r()), (f2r(), f2r(), f2r()), ((R.TOP,) * 2,) * 3]
    assert len(lines) == len(vals)
    ref["line_b"] = [[l[0] + l[1], l[2] + (0, 0), (0, 0, 0, 0)] for l in lines]  # a LineEntry's 72 words first
    ref["mul_line"] = [B._p12_mul(f, R.line_poly(*[tuple(R.unmont(v) for v in c) for c in l]))
                       for f, l in zip(polys, lines)]
    # cyclotomic elements f^((p^6 - 1)(p^2 + 1)), in both representatives, and one
    cyc = [B._p12_pow(f, R.CYC_EXP) for f in polys[:2]]
    ref["cyc_in"] = [R.poly_to_raw(cyc[0]), R.poly_to_raw(cyc[0], upper=True), R.poly_to_raw(cyc[1]),
                     R.poly_to_raw(B.P12_ONE), R.poly_to_raw(B.P12_ONE, upper=True)]
    ref["cyc"] = [B._p12_mul(c, c) for c in (cyc[0], cyc[0], cyc[1], B.P12_ONE, B.P12_ONE)]
    # final exponentiation: random and extreme values (not one), and elements of the proper subfield
    # Fp6 (tower c1 = 0: z1 = z3 = z5 = 0), which give one
    sub = []
    for _ in range(2):
        z = {i: (rng.randrange(P), rng.randrange(P)) for i in (0, 2, 4)}
        lanes = [z[0] + (0, 0), (0, 0) + z[4], z[2] + (0, 0)]  # A_k = (z_k, z_{k+3})
        sub.append([tuple(R.mont(v, upper=bool(len(sub))) for v in lane) for lane in lanes])
    fe_in = [vals[0][1], vals[1][1], vals[5][1], vals[6][1], vals[3][1]] + sub
    ref["fexp_in"] = fe_in
    ref["fexp"] = [B._p12_pow(R.raw_to_poly(raw), R.FEXP3) for raw in fe_in]
    assert [f == B.P12_ONE for f in ref["fexp"]] == [False] * 4 + [True] * 3
    return ref


def _check_groups(db, group, op, A, want, Bv=None, want_flag=None, check=None):
    """Run op over every shape of the group with the case list rotated through the units -- every
    case passes through the first and the last group of a wave and through a launch whose other
    groups shadow it -- and compare what EVERY lane of every unit holds."""
    _, lanes_per, per_wave = GROUPS[group]
    L = len(A)
    compared = set()
    for n in GROUP_SHAPES[group]:
        for rot in range(L):
            idx = [(u + rot) % L for u in range(n)]
            out, flag = db.grp(group, op, [A[i] for i in idx], [Bv[i] for i in idx] if Bv else None)
            for u, i in enumerate(idx):
                base = 64 * (u // per_wave) + lanes_per * (u % per_wave)
                per_role = lanes_per // 3
                got = []
                for k in range(3):
                    held = [out[base + per_role * k + s] for s in range(per_role)]
                    assert all(h == held[0] for h in held), (group, op, n, u, "the lanes of a role differ")
                    assert all(v < 2 * P for v in held[0]), (group, op, n, u)
                    got.append(tuple(R.unmont(v) for v in held[0]))
                fl = flag[base:base + lanes_per]
                assert len(set(fl)) == 1, (group, op, n, u, "the lanes of a group differ in their verdict")
                if check:
                    check(i, R.lanes_to_poly(got))
                elif want is not None:
                    assert R.lanes_to_poly(got) == want[i], (group, op, n, u, i)
                if want_flag is not None:
                    assert fl[0] == int(want_flag[i]), (group, op, n, u, i)
                compared.add((n, rot, u))
    assert len(compared) == L * sum(GROUP_SHAPES[group])


@pytest.mark.parametrize("op", ["sqr", "mul", "mul_line", "conj", "frob1", "frob2"])
@pytest.mark.parametrize("group", list(GROUPS))
def test_group_lazy_ops(db, group_ref, group, op):
    """pair28.h's lane operations (g4_sqr, g4_mul, g4_mul_line, g4_conj, g4_frob<1>, g4_frob<2>)
    over Grp, Grp6 and Grp18 against the oracle's Fp12: random values, one in both representatives,
    all coordinates p - 1 and all 2p - 1; lines: the unit line, a1 = b1 = 0, random ones"""
    A = [raw for _, raw in group_ref["vals"]]
    Bv = {"mul": group_ref["mul_b"], "mul_line": group_ref["line_b"]}.get(op)
    _check_groups(db, group, op, A, group_ref[op], Bv)


@pytest.mark.parametrize("group", list(GROUPS))
def test_group_cyclotomic_square(db, group_ref, group):
    """g4_cyc (Granger-Scott) on elements of the cyclotomic subgroup, where it is defined"""
    _check_groups(db, group, "cyc", group_ref["cyc_in"], group_ref["cyc"])


@pytest.mark.parametrize("group", list(GROUPS))
def test_group_final_exp(db, group_ref, group):
    """g4_final_exp = f^(3 (p^12 - 1) / r) and g4_is_one of the result: random and extreme inputs
    (not one), elements of the proper subfield Fp6 (one)"""
    want = group_ref["fexp"]
    _check_groups(db, group, "fexp", group_ref["fexp_in"], want, want_flag=[f == B.P12_ONE for f in want])


@pytest.mark.parametrize("op,group", [("is_one", "Grp"), ("is_one", "Grp6"), ("is_one", "Grp18"),
                                      ("s_is_one", "Grp"), ("s_is_one", "Grp6")])
def test_group_is_one(db, group, op):
    """g4_is_one over the three groups, g_is_one and g6_is_one: one in both representatives (p + R
    for 1, p for 0), and one changed in a single coordinate of a single role"""
    cases = R.is_one_values()
    A = [raw for _, raw, _ in cases]
    _check_groups(db, group, op, A, [R.raw_to_poly(raw) for raw in A], want_flag=[one for _, _, one in cases])


def test_group_stored_mul(db, group_ref):
    """pair3.h g_mul in stored words (k_pair3<P3_PROD>'s product tree)"""
    A = [raw for _, raw in group_ref["vals"]]
    _check_groups(db, "Grp", "s_mul", A, group_ref["mul"], group_ref["mul_b"])


@pytest.mark.parametrize("group", ["Grp", "Grp6"])
def test_group_stored_inv(db, group_ref, group):
    """g_inv / g6_inv: f times the result is one in the oracle's Fp12; 0 gives 0, as fp_inv does"""
    A = [raw for _, raw in group_ref["vals"]] + [[(0,) * 4] * 3, [(P,) * 4] * 3]
    polys = [R.raw_to_poly(raw) for raw in A]

    def check(i, got):
        if any(polys[i]):
            assert B._p12_mul(polys[i], got) == B.P12_ONE, (group, i)
        else:
            assert got == [0] * 12, (group, i)
    _check_groups(db, group, "s_inv", A, None, check=check)
