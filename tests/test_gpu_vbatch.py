"""The combination and verdict kernels of the batched verification (vbatch.hip, and the verdict
kernels at the end of vgroup.hip) on the GPU, one launcher at a time, against Python integers.

This is the code between the arithmetic layers: it takes decompressed points and a secret key and
yields combined points and per-item status bytes.  The soundness of the batched check lives here --
every item its own coefficient r_i = a_i + b_i lambda from SHA-256(key || position), the same r_i on
the key and on the signature, no item left out of a sum, no ST_OK for an item whose group did not
pass -- and a mistake in it does not show on honest data.  The test-only vb harness
(tests/native/devblocks_vbatch.hip, a library of its own that compiles the product's vbatch.hip
itself) and four entry points of the pair harness (devblocks_vgroup.hip) run one product launcher, or
one launcher sequence the product issues, per call; every output array is pre-filled with a sentinel
and copied back in full, so the entries a kernel must not write are compared too.

References (tests/blocks_ref.py, held against the host check by tests/test_blocks_ref.py; the code
under test is never the reference): the coefficients are hashlib's SHA-256; every key is a known
multiple k_i G1 and every signature k_i Q for one fixed Q of order r, so [r_i] of an item and the sum
over any set are ONE fixed-base multiplication [(sum r_i k_i) mod r] of the base -- which also pins
lambda on both curves.  All comparisons are exact: Montgomery Jacobian records are decoded to affine
group elements, every stored coordinate must be below 2p and infinity must have Z = 0.  There is no
tolerance anywhere in this file.

Not reachable: the `(a | b) == 0 -> a = 1` line of rlc_coeffs needs a digest whose first 64 bits are
zero, i.e. a hash preimage; it is not tested and not faked.

Which shape reaches which branch:
  k_item_group   n = 1 / 64 / 65, grp_off null and given (empty groups among them).
  k_rlc          n = 1 / 64 / 65 in groups of 1, 2, 3, 17; sides 3, and 1 then 2 through coef; key_base
                 0 and n; `always`; grp_off null; each unusable flag alone; sig null; guard 0; the
                 entries past n; ladder tables for some keys (elements identical, exact counters).
  k_plan_*       group sizes from {0, 1, 2, 15, 16, 17, 31, 32, 33, 100}, cmax 1 / 2 / 3 / 16; the scan at
                 ng = 1 / 64 / 65 / 1023 / 1024 / 1025 / 2049 / 5000.
  k_rlc_msm      dense sides 3, dense 1 then 2, sparse 3, sparse 1, dense 1 with tables; cmax 2 / 16;
                 groups of 1, 2, 16, 17, 40; a poisoned chunk of 16 (the unusable item first / middle /
                 last, with the decompression's placeholder and with zero coordinates), a chunk of
                 unusable items only, a chunk holding one key twice; lanes past *total; guard 0.
  k_scatter      every decode / inf flag, every kind of group verdict, groups of one and more, with and
                 without aggregates, first_group null / equal / before / after; n = 1 / 64 / 65 / 200.
  verdicts       ng = 1 / 63 / 64 / 65 / 130, fe_batch 1 / 4 / 64, first-error mode, g0 > 0, the guard.
  FastAggregate  k_seg_sum (affine, Jacobian), k_va_point, k_va_status, k_fb_lines, k_sig_lines.
"""
import ctypes
import itertools
import random

import numpy as np
import pytest

import blocks_ref as R
from oracle import bls12381 as B

pytestmark = pytest.mark.gpu

P = B.P
SENT32, SENT8 = 0xC3A5C3A5, 0xEE  # a sentinel "value" is above 2p, a sentinel byte is no status
DB_E_ARG = -1
W_RLC = ["sides", "always", "n", "n_buf", "key_base", "guard", "n_groups", "n_wide"]
A_RLC = ["pk", "pk_st", "sig", "sig_st", "item_grp", "grp_off", "pout", "sout", "coef", "went", "wide_pk", "ctr"]
W_MSM = ["sides", "then2", "sparse", "always", "n_buf", "ng", "cmax", "key_base", "guard", "cap", "n_wide"]
A_MSM = ["grp_off", "pk", "pk_st", "sig", "sig_st", "pout", "sout", "coef", "coef4", "cnt", "coff", "cfirst", "ccount", "went",
         "wide_pk", "ctr"]
W_SC = ["n", "n_buf", "n_groups", "n_msgs", "n_agg", "agg_buf", "list_len", "has_first", "first"]
A_SC = ["item_grp", "msg_idx", "hm", "pk", "pk_st", "sig", "sig_st", "gverdict", "grp_off", "ta_status", "agg_pk", "agg_pk_st",
        "agg_sig", "agg_status", "status", "list", "count"]
CTR = ["hits", "misses", "size", "wide_built", "wide_chunks", "narrow_chunks", "wide_items", "narrow_items"]


def _ok(rc, what):
    """A failed launch or synchronise (devblocks.h DB_E_LAUNCH, DB_E_SYNC) is a GPU error: the run
    ends there, nothing more is started on the card."""
    if rc in (-5, -6):
        pytest.exit(f"{what} returned {rc}: the GPU reported an error; no further block test is run", returncode=3)
    assert rc == 0, f"{what} returned {rc}"


def _u32(a, width=None):
    a = np.ascontiguousarray(np.array(a, dtype=np.uint64).astype(np.uint32))
    return a.reshape(-1, width) if width else a


def _u8(a):
    return np.ascontiguousarray(np.array(list(a), dtype=np.uint8))


def _sent32(*shape):
    return np.full(shape, SENT32, dtype=np.uint32)


def _sent8(n):
    return np.full(n, SENT8, dtype=np.uint8)


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def untouched(a):
    a = np.asarray(a)
    return bool((a == (SENT8 if a.dtype == np.uint8 else SENT32)).all())


def _offsets(sizes):
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    return off


class VB:
    def __init__(self, lib, pair):
        self.lib, self.pair = lib, pair
        c = (ctypes.c_uint32 * 19)()
        assert lib.db_vb_consts(c) == 19
        c = list(c)
        assert c[:4] == [4 * 28, 4 * R.HM_WORDS, 4 * 36, 4 * 72] and c[4:7] == [4 * R.MSG_WORDS, 4 * R.LINE_WORDS, R.N_LINES]
        self.NONE, digits, self.RLC_CHUNK = c[7], c[8], c[9]
        assert digits == R.SPARSE_DIGITS and c[18] == 8 * len(CTR)
        self.ST_OK, self.ST_BAD_PUBKEY, self.ST_BAD_SIGNATURE, self.ST_NOT_VERIFIED, self.ST_UNCHECKED = c[10:15]
        assert c[10:14] == [B.ST_OK, B.ST_BAD_PUBKEY, B.ST_BAD_SIGNATURE, B.ST_NOT_VERIFIED]
        self.GV_PASS, self.GV_UNCHECKED, self.GV_NOT_READY = c[15:18]
        assert (lib.db_vb_rlc_words(), lib.db_vb_rlc_ptrs()) == (len(W_RLC) + 8, len(A_RLC))
        assert (lib.db_vb_rlc_msm_words(), lib.db_vb_rlc_msm_ptrs()) == (len(W_MSM) + 8, len(A_MSM))
        assert (lib.db_vb_scatter_words(), lib.db_vb_scatter_ptrs()) == (len(W_SC), len(A_SC))
        st = (ctypes.c_uint32 * 3)()
        pair.db_group_states(st)
        self.G_READY, self.G_FALLBACK, self.G_EMPTY = list(st)
        V, U = ctypes.c_void_p, ctypes.c_uint32
        lib.db_vb_item_group.argtypes = [V, U, U, V, U]
        for f in (lib.db_vb_rlc, lib.db_vb_rlc_msm, lib.db_vb_scatter):
            f.argtypes = [V, V]
        lib.db_vb_plan.argtypes = [V, U, U, U, V, V, V, V]
        lib.db_vb_scan.argtypes = [V, U, V]
        lib.db_vb_fb_lines.argtypes = [V, U, U, U, U, V, U, V, U, V]
        lib.db_vb_sig_lines.argtypes = [V, U, V, U, U]
        lib.db_vb_seg_sum.argtypes = [ctypes.c_int, V, V, U, V, U, V, V, U]
        lib.db_vb_va_point.argtypes = [V, U, V, U, V, U]
        lib.db_vb_va_status.argtypes = [V, V, V, U, V, V, U, V, U]
        pair.db_batch_verdict.argtypes = [U, V, V, U, U, V, U, V, U, V, ctypes.c_int, V, U]
        pair.db_slot_verdict.argtypes = [U, V, V, V, U]
        pair.db_first_group.argtypes = [V, U, V]
        pair.db_first_item.argtypes = [V, U, V]

    @staticmethod
    def _call(f, what, names_w, names_a, w, a, key=None, rc=0):
        wa = _u32([w[k] for k in names_w] + (list(key) if key is not None else []))
        pa = (ctypes.c_void_p * len(names_a))(*[_ptr(a.get(k)) for k in names_a])
        got = f(_ptr(wa), pa)
        if rc:
            assert got == rc, (what, got, rc)
        else:
            _ok(got, what)

    def item_group(self, grp_off, n, n_buf, rc=0):
        out = _sent32(n_buf)
        off = None if grp_off is None else _u32(grp_off)
        got = self.lib.db_vb_item_group(_ptr(off), 0 if off is None else len(off) - 1, n, _ptr(out), n_buf)
        if rc:
            assert got == rc
        else:
            _ok(got, "db_vb_item_group")
        return out

    def rlc(self, key, it, n, sides=3, always=0, key_base=0, sizes=None, coef=None, guard=None, keys_only=False, went=None,
            wide_pk=None, rc=0):
        """-> dict(pout, sout, coef, ctr); it: Items; sizes: the group sizes (None: grp_off null)"""
        nb = len(it.pk)
        a = dict(pk=it.pk, pk_st=it.pk_st, sig=None if keys_only else it.sig, sig_st=None if keys_only else it.sig_st)
        w = dict(sides=sides, always=always, n=n, n_buf=nb, key_base=key_base, guard=2 if guard is None else guard, n_groups=0,
                 n_wide=0)
        if sizes is not None:
            off = _offsets(sizes)
            a["grp_off"] = _u32(off)
            a["item_grp"] = _u32([g for g, s in enumerate(sizes) for _ in range(s)] + [0] * (nb - off[-1]))
            w["n_groups"] = len(sizes)
        a["pout"] = _sent32(nb, 36) if sides & 1 else None
        a["sout"] = _sent32(nb, 72) if sides & 2 else None
        a["coef"] = _sent32(nb, 2) if coef is None else coef.copy()
        if went is not None:
            a["went"], a["wide_pk"], a["ctr"] = _u32(went), wide_pk, np.zeros(len(CTR), dtype=np.uint64)
            w["n_wide"] = len(wide_pk)
        self._call(self.lib.db_vb_rlc, "db_vb_rlc", W_RLC, A_RLC, w, a, key, rc)
        return a

    def plan(self, grp_off, cmax, cap, rc=0):
        ng = len(grp_off) - 1
        out = [_sent32(ng), _sent32(ng + 1), _sent32(cap), _sent32(cap)]
        off = _u32(grp_off)
        got = self.lib.db_vb_plan(_ptr(off), ng, cmax, cap, *[_ptr(o) for o in out])
        if rc:
            assert got == rc
        else:
            _ok(got, "db_vb_plan")
        return out

    def scan(self, cnt):
        off, src = _sent32(len(cnt) + 1), _u32(cnt)
        _ok(self.lib.db_vb_scan(_ptr(src), len(cnt), _ptr(off)), "db_vb_scan")
        return off

    def rlc_msm(self, key, it, sizes, cmax, sides=3, then2=0, sparse=0, always=0, key_base=0, guard=None, went=None,
                wide_pk=None, rc=0):
        nb, off = len(it.pk), _offsets(sizes)
        cap = off[-1] // cmax + len(sizes) + 3
        a = dict(grp_off=_u32(off), pk=it.pk, pk_st=it.pk_st, sig=it.sig, sig_st=it.sig_st, pout=_sent32(nb, 36),
                 sout=_sent32(nb, 72), coef=_sent32(nb, 2), coef4=_sent32(nb, 4), cnt=_sent32(len(sizes)),
                 coff=_sent32(len(sizes) + 1), cfirst=_sent32(cap), ccount=_sent32(cap))
        w = dict(sides=sides, then2=then2, sparse=sparse, always=always, n_buf=nb, ng=len(sizes), cmax=cmax, key_base=key_base,
                 guard=2 if guard is None else guard, cap=cap, n_wide=0)
        if went is not None:
            a["went"], a["wide_pk"], a["ctr"] = _u32(went), wide_pk, np.zeros(len(CTR), dtype=np.uint64)
            w["n_wide"] = len(wide_pk)
        self._call(self.lib.db_vb_rlc_msm, "db_vb_rlc_msm", W_MSM, A_MSM, w, a, key, rc)
        return a

    def scatter(self, a, n, n_groups, n_agg, first=None, rc=0):
        w = dict(n=n, n_buf=len(a["status"]), n_groups=n_groups, n_msgs=len(a["hm"]), n_agg=n_agg,
                 agg_buf=0 if a.get("agg_status") is None else len(a["agg_status"]), list_len=len(a["list"]),
                 has_first=0 if first is None else 1, first=first or 0)
        self._call(self.lib.db_vb_scatter, "db_vb_scatter", W_SC, A_SC, w, a, None, rc)


@pytest.fixture(scope="module")
def vb():
    """The vb harness and the pair harness (the verdict kernels are vgroup.hip's), each loaded only if
    it was built from this tree (its embedded id); otherwise built now, and a failure of that fails the
    tests with the id in the message."""
    from gpu_helpers import harness
    return VB(harness.load_devblocks("vb"), harness.load_devblocks("pair"))


# ---- the world: keys k_i G1, signatures k_i Q ---------------------------------------------------
def g1a(pt, inf=False):
    w = R.affine_entry(1, pt)
    w[24] = 1 if (inf or pt is None) else 0
    return w


def hme(pt, inf=False):
    w = R.affine_entry(2, pt)
    w[48] = 1 if (inf or pt is None) else 0
    return w


# what makes an item unusable.  A flag alone sits on an otherwise good record; the placeholders are what
# the decompression leaves for a rejected input: k_dec_pk / k_g1_subgroup the generator with its status
# set, k_dec_sig_pt / k_g2_subgroup zero coordinates with inf and the status set; "zero": zero
# coordinates with the inf flag and a clear status (a decoded point at infinity; k_pk_cached's form)
PK_KINDS = ("pk_st", "pk_inf", "pk_ph", "pk_zero")
SIG_KINDS = ("sig_st", "sig_inf", "sig_ph", "sig_zero")


class Items:
    """specs: per item (key number, kind) with kind None (usable) or one of PK_KINDS / SIG_KINDS;
    padded to n_buf records with usable items of key 0"""

    def __init__(self, vw, specs, n_buf=None):
        self.specs = list(specs)
        pad = [(0, None)] * ((n_buf or len(specs)) - len(specs))
        pk, sig, pst, sst = [], [], [], []
        for ki, kind in self.specs + pad:
            p, s, ps, ss = vw.pkw[ki], vw.sigw[ki], 0, 0
            if kind == "pk_st":
                ps = 1
            elif kind == "pk_inf":
                p = g1a(vw.pk[ki], inf=True)
            elif kind == "pk_ph":
                p, ps = g1a(B.G1_GEN), 1
            elif kind == "pk_zero":
                p = g1a(None)
            elif kind == "sig_st":
                ss = 1
            elif kind == "sig_inf":
                s = hme(vw.sig[ki], inf=True)
            elif kind == "sig_ph":
                s, ss = hme(None), 1
            elif kind == "sig_zero":
                s = hme(None)
            else:
                assert kind is None
            pk.append(p), sig.append(s), pst.append(ps), sst.append(ss)
        self.pk, self.sig, self.pk_st, self.sig_st = _u32(pk, 28), _u32(sig, 52), _u8(pst), _u8(sst)

    def usable(self, i, keys_only=False):
        kind = self.specs[i][1]
        return kind is None or (keys_only and kind in SIG_KINDS)


class World:
    def __init__(self):
        rng = random.Random(20261021)
        self.rng = rng
        self.key = [rng.getrandbits(32) for _ in range(8)]
        self.f1 = R.FixedBase(1, B.G1_GEN)
        self.Q = B.g2_mul(B.G2_GEN, rng.randrange(1, B.R))
        self.f2 = R.FixedBase(2, self.Q)
        self.k = [rng.randrange(1, B.R) for _ in range(48)]
        self.pk = [self.f1.mul(k) for k in self.k]
        self.sig = [self.f2.mul(k) for k in self.k]
        self.pkw = [g1a(p) for p in self.pk]
        self.sigw = [hme(s) for s in self.sig]

    def base(self, field):
        return self.f1 if field == 1 else self.f2


@pytest.fixture(scope="module")
def vw():
    return World()


def decode(field, row):
    """the group element of a Jacobian record (None: Z = 0); every stored coordinate below 2p"""
    w = [int(v) for v in row]
    assert all(R.from_words(w[12 * k:12 * k + 12]) < 2 * P for k in range(3 * field)), "a stored word is not below 2p"
    return R.entry_affine(field, w)


def check_points(vw, field, rows, want_scalars, n):
    """rows[i] is [want_scalars[i]] base (None: infinity) for i < n; the rows past n keep the sentinel"""
    f = vw.base(field)
    for i in range(n):
        want = None if want_scalars[i] is None else f.mul(want_scalars[i])
        assert decode(field, rows[i]) == want, (field, i)
    assert untouched(rows[n:])


# ---- k_item_group -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 64, 65])
def test_item_group(vb, n):
    got = vb.item_group(None, n, n + 2)
    assert list(got[:n]) == list(range(n)) and untouched(got[n:])
    sizes = [s for s in itertools.islice(itertools.cycle([1, 0, 2, 3, 0, 0, 17, 1]), 40)]
    off = _offsets(sizes)
    assert off[-1] >= 65
    got = vb.item_group(off, n, n + 2)
    want = [g for g, s in enumerate(sizes) for _ in range(s)]
    assert list(got[:n]) == want[:n] and untouched(got[n:])


def test_harness_refuses_indices_outside_its_buffers(vb, vw):
    it = Items(vw, [(0, None)] * 4)
    vb.item_group([0, 2, 1, 4], 4, 4, rc=DB_E_ARG)         # offsets not monotone
    vb.item_group([0, 2, 3], 4, 4, rc=DB_E_ARG)            # items beyond the last group
    vb.rlc(vw.key, it, 5, rc=DB_E_ARG)                     # n beyond the buffers
    vb.rlc(vw.key, it, 4, went=[0, 1, 2, 1], wide_pk=_u32([vw.pkw[0]] * 2, 28), sides=1, rc=DB_E_ARG)  # no such table
    vb.rlc(vw.key, it, 4, sides=2, keys_only=True, rc=DB_E_ARG)
    vb.rlc_msm(vw.key, it, [2, 3], 2, rc=DB_E_ARG)         # groups beyond the items
    vb.plan([0, 3, 2], 2, 8, rc=DB_E_ARG)
    vb.plan([0, 3, 9], 2, 4, rc=DB_E_ARG)                  # more chunks than cap
    a = _scatter_arrays(vb, vw, [dict(grp=0, msg=0)] * 2, [vb.GV_PASS], None, 0)
    a["item_grp"][1] = 1
    vb.scatter(a, 2, 1, 0, rc=DB_E_ARG)


# ---- k_rlc --------------------------------------------------------------------------------------
RLC_SIZES = [1, 2, 3, 17]
FLAG_KINDS = {3: "pk_st", 5: "sig_st", 7: "pk_inf", 9: "sig_inf"}  # by i % 11, for n > 1


def _rlc_items(vw, n):
    specs = [(i % len(vw.k), FLAG_KINDS.get(i % 11) if n > 1 else None) for i in range(n)]
    sizes, left = [], n
    for s in itertools.cycle(RLC_SIZES):
        if not left:
            break
        sizes.append(min(s, left))
        left -= sizes[-1]
    return Items(vw, specs, n + 3), sizes


def rlc_expect(vw, it, n, sizes, key_base, always, keys_only=False):
    """per item: ((a, b), the scalar of both outputs or None for infinity) -- the comment above k_rlc"""
    gsize = [1] * n if sizes is None else [s for s in sizes for _ in range(s)]
    out = []
    for i in range(n):
        k = vw.k[it.specs[i][0]]
        if not it.usable(i, keys_only):
            out.append(((0, 0), None))
        elif not always and (sizes is None or gsize[i] <= 1):
            out.append(((1, 0), k))
        else:
            a, b = R.rlc_coeffs(vw.key, key_base + i)
            out.append(((a, b), R.rlc_scalar(a, b) * k % B.R))
    return out


def check_rlc(vw, got, exp, n, sides):
    if sides & 1:
        check_points(vw, 1, got["pout"], [e[1] for e in exp], n)
    if sides & 2:
        check_points(vw, 2, got["sout"], [e[1] for e in exp], n)
    if sides != 2:
        assert [tuple(int(x) for x in r) for r in got["coef"][:n]] == [e[0] for e in exp]
        assert untouched(got["coef"][n:])


@pytest.mark.parametrize("at_n", [False, True])
@pytest.mark.parametrize("n", [1, 64, 65])
def test_rlc_elements(vb, vw, n, at_n):
    """sides 3: [r_i] pk_i and [r_i] sig_i with the SAME r_i, coef the hash's pair; sides 1 then sides 2
    reading coef: the same elements; key_base n (the folded aggregates' launch): item i carries the
    coefficient of stream position n + i, never that of position i"""
    it, sizes = _rlc_items(vw, n)
    base = n if at_n else 0
    always = 1 if n == 1 else 0  # a lone item takes a hashed coefficient only with `always`
    exp = rlc_expect(vw, it, n, sizes, base, always)
    both = vb.rlc(vw.key, it, n, sides=3, key_base=base, sizes=sizes, always=always)
    check_rlc(vw, both, exp, n, 3)
    one = vb.rlc(vw.key, it, n, sides=1, key_base=base, sizes=sizes, always=always)
    check_rlc(vw, one, exp, n, 1)
    assert one["sout"] is None
    two = vb.rlc(vw.key, it, n, sides=2, key_base=base, sizes=sizes, always=always, coef=one["coef"])
    check_rlc(vw, two, exp, n, 2)
    assert (two["coef"] == one["coef"]).all()  # read, not written
    if at_n:
        other = rlc_expect(vw, it, n, sizes, 0, always)
        hashed = [i for i in range(n) if exp[i][0] not in ((0, 0), (1, 0))]
        assert hashed and all(exp[i][0] != other[i][0] for i in hashed)


def test_rlc_singletons_always_and_null_offsets(vb, vw):
    n = 65
    it, sizes = _rlc_items(vw, n)
    # singleton groups keep (1, 0) and the point itself ...
    exp = rlc_expect(vw, it, n, sizes, 0, 0)
    single = [i for i, s in zip(range(n), [s for s in sizes for _ in range(s)]) if s == 1 and it.usable(i)]
    assert single and all(exp[i] == ((1, 0), vw.k[it.specs[i][0]]) for i in single)
    # ... unless `always`
    exp_a = rlc_expect(vw, it, n, sizes, 0, 1)
    assert all(exp_a[i][0] not in ((1, 0), (0, 0)) for i in single)
    check_rlc(vw, vb.rlc(vw.key, it, n, sizes=sizes, always=1), exp_a, n, 3)
    # grp_off null: (1, 0) for every usable item, unless `always`
    exp0 = rlc_expect(vw, it, n, None, 0, 0)
    assert all(e[0] in ((1, 0), (0, 0)) for e in exp0)
    check_rlc(vw, vb.rlc(vw.key, it, n, sizes=None), exp0, n, 3)
    check_rlc(vw, vb.rlc(vw.key, it, n, sizes=None, always=1), rlc_expect(vw, it, n, None, 0, 1), n, 3)


@pytest.mark.parametrize("kind", ["pk_st", "sig_st", "pk_inf", "sig_inf"])
def test_rlc_each_unusable_flag_alone(vb, vw, kind):
    """one flag on an otherwise good record: both outputs at infinity, coef (0, 0); with sig null (keys
    only) the signature's flags do not count"""
    specs = [(1, None), (2, kind), (3, None)]
    it = Items(vw, specs, 4)
    exp = rlc_expect(vw, it, 3, [3], 0, 0)
    assert exp[1] == ((0, 0), None)
    check_rlc(vw, vb.rlc(vw.key, it, 3, sizes=[3]), exp, 3, 3)
    expk = rlc_expect(vw, it, 3, [3], 0, 0, keys_only=True)
    assert (expk[1][1] is None) == (kind in PK_KINDS)
    check_rlc(vw, vb.rlc(vw.key, it, 3, sides=1, sizes=[3], keys_only=True), expk, 3, 1)


def test_rlc_guard_byte(vb, vw):
    it, sizes = _rlc_items(vw, 65)
    for sides in (1, 3):
        got = vb.rlc(vw.key, it, 65, sides=sides, sizes=sizes, guard=0)
        assert all(untouched(got[k]) for k in ("pout", "sout", "coef") if got[k] is not None)
    got = vb.rlc(vw.key, it, 65, sizes=sizes, guard=1)
    check_rlc(vw, got, rlc_expect(vw, it, 65, sizes, 0, 0), 65, 3)


def _went(vb, it, n, n_wide):
    """entry numbers (table e is key e's): none for every third item, for a rejected key and for a key without a table"""
    return [vb.NONE if (i % 3 == 1 or it.specs[i][1] in PK_KINDS or it.specs[i][0] >= n_wide) else it.specs[i][0]
            for i in range(n)]


def test_rlc_ladder_tables(vb, vw):
    """KeyWideRef: a mix of entries and KEY_WIDE_NONE; the elements are those of the narrow run, and
    wide_items / narrow_items are the exact counts of hashed-coefficient lanes with / without a table"""
    n, n_wide = 65, 12
    it, sizes = _rlc_items(vw, n)
    exp = rlc_expect(vw, it, n, sizes, 0, 0)
    went = _went(vb, it, n, n_wide)
    wide_pk = _u32(vw.pkw[:n_wide], 28)
    got = vb.rlc(vw.key, it, n, sides=1, sizes=sizes, went=went, wide_pk=wide_pk)
    check_rlc(vw, got, exp, n, 1)
    hashed = [i for i in range(n) if exp[i][0] not in ((0, 0), (1, 0))]
    ctr = dict(zip(CTR, (int(x) for x in got["ctr"])))
    wide = sum(went[i] != vb.NONE for i in hashed)
    assert 0 < wide < len(hashed)
    assert ctr == dict(hits=0, misses=0, size=0, wide_built=0, wide_chunks=0, narrow_chunks=0, wide_items=wide,
                       narrow_items=len(hashed) - wide)
    # sides 3 never goes through the tables
    got3 = vb.rlc(vw.key, it, n, sides=3, sizes=sizes, went=went, wide_pk=wide_pk)
    check_rlc(vw, got3, exp, n, 3)
    assert not got3["ctr"].any()


# ---- the chunk plans ----------------------------------------------------------------------------
PLAN_SIZES = [0, 1, 2, 15, 16, 17, 31, 32, 33, 100]


@pytest.mark.parametrize("cmax", [1, 2, 3, 16])
def test_plan(vb, cmax):
    rng = random.Random(700 + cmax)
    sizes = PLAN_SIZES + [rng.choice(PLAN_SIZES) for _ in range(60)]  # 70 groups: two blocks
    off = _offsets(sizes)
    ng, n = len(sizes), off[-1]
    bound = n // cmax + ng  # how the product sizes the launch
    cnt, coff, cfirst, ccount = (list(int(x) for x in a) for a in vb.plan(off, cmax, bound + 2))
    total = coff[ng]
    assert total == sum(cnt) <= bound
    assert coff[:ng] == [sum(cnt[:g]) for g in range(ng)]
    assert all(v == SENT32 for v in cfirst[total:] + ccount[total:])
    for g, s in enumerate(sizes):
        cs = [(cfirst[c], ccount[c] & 0x7FFFFFFF, ccount[c] >> 31) for c in range(coff[g], coff[g + 1])]
        assert len(cs) == -(-s // cmax)
        assert all(c[2] == (1 if s == 1 else 0) for c in cs)   # bit 31 exactly for groups of one item
        pos = off[g]
        for first, m, _ in cs:                                 # the chunks partition the items in order
            assert first == pos and 1 <= m <= cmax
            pos += m
        assert pos == off[g + 1]
        assert not cs or max(c[1] for c in cs) - min(c[1] for c in cs) <= 1
    assert (cnt, coff, cfirst[:total], ccount[:total]) == R.plan_chunks(off, cmax)


@pytest.mark.parametrize("ng", [1, 64, 65, 1023, 1024, 1025, 2049, 5000])
def test_plan_scan(vb, ng):
    rng = random.Random(800 + ng)
    cnt = [rng.choice([0, 1, 2, 7, 50]) for _ in range(ng)]
    cnt[0], cnt[-1] = 3, 5
    off = [int(x) for x in vb.scan(cnt)]
    assert off == _offsets(cnt)


# ---- k_rlc_msm ----------------------------------------------------------------------------------
def msm_expect(vw, it, sizes, cmax, sparse, always, key_base=0):
    """From the plan's restatement and the comments above k_rlc_msm / rlc_single: per item the (a, b)
    pair or sparse record it must hold (None: not written), and the scalar of pout / sout (None:
    infinity) -- the chunk's sum at its first item, infinity at the others"""
    _, coff, cfirst, ccount = R.plan_chunks(_offsets(sizes), cmax)
    n = _offsets(sizes)[-1]
    coef, coef4, scal = [None] * n, [None] * n, [None] * n
    for c in range(coff[-1]):
        first, m = cfirst[c], ccount[c] & 0x7FFFFFFF
        if ccount[c] >> 31 and not always:
            ok = it.usable(first)
            coef[first] = (1, 0) if ok else (0, 0)
            scal[first] = vw.k[it.specs[first][0]] if ok else None
            continue
        total = 0
        for i in range(first, first + m):
            k = vw.k[it.specs[i][0]]
            if sparse:
                coef4[i] = R.rlc_record(vw.key, key_base + i) if it.usable(i) else (0, 0, 0, 0)
                r = R.rlc_scalar(*R.sparse_ab(coef4[i])) if it.usable(i) else 0
            else:
                coef[i] = R.rlc_coeffs(vw.key, key_base + i) if it.usable(i) else (0, 0)
                r = R.rlc_scalar(*coef[i])
            total += r * k
        scal[first] = total % B.R or None
    return coef, coef4, scal


def check_msm(vw, got, exp, n, sides, written=True):
    coef, coef4, scal = exp
    if sides & 1:
        check_points(vw, 1, got["pout"], scal, n)
    else:
        assert untouched(got["pout"])
    if sides & 2:
        check_points(vw, 2, got["sout"], scal, n)
    else:
        assert untouched(got["sout"])
    for name, want, width in (("coef", coef, 2), ("coef4", coef4, 4)):
        for i in range(n):
            if want[i] is None or not sides & 1:
                assert untouched(got[name][i]), (name, i)
            else:
                assert tuple(int(x) for x in got[name][i]) == tuple(want[i]), (name, i)
        assert untouched(got[name][n:])


MSM_SIZES = [1, 2, 16, 17, 40, 1, 2]
MSM_BAD = {0: None, 5: "sig_st", 9: "pk_inf", 20: "sig_inf", 40: "pk_st", 76: "pk_st", 78: "sig_zero"}


def _msm_items(vw):
    n = sum(MSM_SIZES)
    specs = [((5 * i + 1) % len(vw.k), MSM_BAD.get(i)) for i in range(n)]
    return Items(vw, specs, n + 2), n


@pytest.mark.parametrize("cmax", [2, 16])
@pytest.mark.parametrize("variant", ["dense3", "dense12", "sparse3", "sparse1", "always3"])
def test_rlc_msm(vb, vw, variant, cmax):
    """pout[cfirst[c]] is the sum over the chunk's usable items and every other item of the chunk is
    infinity, likewise sout; coef / coef4 per item, zeros for unusable ones; groups of one keep r = 1
    ((1, 0), or (0, 0) when unusable) unless `always`; lanes at or beyond *total write nothing"""
    it, n = _msm_items(vw)
    sparse, always = int(variant.startswith("sparse")), int(variant == "always3")
    sides = 1 if variant in ("dense12", "sparse1") else 3
    exp = msm_expect(vw, it, MSM_SIZES, cmax, sparse, always)
    got = vb.rlc_msm(vw.key, it, MSM_SIZES, cmax, sides=sides, sparse=sparse, always=always)
    plan = R.plan_chunks(_offsets(MSM_SIZES), cmax)
    total = plan[1][-1]
    assert [list(int(x) for x in got[k])[:len(p)] for k, p in zip(("cnt", "coff", "cfirst", "ccount"), plan)] == list(plan)
    assert untouched(got["cfirst"][total:]) and untouched(got["ccount"][total:])
    assert total < n // cmax + len(MSM_SIZES)  # lanes beyond *total ran
    check_msm(vw, got, exp, n, sides)
    if variant == "dense12":  # the second pass reads the coef the first left: the same r_i on both sides
        two = vb.rlc_msm(vw.key, it, MSM_SIZES, cmax, sides=1, then2=1)
        check_msm(vw, two, exp, n, 3)
    singles = [i for i, s in zip(range(n), [s for s in MSM_SIZES for _ in range(s)]) if s == 1]
    if not sparse:
        for i in singles:
            want = ((1, 0) if it.usable(i) else (0, 0)) if not always else exp[0][i]
            assert exp[0][i] == want and (always == 0 or not it.usable(i) or want not in ((1, 0), (0, 0)))


def test_rlc_msm_guard_and_key_base(vb, vw):
    it, n = _msm_items(vw)
    got = vb.rlc_msm(vw.key, it, MSM_SIZES, 16, guard=0)
    assert all(untouched(got[k]) for k in ("pout", "sout", "coef", "coef4"))
    assert int(got["coff"][-1]) == R.plan_chunks(_offsets(MSM_SIZES), 16)[1][-1]  # the plan has no guard
    got = vb.rlc_msm(vw.key, it, MSM_SIZES, 16, guard=1, key_base=1000)
    exp = msm_expect(vw, it, MSM_SIZES, 16, 0, 0, key_base=1000)
    assert exp[0] != msm_expect(vw, it, MSM_SIZES, 16, 0, 0)[0]
    check_msm(vw, got, exp, n, 3)


POISON = [(pos, kind) for kind in ("pk_ph", "pk_zero", "sig_ph", "sig_zero") for pos in (0, 7, 15)]


@pytest.mark.parametrize("sparse", [0, 1])
def test_rlc_msm_poisoned_chunks(vb, vw, sparse):
    """One chunk of 16 shares one Montgomery inversion.  An unusable item at its first, a middle and
    its last position -- with the placeholder the decompression leaves, and with zero coordinates and
    the inf flag -- must not disturb the other 15 items' sum; a chunk of unusable items only gives
    infinity; a chunk holding one key twice adds it twice."""
    specs = []
    for c, (pos, kind) in enumerate(POISON):
        specs += [((3 * c + j) % len(vw.k), kind if j == pos else None) for j in range(16)]
    specs += [(j, ("pk_ph", "sig_ph", "pk_zero", "sig_zero")[j % 4]) for j in range(16)]   # all unusable
    specs += [(j if j != 9 else 4, None) for j in range(16)]                                  # key 4 twice
    sizes = [16] * (len(POISON) + 2)
    it = Items(vw, specs, len(specs) + 1)
    n = len(specs)
    exp = msm_expect(vw, it, sizes, 16, sparse, 0)
    assert exp[2][16 * len(POISON)] is None and sum(s is not None for s in exp[2]) == len(POISON) + 1
    got = vb.rlc_msm(vw.key, it, sizes, 16, sparse=sparse)
    check_msm(vw, got, exp, n, 3)


@pytest.mark.parametrize("cmax", [2, 16])
def test_rlc_msm_ladder_tables(vb, vw, cmax):
    """dense sides 1 with ladder tables: a chunk whose items all have entries goes through the tables, a
    chunk with one KEY_WIDE_NONE does not; the elements are identical either way; wide_chunks and
    narrow_chunks are exact"""
    sizes, n_wide = [16, 16, 1, 17, 2, 1], len(vw.k)  # table e is key e's
    n = sum(sizes)
    specs = [((7 * i + 2) % len(vw.k), {3: "sig_st", 20: "pk_st"}.get(i)) for i in range(n)]
    it = Items(vw, specs, n + 1)
    # item 3 is unusable by its signature: still an entry; item 20 is a rejected key: no entry; one more
    # item without an entry inside the group of 17; both groups of one have entries
    went = [it.specs[i][0] for i in range(n)]
    for i in (20, 33 + 12):
        went[i] = vb.NONE
    wide_pk = _u32(vw.pkw[:n_wide], 28)
    _, coff, cfirst, ccount = R.plan_chunks(_offsets(sizes), cmax)
    for always in (0, 1):
        # the chunks that reach a ladder (not the groups of one, unless `always`), with / without a full set of entries
        ladder = [c for c in range(coff[-1]) if always or not ccount[c] >> 31]
        full = [c for c in ladder if all(went[i] != vb.NONE for i in range(cfirst[c], cfirst[c] + (ccount[c] & 0x7FFFFFFF)))]
        assert 0 < len(full) < len(ladder)
        if cmax == 16:  # [0..15] wide, [16..31] narrow, [33..40] wide, [41..49] narrow, [50..51] wide; [32], [52] alone
            assert (len(full), len(ladder)) == (3 + 2 * always, 5 + 2 * always)
        exp = msm_expect(vw, it, sizes, cmax, 0, always)
        got = vb.rlc_msm(vw.key, it, sizes, cmax, sides=1, always=always, went=went, wide_pk=wide_pk)
        check_msm(vw, got, exp, n, 1)
        narrow = vb.rlc_msm(vw.key, it, sizes, cmax, sides=1, always=always)
        for i in range(n):
            assert decode(1, got["pout"][i]) == decode(1, narrow["pout"][i])
        ctr = dict(zip(CTR, (int(x) for x in got["ctr"])))
        want = dict(wide_chunks=len(full), narrow_chunks=len(ladder) - len(full), wide_items=0, narrow_items=0, hits=0,
                    misses=0, size=0, wide_built=0)
        assert ctr == want, always
    # sides 3 never goes through the tables (always == 1 here: every chunk reaches the ladder)
    got = vb.rlc_msm(vw.key, it, sizes, cmax, sides=3, always=1, went=went, wide_pk=wide_pk)
    assert not got["ctr"][3:5].any() and int(got["ctr"][5]) == coff[-1]
    check_msm(vw, got, msm_expect(vw, it, sizes, cmax, 0, 1), n, 3)


# ---- k_scatter ----------------------------------------------------------------------------------
SC_FLAGS = [(), ("pk_st",), ("sig_st",), ("pk_inf",), ("sig_inf",), ("msg_inf",), ("pk_st", "sig_st"), ("sig_st", "pk_inf"),
            ("pk_inf", "msg_inf")]
LISTED = "list"


def scatter_status(vb, flags, gv, gsize, n_agg, first, g):
    """An item's status, or LISTED -- the comments of layout.h (ScatterArgs, the group verdicts): decode
    statuses first (key, then signature), then infinity anywhere (verify_core), then the group's verdict;
    first-error mode leaves groups after the first failing one unresolved; a failing group of one item is
    that item's verdict unless aggregates are folded in; everything else is re-checked alone"""
    if "pk_st" in flags:
        return vb.ST_BAD_PUBKEY
    if "sig_st" in flags:
        return vb.ST_BAD_SIGNATURE
    if flags:
        return vb.ST_NOT_VERIFIED
    if gv == vb.GV_PASS:
        return vb.ST_OK
    failed = gv != vb.GV_PASS and gv < vb.GV_UNCHECKED
    if first is not None and (gv == vb.GV_UNCHECKED or (failed and g != first)):
        return vb.ST_UNCHECKED
    if not n_agg and gsize <= 1:
        return vb.ST_NOT_VERIFIED
    return LISTED


def agg_status(vb, ta, flags, gv):
    if ta != vb.ST_OK:
        return ta
    if "pk_st" in flags:
        return vb.ST_BAD_PUBKEY
    if flags:
        return vb.ST_NOT_VERIFIED
    return vb.ST_OK if gv == vb.GV_PASS else LISTED


def _hm_table(vw):
    """three MsgEntry: only h.inf is read; entry 2 is flagged infinite"""
    tab = _sent32(3, R.MSG_WORDS)
    for m in range(3):
        tab[m, :R.HM_WORDS] = _u32(hme(vw.sig[m], inf=m == 2))
    return tab


def _scatter_arrays(vb, vw, items, gver, grp_off, n_agg, aggs=()):
    n, ng = len(items), len(gver)
    pk, sig = _u32([vw.pkw[i % 8] for i in range(n)], 28), _u32([vw.sigw[i % 8] for i in range(n)], 52)
    for i, it in enumerate(items):
        f = it.get("flags", ())
        pk[i, 24] = int("pk_inf" in f)
        sig[i, 48] = int("sig_inf" in f)
    a = dict(item_grp=_u32([it["grp"] for it in items]),
             msg_idx=_u32([2 if "msg_inf" in it.get("flags", ()) else it["msg"] for it in items]),
             hm=_hm_table(vw), pk=pk, pk_st=_u8(int("pk_st" in it.get("flags", ())) for it in items), sig=sig,
             sig_st=_u8(2 * int("sig_st" in it.get("flags", ())) for it in items), gverdict=_u8(gver),
             grp_off=None if grp_off is None else _u32(grp_off), status=_sent8(n + 2), list=_sent32(n + n_agg + 2),
             count=np.zeros(1, dtype=np.uint32))
    if n_agg:
        apk, asig = _u32([vw.pkw[8 + v % 8] for v in range(n_agg)], 28), _u32([vw.sigw[8 + v % 8] for v in range(n_agg)], 52)
        for v, (ta, f) in enumerate(aggs):
            apk[v, 24] = int("pk_inf" in f)
            asig[v, 48] = int("sig_inf" in f)
        a.update(ta_status=_u8(ta for ta, _ in aggs), agg_pk=apk, agg_pk_st=_u8(int("pk_st" in f) for _, f in aggs),
                 agg_sig=asig, agg_status=_sent8(n_agg + 1))
    return a


def _scatter_case(vb, n, with_off, rot):
    """n items over groups of one and of several items whose verdicts walk through every kind, the items'
    flags through SC_FLAGS; -> (items, gver, grp_off or None, sizes)"""
    kinds = [vb.GV_PASS, 1, 0x7F, vb.GV_UNCHECKED, vb.GV_NOT_READY]
    items, gver, sizes = [], [], []
    if not with_off:  # every item its own group
        for i in range(n):
            items.append(dict(grp=i, msg=i % 2, flags=SC_FLAGS[(i + rot) % len(SC_FLAGS)]))
            gver.append(kinds[((i + rot) // len(SC_FLAGS)) % len(kinds)])
        return items, gver, None, [1] * n
    g = 0
    while len(items) < n:
        size = min(1 if g % 2 == 0 else len(SC_FLAGS), n - len(items))
        for j in range(size):
            flags = SC_FLAGS[(g // 2 // len(kinds) + rot) % len(SC_FLAGS)] if g % 2 == 0 else SC_FLAGS[j]
            items.append(dict(grp=g, msg=(g + j) % 2, flags=flags))
        gver.append(kinds[(g // 2 + rot) % len(kinds)])
        sizes.append(size)
        g += 1
    return items, gver, _offsets(sizes), sizes


AGG_CASES = [(0, ()), (2, ()), (3, ("pk_st",)), (5, ()), (0, ("pk_st",)), (0, ("pk_inf",)), (0, ("sig_inf",)),
             (0, ("pk_st", "pk_inf"))]


@pytest.mark.parametrize("n", [1, 64, 65, 200])
def test_scatter(vb, vw, n):
    seen = set()
    for rot, with_off, with_agg, first_mode in itertools.product(range(3 if n < 200 else 1), (True, False), (False, True),
                                                                 (None, "mid", "none")):
        items, gver, off, sizes = _scatter_case(vb, n, with_off, rot + (0 if n > 1 else 4 * with_agg))
        ng = len(gver)
        n_agg = ng if with_agg else 0
        aggs = [AGG_CASES[(v + rot) % len(AGG_CASES)] for v in range(n_agg)]
        failing = [g for g in range(ng) if gver[g] in (1, 0x7F)]
        # first_group: a failing group in the middle with an unflagged item (failing groups before, at and after it), or
        # 0xffffffff (no group's own check failed)
        clean = [g for g in failing if any(not it["flags"] for it in items if it["grp"] == g)] or failing
        first = None if first_mode is None else (clean[len(clean) // 2] if first_mode == "mid" and clean else 0xFFFFFFFF)
        a = _scatter_arrays(vb, vw, items, gver, off, n_agg, aggs)
        vb.scatter(a, n, ng, n_agg, first)
        want = [scatter_status(vb, it["flags"], gver[it["grp"]], sizes[it["grp"]], n_agg, first, it["grp"]) for it in items]
        wagg = [agg_status(vb, ta, f, gver[v]) for v, (ta, f) in enumerate(aggs)]
        listed = sorted([i for i, s in enumerate(want) if s == LISTED] + [n + v for v, s in enumerate(wagg) if s == LISTED])
        count = int(a["count"][0])
        got_list = [int(x) for x in a["list"][:count]]
        assert count == len(listed) and sorted(got_list) == listed and len(set(got_list)) == count
        assert untouched(a["list"][count:])
        for i, s in enumerate(want):
            assert int(a["status"][i]) == (SENT8 if s == LISTED else s), (i, items[i], gver[items[i]["grp"]])
        assert untouched(a["status"][n:])
        for v, s in enumerate(wagg):
            assert int(a["agg_status"][v]) == (SENT8 if s == LISTED else s), (v, aggs[v])
        if n_agg:
            assert untouched(a["agg_status"][n_agg:])
        # safety, apart from the table: ST_OK implies clear flags and a passing group; no item ends with
        # neither a status nor a place in the list
        for i, it in enumerate(items):
            st = int(a["status"][i])
            if st == vb.ST_OK:
                assert not it["flags"] and gver[it["grp"]] == vb.GV_PASS
            assert (st != SENT8) != (i in got_list)
            seen.add((it["flags"], gver[it["grp"]], sizes[it["grp"]] > 1, bool(n_agg),
                      None if first is None else (it["grp"] > first) - (it["grp"] < first)))
        for v, (ta, f) in enumerate(aggs):
            st = int(a["agg_status"][v])
            if st == vb.ST_OK:
                assert ta == vb.ST_OK and not f and gver[v] == vb.GV_PASS
            assert (st != SENT8) != (n + v in got_list)
    if n == 200:  # the enumeration is complete: every flag set x verdict x group kind x aggregates x relation
        kinds = [vb.GV_PASS, 1, 0x7F, vb.GV_UNCHECKED, vb.GV_NOT_READY]
        for flags, gv, many, agg in itertools.product(SC_FLAGS[:6], kinds, (False, True), (False, True)):
            rel = {s[4] for s in seen if s[:4] == (flags, gv, many, agg)}
            assert {None, -1, 1} <= rel, (flags, gv, many, agg, rel)
        assert any(s[4] == 0 and s[1] in (1, 0x7F) and not s[0] for s in seen)


# ---- the verdict kernels (vgroup.hip) -----------------------------------------------------------
def _batch_verdict(vb, gst, bver, fb, guard=None, first=None, g0=0):
    ng = len(gst)
    gver, lst, count = _sent8(ng + 2), _sent32(ng + 2), np.zeros(1, dtype=np.uint32)
    fa = None if first is None else _u32([first])
    gs, bv = _u8(gst), _u8(bver)
    _ok(vb.pair.db_batch_verdict(ng, _ptr(gs), _ptr(bv), len(bver), fb, _ptr(gver), ng + 2, _ptr(lst), ng + 2,
                                 _ptr(count), -1 if guard is None else guard, _ptr(fa), g0), "db_batch_verdict")
    return gver, lst, int(count[0]), None if fa is None else int(fa[0])


def batch_verdict_expect(vb, gst, bver, fb, first, g0):
    """layout.h: not READY -> GV_NOT_READY; READY in a passing batch -> GV_PASS; else the group joins
    the list -- in first-error mode only the groups of the failing batch with the smallest key g0 +
    (first group of the batch), the other failing batches' groups get GV_UNCHECKED"""
    ng = len(gst)
    keyof = [g0 + (g // fb) * fb for g in range(ng)]
    failing = [keyof[g] for g in range(ng) if gst[g] == vb.G_READY and bver[g // fb]]
    f = None if first is None else min([first] + failing)
    gver, lst = [], []
    for g in range(ng):
        if gst[g] != vb.G_READY:
            gver.append(vb.GV_NOT_READY)
        elif not bver[g // fb]:
            gver.append(vb.GV_PASS)
        elif f is not None and keyof[g] != f:
            gver.append(vb.GV_UNCHECKED)
        else:
            gver.append(SENT8)
            lst.append(g)
    return gver, lst, f


@pytest.mark.parametrize("fb", [1, 4, 64])
@pytest.mark.parametrize("ng", [1, 63, 64, 65, 130])
def test_batch_verdict(vb, ng, fb):
    rng = random.Random(900 + 7 * ng + fb)
    nb = -(-ng // fb)
    states = [vb.G_READY, vb.G_READY, vb.G_FALLBACK, vb.G_READY, vb.G_EMPTY]
    for trial in range(3):
        gst = [states[(g + trial) % 5] if rng.random() < 0.8 else vb.G_READY for g in range(ng)]
        bver = [0] * nb
        bad = sorted(rng.sample(range(nb), min(nb, 3)))  # up to three failing batches (the last one ragged at times)
        for k, bi in enumerate(bad):
            bver[bi] = (1, 0x7F, 3)[k]
        if trial == 2:
            bver[-1] = 1
        if len(bad) >= 2 and trial == 1:  # the failing batch with the smallest key holds no READY group: not the first
            for g in range(bad[0] * fb, min(ng, bad[0] * fb + fb)):
                gst[g] = vb.G_FALLBACK
        for first, g0 in ((None, 0), (0xFFFFFFFF, 0), (0xFFFFFFFF, 192), (5, 64)):
            gver, lst, count, f = _batch_verdict(vb, gst, bver, fb, first=first, g0=g0)
            wv, wl, wf = batch_verdict_expect(vb, gst, bver, fb, first, g0)
            assert list(gver[:ng]) == wv and untouched(gver[ng:]), (trial, first, g0)
            assert count == len(wl) and sorted(int(x) for x in lst[:count]) == wl and untouched(lst[count:])
            assert f == wf
            if first == 5:  # an earlier chunk holds the first failing batch: nothing of this one is listed
                assert count == 0 and f == 5
            if first == 0xFFFFFFFF and len({g0 + (g // fb) * fb for g in wl}) and wl:
                assert len({g // fb for g in wl}) == 1 and f == g0 + (wl[0] // fb) * fb
    gver, lst, count, f = _batch_verdict(vb, gst, bver, fb, guard=0, first=0xFFFFFFFF)
    assert untouched(gver) and untouched(lst) and count == 0 and f == 0xFFFFFFFF
    gver, lst, count, f = _batch_verdict(vb, gst, bver, fb, guard=1)
    assert list(gver[:ng]) == batch_verdict_expect(vb, gst, bver, fb, None, 0)[0]


@pytest.mark.parametrize("ng", [1, 63, 64, 65, 130])
def test_slot_verdict(vb, ng):
    """sfail[0] set: no verdict is written and sfail[1] is raised; clear: GV_NOT_READY / GV_PASS, and
    sfail[1] raised exactly when a group is not READY"""
    for pattern in ("ready", "last", "first", "mixed"):
        gst = [vb.G_READY] * ng
        if pattern == "last":
            gst[-1] = vb.G_EMPTY
        elif pattern == "first":
            gst[0] = vb.G_FALLBACK
        elif pattern == "mixed":
            gst = [(vb.G_READY, vb.G_FALLBACK, vb.G_READY, vb.G_EMPTY)[g % 4] for g in range(ng)]
        for fail in (0, 1, 3):
            sfail, gver, gs = _u8([fail, 0]), _sent8(ng + 2), _u8(gst)
            _ok(vb.pair.db_slot_verdict(ng, _ptr(gs), _ptr(sfail), _ptr(gver), ng + 2), "db_slot_verdict")
            assert int(sfail[0]) == fail
            if fail:
                assert untouched(gver) and int(sfail[1]) == 1
            else:
                assert list(gver[:ng]) == [vb.GV_PASS if s == vb.G_READY else vb.GV_NOT_READY for s in gst]
                assert untouched(gver[ng:])
                assert int(sfail[1]) == int(any(s != vb.G_READY for s in gst)), pattern


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_first_group_and_first_item(vb, n):
    rng = random.Random(950 + n)
    gv_kinds = [vb.GV_PASS, vb.GV_UNCHECKED, vb.GV_NOT_READY]
    st_kinds = [vb.ST_OK, vb.ST_UNCHECKED]
    for hit in (None, 0, n // 2, n - 1):
        for fn, quiet, loud, name in ((vb.pair.db_first_group, gv_kinds, [1, 3, 0x7F], "db_first_group"),
                                      (vb.pair.db_first_item, st_kinds, [vb.ST_BAD_PUBKEY, vb.ST_BAD_SIGNATURE,
                                                                         vb.ST_NOT_VERIFIED], "db_first_item")):
            b = [rng.choice(quiet) for _ in range(n)]
            if hit is not None:
                b[hit] = rng.choice(loud)
                for j in range(hit + 1, n, 3):
                    b[j] = rng.choice(loud)
            for start in (0xFFFFFFFF, 0 if hit is None else hit + 1, 40):
                first, bb = _u32([start]), _u8(b)
                _ok(fn(_ptr(bb), n, _ptr(first)), name)
                assert int(first[0]) == min([start] + ([hit] if hit is not None else [])), (name, hit, start)


# ---- FastAggregateVerify ------------------------------------------------------------------------
SEG_SIZES = [0, 1, 2, 17, 0, 2, 2, 2, 1]  # ..., then [P, -P], [P, P], [infinity, P], [infinity]


def _seg_points(vw):
    """per entry (scalar of G1 or None for infinity, status byte); the segments' sums and ORs"""
    ks = [vw.k[i] for i in range(20)]
    ent = [(ks[i], 0) for i in range(20)]               # segments of 1, 2, 17
    ent[5] = (ks[5], 4)                                 # a bad flag inside the segment of 17
    ent[9] = (ks[9], 1)
    ent += [(ks[3], 0), (B.R - ks[3], 0)]               # P, -P
    ent += [(ks[4], 2), (ks[4], 0)]                     # P, P
    ent += [(None, 1), (ks[6], 2)]                      # infinity (flagged bad), P
    ent += [(None, 0)]
    off = _offsets(SEG_SIZES)
    assert off[-1] == len(ent)
    sums = [sum(e[0] for e in ent[off[s]:off[s + 1]] if e[0] is not None) % B.R or None for s in range(len(SEG_SIZES))]
    ors = [int(np.bitwise_or.reduce([e[1] for e in ent[off[s]:off[s + 1]]] or [0])) for s in range(len(SEG_SIZES))]
    return ent, off, sums, ors


@pytest.mark.parametrize("affine", [1, 0])
def test_seg_sum(vb, vw, affine):
    ent, off, sums, ors = _seg_points(vw)
    assert sums[5] is None and sums[0] is None and ors[3] == 5 and ors[7] == 3
    rng = random.Random(970)
    if affine:
        pts = _u32([g1a(None if k is None else vw.f1.mul(k)) for k, _ in ent], 28)
    else:
        pts = _u32([R.jac_entry(1, None if k is None else vw.f1.mul(k), rng.randrange(1, P)) for k, _ in ent], 36)
    n_seg = len(SEG_SIZES)
    out, st_out, st_in, offs = _sent32(n_seg + 1, 36), _sent8(n_seg + 1), _u8(s for _, s in ent), _u32(off)
    _ok(vb.lib.db_vb_seg_sum(affine, _ptr(pts), _ptr(st_in), len(ent), _ptr(offs), n_seg, _ptr(out),
                             _ptr(st_out), n_seg + 1), "db_vb_seg_sum")
    check_points(vw, 1, out, sums, n_seg)
    assert list(st_out[:n_seg]) == ors and untouched(st_out[n_seg:])


def test_va_point(vb, vw):
    """an empty group (0xffffffff) and a sum at infinity give the infinite entry; any other the affine point"""
    rng = random.Random(971)
    ks = [vw.k[0], None, vw.k[1], vw.k[2]]
    sums = _u32([R.jac_entry(1, None if k is None else vw.f1.mul(k), rng.randrange(1, P)) for k in ks], 36)
    sog = [0, 0xFFFFFFFF, 1, 3, 2, 0xFFFFFFFF, 0] * 10  # 70 groups: two blocks
    out, sg = _sent32(len(sog) + 1, 28), _u32(sog)
    _ok(vb.lib.db_vb_va_point(_ptr(sums), len(ks), _ptr(sg), len(sog), _ptr(out), len(sog) + 1), "db_vb_va_point")
    for g, s in enumerate(sog):
        k = None if s == 0xFFFFFFFF else ks[s]
        w = [int(v) for v in out[g]]
        assert w[24:] == [int(k is None), 0, 0, 0]
        x, y = R.from_words(w[:12]), R.from_words(w[12:24])
        assert x < 2 * P and y < 2 * P
        assert (R.unmont(x), R.unmont(y)) == ((0, 0) if k is None else vw.f1.mul(k)), g
    assert untouched(out[len(sog):])


def test_va_status(vb, vw):
    """herumi's order: the signature's decoding, the key's, then an empty group or an identity signature
    never verify, then the pairing verdict"""
    cases = list(itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (B.ST_OK, B.ST_NOT_VERIFIED, 1))) * 2  # two blocks
    sig = _u32([hme(vw.sig[g % 8], inf=bool(c[3])) for g, c in enumerate(cases)], 52)
    sog = [0xFFFFFFFF if c[2] else c[1] for c in cases]  # sum 1 is a bad key
    status = _sent8(len(cases) + 1)
    sst, kb, sg, pv = _u8(2 * c[0] for c in cases), _u8([0, 1]), _u32(sog), _u8(c[4] for c in cases)
    _ok(vb.lib.db_vb_va_status(_ptr(sig), _ptr(sst), _ptr(kb), 2, _ptr(sg),
                               _ptr(pv), len(cases), _ptr(status), len(cases) + 1), "db_vb_va_status")
    assert len(cases) > 64
    for g, (sst, kbad, empty, inf, pv) in enumerate(cases):
        if sst:
            want = vb.ST_BAD_SIGNATURE
        elif kbad and not empty:
            want = vb.ST_BAD_PUBKEY
        elif empty or inf:
            want = vb.ST_NOT_VERIFIED
        else:
            want = vb.ST_OK if pv == vb.ST_OK else vb.ST_NOT_VERIFIED
        assert int(status[g]) == want, cases[g]
        if int(status[g]) == vb.ST_OK:
            assert cases[g] == (0, 0, 0, 0, B.ST_OK)
    assert untouched(status[len(cases):])


def _check_column(col, Q):
    """a column [N_LINES, 72] is the chain of Q evaluated at -g1; every stored word below 2p"""
    chain = R.miller_chain(Q)
    for j, row in enumerate(col):
        l, raw = R.line_of_words([int(v) for v in row])
        assert max(raw) < 2 * P
        assert R.line_matches(l, chain[j], R.G1_NEG), ("line", j)


def test_sig_lines(vb, vw):
    n, stride = 3, 5
    lines, sig = _sent32(R.N_LINES, stride, R.LINE_WORDS), _u32(vw.sigw[:n], 52)
    _ok(vb.lib.db_vb_sig_lines(_ptr(sig), n, _ptr(lines), R.N_LINES * stride, stride), "db_vb_sig_lines")
    for i in range(n):
        _check_column(lines[:, i], vw.sig[i])
    assert untouched(lines[:, n:])


def test_fb_lines(vb, vw):
    """slot u = list position - base: base > 0, cap smaller than the remaining entries, *count below base
    + cap, entries on both sides of n_items (the folded aggregates' signatures)"""
    n_items, n_agg = 4, 3
    sig, agg = _u32(vw.sigw[:n_items], 52), _u32(vw.sigw[10:10 + n_agg], 52)
    lst = [3, 4, 0, 6, 5, 1, 2, SENT32]
    la = _u32(lst)
    where = lambda e: vw.sig[e] if e < n_items else vw.sig[10 + e - n_items]  # noqa: E731
    for base, cap, count in ((2, 3, 7), (5, 4, 7), (0, 2, 1)):
        lines = _sent32(R.N_LINES, cap, R.LINE_WORDS)
        _ok(vb.lib.db_vb_fb_lines(_ptr(la), len(lst), count, base, cap, _ptr(sig), n_items, _ptr(agg), n_agg,
                                  _ptr(lines)), "db_vb_fb_lines")
        for u in range(cap):
            if base + u < count:
                _check_column(lines[:, u], where(lst[base + u]))
            else:
                assert untouched(lines[:, u]), (base, u)
