"""The Miller-loop kernels (pipeline.hip) and the group stage (vgroup.hip) on the GPU against the
oracle.

Through the C ABI these kernels only ever give OK / NOT_VERIFIED bytes, at the shapes whole calls
happen to produce.  Here the test-only pair harness (tests/native/devblocks_pair.hip and
devblocks_vgroup.hip, a library of its own, compiling the product's pipeline.hip and vgroup.hip
themselves) runs one launcher per call on explicit raw words and copies every output array back in
full, pre-filled with a sentinel -- so the entries a kernel must not write are compared too.  The
oracle (oracle/bls12381.py) and Python integers are the only reference (tests/blocks_ref.py:
miller_chain, line_matches, miller_from_lines, pairing3; checked on the CPU by
tests/test_blocks_ref.py); the host harness is never the reference.

How values are compared: a line through line_matches (scaling-free); a stored Miller value computed
from lines that lie in memory exactly against the Python schedule over those same lines, which the
test has matched against the oracle; a value whose lines never leave the kernel (k_lml), and one
route per (P, Q), after the Python exponentiation; every stored word below 2p.

Which shape reaches which branch:
  k_lines_msg    n = 1 / 64 / 65: a partly filled wave, a full one, a second block of one lane; the
                 entry past n and -- with the guard byte 0 -- the whole table keep the sentinel.
  k_slines       65 units: an infinite point in the first, a middle and the last lane of wave 0 and
                 in the only lane of wave 1 (bad = 1, column untouched, neighbours right); Z = 1,
                 random Z, upper representatives, Z = p; stride > n (the gap keeps the sentinel);
                 list mode with *count below and above n.
  k_lines_at_p,  n = 1 / 64 / 65 on the same inputs: groups sharing a message and distinct ones, a
  k_mml_eval     nonzero pk_st in the first, a middle and the last group (the unit line, exactly),
                 a null pk_st.
  k_pair3        n = 1 / 21 / 22 / 43 (21 groups per wave: a full wave, one unit next to 20 shadow
                 groups, two waves and a unit), the cases rotated through every unit.
    ML           pk_st -> one; f_bad for pk_st, P.inf, hm.inf alone; f_out_stride 2 / f_out_off 1.
    MLS          the lines of k_slines at a stride above n.
    MML          f_range = MML_PAIRS and 1, f_n = 1 / 4 / 5 / 7 / 85: the select `k < cnt` of the
                 tail unit, pairs that are not READY first / middle / last; both line producers.
    PROD         f_range = 1 / 3 / PROD_FAN with f_n no multiple: `j >= cnt` of the tail unit.
    FIN, pair6   one route with sig_lines, three without (k_pair3<FIN>, k_pair6_fin<3>, <10>) on
                 the same stored values: a valid batch, one wrong member, pk_st, a short tail unit.
    FULL         direct and list mode (base > 0, *count below base / between / above), entries
                 >= n_items through the agg arrays, the precedence of the statuses, a valid and an
                 invalid signature in neighbouring units.
    guard        byte 0: no output of any mode changes.
  k_lml          side 0: n = 1 / 2 / 5, Z = 1 and random, f_stride / f_off, S infinite; side 1: units
                 sharing a message, bad for pk_st, P.inf, hm.inf alone; the guard byte.  The entry
                 point exposes the three stored roles (lanes with j == 0), which are compared.
  k_group_prep*  groups of 1 / 2 / 5 items with and without grp_off, g0 > 0; ng = 1 / 63 / 64 / 65
                 with fe_batch 0 / 4 / 64 for the butterfly (the last batch and wave partly
                 filled); every case of group_scan's rules (see _group_cases).
  k_batch_sum    k = 1 and MML_PAIRS with ng no multiple of k, one and two blocks.
"""
import ctypes
import random

import numpy as np
import pytest

import blocks_ref as R
from oracle import bls12381 as B

pytestmark = pytest.mark.gpu

P = B.P
SENT32, SENT8 = 0xC3A5C3A5, 0xEE  # a sentinel "value" is above 2p, a sentinel byte is no status
FULL, ML, FIN, PROD, MML, MLS = range(6)  # pipeline.hip's P3_* modes, in its enum's order
ST_OK, ST_BAD_PUBKEY, ST_BAD_SIGNATURE, ST_NOT_VERIFIED = B.ST_OK, B.ST_BAD_PUBKEY, B.ST_BAD_SIGNATURE, B.ST_NOT_VERIFIED
UNIT_LINE = R.words(R.RM) + [0] * 60  # (R, 0, 0): the Montgomery one, then zeros
W3 = ["n", "stride", "base", "n_items", "f_range", "f_n", "f_out_stride", "f_out_off", "count", "guard", "n_ent",
      "n_msgs", "n_agg", "list_len", "n_lines", "f_in_len", "f_out_len"]
A3 = ["pk", "pk_st", "sig_st", "sig_inf", "msg_idx", "hm", "sig_lines", "list", "agg_pk", "agg_msg", "f_in", "status",
      "agg_status", "f_out", "f_bad"]
WG = ["g0", "ng", "n_groups", "n_items", "n_msgs", "fe_batch", "keys_only", "skip_hm", "guard"]
AG = ["grp_off", "msg_idx", "hm", "pk", "pk_st", "sig", "sig_st", "pr", "sr", "agg_pk", "agg_pk_st", "agg_sig", "agg_st",
      "agg_pr", "agg_sr", "gP", "gmsg", "gst", "glines", "gS", "bS"]


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


def _g(guard):
    return -1 if guard is None else int(guard)


class Pair:
    def __init__(self, lib):
        self.lib = lib
        c = (ctypes.c_uint32 * 11)()
        lib.db_pair_consts(c)
        (self.n_lines, self.per_wave, self.mml_pairs, self.prod_fan, self.fe_batch, msg, line, fp4, g2j, g1a, hm) = list(c)
        # the raw-word formats of this file and blocks_ref are the library's
        assert self.n_lines == R.N_LINES and (msg, line, 3 * fp4, hm) == (4 * R.MSG_WORDS, 4 * R.LINE_WORDS, 4 * R.F12_WORDS, 4 * R.HM_WORDS)
        assert (g2j, g1a) == (4 * 72, 4 * 28)
        assert lib.db_pair3_words() == len(W3) and lib.db_pair3_ptrs() == len(A3)
        assert lib.db_group_words() == len(WG) and lib.db_group_ptrs() == len(AG)
        st = (ctypes.c_uint32 * 3)()
        lib.db_group_states(st)
        self.G_READY, self.G_FALLBACK, self.G_EMPTY = list(st)
        lib.db_lines_msg.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int]
        for f in (lib.db_lines_at_p, lib.db_mml_eval):
            f.argtypes = [ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 5
        lib.db_pair3.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        lib.db_group_prep.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        lib.db_pair6_fin.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
                                     ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        lib.db_lml.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 6 + \
            [ctypes.c_uint32] * 3 + [ctypes.c_void_p, ctypes.c_int]
        lib.db_slines.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                  ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                  ctypes.c_int]
        lib.db_batch_sum.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]

    def lines_msg(self, tab, n, guard=None, rc=0):
        got = self.lib.db_lines_msg(n, len(tab), _ptr(tab), _g(guard))
        if rc:
            assert got == rc
        else:
            _ok(got, "db_lines_msg")

    def eval_lines(self, at_p, pk, pk_st, msg_idx, tab):
        """-> ev [N_LINES, n, 72]"""
        n = len(pk)
        ev = _sent32(self.n_lines, n, R.LINE_WORDS)
        f = self.lib.db_lines_at_p if at_p else self.lib.db_mml_eval
        _ok(f(n, len(tab), _ptr(pk), _ptr(pk_st), _ptr(msg_idx), _ptr(tab), _ptr(ev)), "db_lines_at_p" if at_p else "db_mml_eval")
        return ev

    def slines(self, n, pts, stride, rows=None, list_=None, count=0, bad=True, guard=None):
        """-> (lines [N_LINES, stride, 72] -- unit u's line j at [j, u] --, bad [n] or None)"""
        lines = _sent32(rows or self.n_lines, stride, R.LINE_WORDS)
        b = _sent8(n) if bad else None
        _ok(self.lib.db_slines(n, len(pts), _ptr(pts), _ptr(list_), 0 if list_ is None else len(list_), count, _ptr(lines),
                               lines.shape[0] * stride, stride, _ptr(b), _g(guard)), "db_slines")
        return lines, b

    def pair3(self, mode, rc=0, **kw):
        """words and arrays by name (W3, A3); lengths are taken from the arrays"""
        a = {k: kw.pop(k, None) for k in A3}
        w = {k: 0 for k in W3}
        w["guard"] = 2
        ent = [a[k] for k in ("pk", "pk_st", "sig_st", "sig_inf", "msg_idx", "status", "f_bad") if a[k] is not None]
        w["n_ent"] = kw.pop("n_ent", len(ent[0]) if ent else 0)
        assert all(len(x) == w["n_ent"] for x in ent)
        for k, src in (("n_msgs", "hm"), ("n_agg", "agg_pk"), ("list_len", "list"), ("f_in_len", "f_in"), ("f_out_len", "f_out")):
            w[k] = 0 if a[src] is None else len(a[src])
        if a["agg_status"] is not None:
            w["n_agg"] = len(a["agg_status"])
        if a["sig_lines"] is not None:
            w["n_lines"] = a["sig_lines"].shape[0] * a["sig_lines"].shape[1]
        guard = kw.pop("guard", None)
        w["guard"] = 2 if guard is None else guard
        for k, v in kw.items():
            assert k in w, k
            w[k] = v
        wa = _u32([w[k] for k in W3])
        pa = (ctypes.c_void_p * len(A3))(*[_ptr(a[k]) for k in A3])
        got = self.lib.db_pair3(mode, _ptr(wa), pa)
        if rc:
            assert got == rc, (got, rc)
        else:
            _ok(got, f"db_pair3({mode})")

    def pair6_fin(self, per_wave, n, f_range, f_n, f_in, pk_st=None, guard=None):
        status = _sent8(n)
        _ok(self.lib.db_pair6_fin(per_wave, n, f_range, f_n, _g(guard), _ptr(f_in), len(f_in), _ptr(pk_st), _ptr(status)),
            f"db_pair6_fin({per_wave})")
        return status

    def lml(self, side, n, f_out_len, f_stride=0, f_off=0, pts=None, pk=None, pk_st=None, msg_idx=None, tab=None, bad=True,
            guard=None):
        f_out = _sent32(f_out_len, R.F12_WORDS)
        b = _sent8(n) if bad else None
        _ok(self.lib.db_lml(side, n, 0 if tab is None else len(tab), _ptr(pts), _ptr(pk), _ptr(pk_st), _ptr(msg_idx), _ptr(tab),
                            _ptr(f_out), f_out_len, f_stride, f_off, _ptr(b), _g(guard)), f"db_lml({side})")
        return f_out, b

    def group_prep(self, kind, arrays, g0, ng, fe_batch=0, keys_only=0, skip_hm=0, guard=None, rc=0):
        """arrays by name (AG); the lengths are taken from them"""
        a = {k: arrays.get(k) for k in AG}
        w = dict(g0=g0, ng=ng, n_groups=len(a["gmsg"]), n_items=len(a["pk"]), n_msgs=len(a["hm"]), fe_batch=fe_batch,
                 keys_only=keys_only, skip_hm=skip_hm, guard=2 if guard is None else guard)
        wa = _u32([w[k] for k in WG])
        pa = (ctypes.c_void_p * len(AG))(*[_ptr(a[k]) for k in AG])
        got = self.lib.db_group_prep(kind, _ptr(wa), pa)
        if rc:
            assert got == rc, (got, rc)
        else:
            _ok(got, f"db_group_prep({kind})")

    def batch_sum(self, gS, k, guard=None):
        ng = len(gS)
        bS = _sent32((ng + k - 1) // k, 72)
        _ok(self.lib.db_batch_sum(ng, k, _ptr(gS), _ptr(bS), _g(guard)), "db_batch_sum")
        return bS


@pytest.fixture(scope="module")
def pp():
    """The pair harness, loaded only if it was built from this tree (its embedded id); otherwise
    built now, and a failure of that fails the tests."""
    from gpu_helpers import harness
    return Pair(harness.load_devblocks("pair"))


# ---- records ------------------------------------------------------------------------------------
def g1a(pt, upper=False, inf=False):
    """G1AEntry of a finite point; inf: the flag set on the otherwise unchanged record"""
    w = R.affine_entry(1, pt, upper)
    w[24] = 1 if (inf or pt is None) else 0
    return w


def hme(pt, upper=False, inf=False):
    w = R.affine_entry(2, pt, upper)
    w[48] = 1 if (inf or pt is None) else 0
    return w


def below_2p(words):
    w = np.asarray(words).reshape(-1, 12)
    return all(R.from_words(row) < 2 * P for row in w)


def untouched(a):
    return bool((np.asarray(a) == (SENT8 if np.asarray(a).dtype == np.uint8 else SENT32)).all())


def parse_lines(col):
    """a column [N_LINES, 72] -> the lines as field elements; every stored word below 2p"""
    out = []
    for row in col:
        l, raw = R.line_of_words([int(v) for v in row])
        assert max(raw) < 2 * P
        out.append(l)
    return out


def f12(words):
    v, raw = R.f12_of_words([int(x) for x in words])
    assert max(raw) < 2 * P, "a stored word is not below 2p"
    return v


def p12_prod(vals):
    f = B.P12_ONE
    for v in vals:
        f = B._p12_mul(f, v)
    return f


class World:
    """Six keys (sk g1: g1 itself, (r - 1) g1, four random), six hashed messages (random multiples of
    G2_GEN; hashing is tested elsewhere) and the signatures sk H, from seeded random numbers; the
    message table of seven entries -- H_1 and H_4 in the upper representative, entry 6 = H_0 with its
    infinity flag set -- whose lines k_lines_msg computed and the fixture matched against the oracle."""

    def __init__(self, pp):
        rng = random.Random(20261020)
        self.rng = rng
        self.sk = [1, B.R - 1] + [rng.randrange(2, B.R - 1) for _ in range(4)]
        self.P = [B.g1_mul(B.G1_GEN, s) for s in self.sk]
        self.H = [B.g2_mul(B.G2_GEN, rng.randrange(1, B.R)) for _ in range(6)]
        self.H.append(self.H[0])
        self._sig = {}
        tab = _sent32(7, R.MSG_WORDS)
        for m, h in enumerate(self.H):
            tab[m, :R.HM_WORDS] = _u32(hme(h, upper=m in (1, 4), inf=m == 6))
        self.tab0 = tab.copy()  # before the lines
        pp.lines_msg(tab, 7)
        self.tab = tab
        self.tlines = [self.msg_lines(tab, m) for m in range(7)]
        for m in range(6):  # entry 6 is flagged infinite: its lines are never used for a verdict
            check_chain(self.tlines[m], self.H[m])

    def sig(self, i, m):
        if (i, m) not in self._sig:
            self._sig[(i, m)] = B.g2_mul(self.H[m], self.sk[i])
        return self._sig[(i, m)]

    @staticmethod
    def msg_lines(tab, m):
        return parse_lines(tab[m, R.HM_WORDS:].reshape(R.N_LINES, R.LINE_WORDS))

    _ml = {}

    def ml_value(self, i, m):
        """the Python schedule over the table's stored lines of message m, evaluated at P_i"""
        if (i, m) not in self._ml:
            self._ml[(i, m)] = R.miller_from_lines([R.eval_line(l, self.P[i]) for l in self.tlines[m]])
        return self._ml[(i, m)]


def check_chain(lines, Q, at=None):
    chain = R.miller_chain(Q)
    for j, (l, s) in enumerate(zip(lines, chain)):
        assert R.line_matches(l, s, at), ("line", j)


@pytest.fixture(scope="module")
def world(pp):
    return World(pp)


_SL = {}


def sig_columns(pp, pts):
    """The lines at -g1 of the points (k_slines, Z = 1), one launch for the module's distinct points,
    each column matched against the oracle once: -> [(column [N_LINES, 72], lines, Python MLS value)]"""
    todo = [s for s in dict.fromkeys(pts) if s not in _SL]
    if todo:
        lines, bad = pp.slines(len(todo), _u32([R.jac_entry(2, s) for s in todo], 72), len(todo))
        assert not bad.any()
        for u, s in enumerate(todo):
            col = lines[:, u].copy()
            parsed = parse_lines(col)
            check_chain(parsed, s, R.G1_NEG)
            _SL[s] = (col, parsed, R.miller_from_lines(parsed))
    return [_SL[s] for s in pts]


def sig_lines_of(cols, stride=None):
    """sig_lines [N_LINES, stride, 72] with unit u's column at u, the gap the sentinel"""
    out = _sent32(R.N_LINES, stride or len(cols), R.LINE_WORDS)
    for u, c in enumerate(cols):
        out[:, u] = c[0]
    return out


SHAPES3 = [1, 21, 22, 43]


# ---- the line producers -------------------------------------------------------------------------
def test_harness_refuses_indices_outside_its_buffers(pp, world):
    """every entry point checks what the kernel would follow before it launches (DB_E_ARG = -1)"""
    w = world
    tab = w.tab.copy()
    pp.lines_msg(tab, 8, rc=-1)
    pk, mi = _u32([g1a(w.P[0])], 28), _u32([7])
    ev, f1, f2 = _sent32(68, 72), _sent32(1, 144), _sent32(2, 144)
    assert pp.lib.db_mml_eval(1, 7, _ptr(pk), None, _ptr(mi), _ptr(tab), _ptr(ev)) == -1
    assert pp.lib.db_lml(1, 1, 7, None, _ptr(pk), None, _ptr(mi), _ptr(tab), _ptr(f1), 1, 0, 0, None, -1) == -1
    two = _sent32(2, 72)
    assert pp.lib.db_lml(0, 2, 0, _ptr(two), None, None, None, None, _ptr(f2), 2, 2, 0, None, -1) == -1
    one = _u32([R.f12_words(B.P12_ONE)] * 4, 144)
    pp.pair3(PROD, rc=-1, n=2, f_range=2, f_n=4, f_in=one, f_out=_sent32(2, 144), f_out_off=1)
    pp.pair3(PROD, rc=-1, n=2, f_range=2, f_n=5, f_in=one, f_out=_sent32(2, 144))
    pp.pair3(ML, rc=-1, n=1, pk=pk, msg_idx=mi, hm=tab, f_out=_sent32(1, 144))
    pp.pair3(MML, rc=-1, n=2, f_range=4, f_n=4, sig_lines=_sent32(68, 4, 72), f_out=_sent32(2, 144))
    pp.pair3(MLS, rc=-1, n=3, stride=2, sig_lines=_sent32(68, 2, 72), f_out=_sent32(3, 144))
    pp.pair3(FULL, rc=-1, n=1, n_items=1, list=_u32([1]), count=1, pk=pk, msg_idx=_u32([0]), hm=tab,
             sig_lines=_sent32(68, 1, 72), status=_sent8(1))
    pts, lst, lines = _u32([R.jac_entry(2, w.H[0])], 72), _u32([1]), _sent32(136, 72)
    assert pp.lib.db_slines(1, 1, _ptr(pts), _ptr(lst), 1, 1, _ptr(lines), 68, 1, None, -1) == -1
    assert pp.lib.db_slines(2, 1, _ptr(pts), None, 0, 0, _ptr(lines), 136, 2, None, -1) == -1
    assert pp.lib.db_batch_sum(0, 1, _ptr(pts), _ptr(two), -1) == -1


@pytest.mark.parametrize("n", [1, 64, 65])
def test_lines_msg(pp, world, n):
    w = world
    tab = _sent32(n + 1, R.MSG_WORDS)
    for i in range(n + 1):
        tab[i, :R.HM_WORDS] = w.tab0[i % 6, :R.HM_WORDS]
    before = tab.copy()
    pp.lines_msg(tab, n, guard=0)
    assert (tab == before).all()  # the guard byte 0: the table stays the sentinel
    outs = []
    for guard in (1, None):
        t = before.copy()
        pp.lines_msg(t, n, guard=guard)
        outs.append(t)
        assert (t[:, :R.HM_WORDS] == before[:, :R.HM_WORDS]).all() and untouched(t[n, R.HM_WORDS:])
        for i in range(n):
            if i < 6 or i in (n - 1, 63):
                check_chain(World.msg_lines(t, i), w.H[i % 6])
            else:  # the same point: the same lines, bit for bit, as the lane that was checked
                assert (t[i, R.HM_WORDS:] == t[i % 6, R.HM_WORDS:]).all(), i
    assert (outs[0] == outs[1]).all()


def _spoints(world):
    """(group element or None, Jacobian record) x 65 for k_slines: Z = 1, random Z, upper
    representatives; infinity in lanes 0, 30, 63 and 64, as (1, 1, 0), as Z = p and as Z = 0 under
    random X, Y"""
    w, rng = world, random.Random(77)
    out = []
    for u in range(65):
        s = w.sig(2 + u % 4, (u // 4) % 2)
        lam = None if u % 3 == 0 else R.frand(2, rng)
        out.append((s, R.jac_entry(2, s, lam, upper=u % 5 == 2)))
    rnd = R.jac_entry(2, w.H[3], R.frand(2, rng))
    out[0] = (None, R.jac_entry(2, None))
    out[30] = (None, R.jac_entry(2, None, upper=True))  # Z = p
    out[63] = (None, rnd[:48] + [0] * 24)
    out[64] = (None, rnd[:48] + R.words(P) + R.words(0))
    return out


def test_slines(pp, world):
    pts = _spoints(world)
    rec = _u32([r for _, r in pts], 72)
    n, stride = 65, 70

    def check(lines, bad, units, avail):
        """units: unit -> entry; columns from avail on, and those of infinite points, untouched"""
        for u in range(lines.shape[1]):
            col = lines[:, u]
            s = pts[units[u]][0] if u < avail else None
            if s is None:
                assert untouched(col), u
            else:
                check_chain(parse_lines(col), s, R.G1_NEG)
            if bad is not None and u < len(bad):
                assert bad[u] == (SENT8 if u >= avail else (1 if s is None else 0)), u
    lines, bad = pp.slines(n, rec, stride)
    check(lines, bad, list(range(n)), n)
    lines2, none = pp.slines(n, rec, stride, bad=False)  # a null bad
    assert none is None and (lines2 == lines).all()
    g, gb = pp.slines(n, rec, stride, guard=0)
    assert untouched(g) and untouched(gb)
    # list mode: *count below n (the rest untouched) and above n (n units)
    rng = random.Random(78)
    order = list(range(65))
    rng.shuffle(order)
    order = [0, 64] + [e for e in order if e not in (0, 64)] + [5, 6, 7]
    lst = _u32(order)
    for cnt, nn in ((3, 65), (40, 65), (68, 65), (68, 7)):
        lines, bad = pp.slines(nn, rec, stride, list_=lst, count=cnt)
        check(lines, bad, order, min(cnt, nn))


def _eval_inputs(world, n):
    """n groups over the six keys and messages: runs of groups sharing one message, then distinct
    ones; pk_st nonzero in the first, a middle and the last group; P in both representatives"""
    w = world
    pi = [(3 * g + g // 6) % 6 for g in range(n)]
    mi = [0 if g < 4 else (g % 6) for g in range(n)]
    st = [0] * n
    for g in {0, n // 2, n - 1} if n > 1 else ():
        st[g] = 1 + g % 3
    pk = _u32([g1a(w.P[i], upper=g % 2 == 1) for g, i in enumerate(pi)], 28)
    return pi, mi, st, pk


@pytest.mark.parametrize("n", [1, 64, 65])
def test_lines_at_p_and_mml_eval(pp, world, n):
    """both producers of evaluated lines on the same inputs: line j of group g at ev[j n + g] is the
    oracle's line of H(m_g) at P_g; a nonzero pk_st gives the unit line in all 68 rows"""
    w = world
    pi, mi, st, pk = _eval_inputs(w, n)
    for at_p in (True, False):
        for pk_st in ((_u8(st), None) if n == 1 else (_u8(st),)):
            ev = pp.eval_lines(at_p, pk, pk_st, _u32(mi), w.tab)
            for g in range(n):
                if pk_st is not None and st[g]:
                    assert (ev[:, g] == _u32(UNIT_LINE)).all(), (at_p, g)
                else:
                    check_chain(parse_lines(ev[:, g]), w.H[mi[g]], w.P[pi[g]])


# ---- k_pair3 ------------------------------------------------------------------------------------
# (key, message entry, pk_st, P.inf) per case of the (P, H(m)) loop; entry 6 is H_0 flagged infinite
ML_CASES = [(0, 0, 0, 0), (1, 1, 0, 0), (2, 2, 0, 0), (3, 3, 5, 0), (4, 4, 0, 1), (5, 6, 0, 0), (2, 0, 0, 0), (3, 5, 0, 0),
            (5, 1, 1, 1)]


@pytest.mark.parametrize("n", SHAPES3)
def test_pair3_ml(pp, world, n):
    """P3_ML: the stored value is exactly the Python schedule over the table's lines at P; one where
    pk_st is nonzero; f_bad; entry e at f_out[2 e + 1], the other half untouched"""
    w = world
    L = len(ML_CASES)
    for rot in range(L):
        cs = [ML_CASES[(u + rot) % L] for u in range(n)]
        pk = _u32([g1a(w.P[i], upper=u % 2 == 0, inf=bool(pinf)) for u, (i, m, s, pinf) in enumerate(cs)], 28)
        f_out, f_bad = _sent32(2 * n, R.F12_WORDS), _sent8(n)
        pp.pair3(ML, n=n, pk=pk, pk_st=_u8(c[2] for c in cs), msg_idx=_u32([c[1] for c in cs]), hm=w.tab, f_out=f_out,
                 f_bad=f_bad, f_out_stride=2, f_out_off=1)
        assert untouched(f_out[0::2])
        for u, (i, m, s, pinf) in enumerate(cs):
            assert f12(f_out[2 * u + 1]) == (B.P12_ONE if s else w.ml_value(i, m)), (n, rot, u)
            assert f_bad[u] == (1 if (s or pinf or m == 6) else 0), (n, rot, u)
    # plain placement, no pk_st, no f_bad
    f_out = _sent32(n, R.F12_WORDS)
    pp.pair3(ML, n=n, pk=pk, msg_idx=_u32([c[1] for c in cs]), hm=w.tab, f_out=f_out)
    for u, (i, m, s, pinf) in enumerate(cs):
        assert f12(f_out[u]) == w.ml_value(i, m)
    if n == 1:  # one route per (P, Q) through the exponentiation
        for i, m in ((0, 0), (1, 1), (2, 2)):
            assert R.pow3(w.ml_value(i, m)) == R.pairing3(w.P[i], w.H[m])


def _mls_points(world):
    w = world
    return [w.sig(2, 0), w.sig(3, 1), w.sig(0, 2), w.sig(1, 3), w.H[5]]


@pytest.mark.parametrize("n", SHAPES3)
def test_pair3_mls(pp, world, n):
    """P3_MLS over k_slines' lines (stride above n): exactly the Python schedule over those lines"""
    pts = _mls_points(world)
    cols = sig_columns(pp, pts)
    L = len(pts)
    for rot in range(L):
        cs = [cols[(u + rot) % L] for u in range(n)]
        f_out = _sent32(2 * n, R.F12_WORDS)
        pp.pair3(MLS, n=n, stride=n + 2, sig_lines=sig_lines_of(cs, n + 2), f_out=f_out, f_out_stride=2)
        assert untouched(f_out[1::2])
        for u, c in enumerate(cs):
            assert f12(f_out[2 * u]) == c[2], (n, rot, u)
    if n == 1:
        assert R.pow3(cols[0][2]) == R.pairing3(R.G1_NEG, pts[0])


@pytest.mark.parametrize("f_n", [1, 4, 5, 7, 85])
@pytest.mark.parametrize("f_range", ["MML_PAIRS", 1])
def test_pair3_mml(pp, world, f_range, f_n):
    """P3_MML over the lines of k_mml_eval and of k_lines_at_p: exactly the shared-squarings schedule
    over those evaluated lines; after exponentiation the product of the members' P3_ML values"""
    w = world
    f_range = pp.mml_pairs if f_range == "MML_PAIRS" else f_range
    pi, mi, st, pk = _eval_inputs(w, f_n)
    if f_n == 7:
        st = [1, 0, 0, 0, 0, 2, 1]  # not READY: first of a unit, the middle and the end of the short tail
    elif f_n > 4:
        st[-1], st[-2] = 0, 2       # a READY pair alone in the short tail, behind one that is not
    n = (f_n + f_range - 1) // f_range
    for at_p in (False, True):
        ev = pp.eval_lines(at_p, pk, _u8(st), _u32(mi), w.tab)
        f_out = _sent32(n + 1, R.F12_WORDS)
        pp.pair3(MML, n=n, f_range=f_range, f_n=f_n, sig_lines=ev, f_out=f_out, f_out_off=1)
        assert untouched(f_out[0])
        chains = [parse_lines(ev[:, g]) for g in range(f_n)]
        for e in range(n):
            members = range(e * f_range, min((e + 1) * f_range, f_n))
            got = f12(f_out[e + 1])
            assert got == R.miller_from_lines(*[chains[g] for g in members]), (at_p, e)
            if e in (0, n - 1) and f_n in (5, 7):
                ml = p12_prod(w.ml_value(pi[g], mi[g]) for g in members if not st[g])
                assert R.pow3(got) == R.pow3(ml), (at_p, e)


@pytest.mark.parametrize("f_range,f_n", [(1, 43), (3, 64), ("PROD_FAN", 13), ("PROD_FAN", 1), (3, 127)])
def test_pair3_prod(pp, f_range, f_n):
    """P3_PROD: the product of the range's stored values, exactly the oracle's _p12_mul chain; a tail
    unit with fewer than f_range values; placement by stride and offset"""
    f_range = pp.prod_fan if f_range == "PROD_FAN" else f_range
    rng = random.Random(300 + f_n)
    vals = [[rng.randrange(P) for _ in range(12)] for _ in range(min(f_n, 9))] + [B.P12_ONE]
    idx = [rng.randrange(len(vals)) for _ in range(f_n)]
    f_in = _u32([R.f12_words(vals[i], upper=k % 3 == 1) for k, i in enumerate(idx)], 144)
    n = (f_n + f_range - 1) // f_range
    assert f_n % f_range or f_range == 1
    f_out = _sent32(2 * n, R.F12_WORDS)
    pp.pair3(PROD, n=n, f_range=f_range, f_n=f_n, f_in=f_in, f_out=f_out, f_out_stride=2, f_out_off=1)
    assert untouched(f_out[0::2])
    for e in range(n):
        want = p12_prod(vals[i] for i in idx[e * f_range:(e + 1) * f_range])
        assert f12(f_out[2 * e + 1]) == want, e
    f_out = _sent32(n, R.F12_WORDS)
    pp.pair3(PROD, n=n, f_range=f_range, f_n=f_n, f_in=f_in, f_out=f_out)
    assert f12(f_out[n - 1]) == p12_prod(vals[i] for i in idx[(n - 1) * f_range:])


def _fin_world(pp, world):
    """Stored values for the final exponentiations, all computed on the device and matched above:
    per valid group g its two factors ML(P, H) and MLS(S = sk H); a wrong signature's MLS"""
    w = world
    groups = [(2, 0), (3, 1), (0, 2), (1, 3), (4, 4), (5, 5)]
    sigs = [w.sig(i, m) for i, m in groups] + [w.sig(3, 0)]
    cols = sig_columns(pp, sigs)
    n = len(groups)
    f_out = _sent32(n, R.F12_WORDS)
    pp.pair3(ML, n=n, pk=_u32([g1a(w.P[i]) for i, _ in groups], 28), msg_idx=_u32([m for _, m in groups]), hm=w.tab, f_out=f_out)
    ml = [f_out[g].copy() for g in range(n)]
    for g, (i, m) in enumerate(groups):
        assert f12(ml[g]) == w.ml_value(i, m)
    f_out = _sent32(len(sigs), R.F12_WORDS)
    pp.pair3(MLS, n=len(sigs), stride=len(sigs), sig_lines=sig_lines_of(cols), f_out=f_out)
    mls = [f_out[g].copy() for g in range(len(sigs))]
    for g in range(len(sigs)):
        assert f12(mls[g]) == cols[g][2]
    return groups, cols, ml, mls


@pytest.fixture(scope="module")
def fin_world(pp, world):
    return _fin_world(pp, world)


def test_pair3_fin_with_sig_lines(pp, world, fin_world):
    """P3_FIN with sig_lines: its own (-g1, S) loop times the stored (P, H) loops, exponentiated: OK
    for a valid group, NOT_VERIFIED for a wrong signature, 1 behind a nonzero pk_st; f_range 2 with
    an odd f_n: the last unit's short tail"""
    groups, cols, ml, mls = fin_world
    G = len(groups)
    one = _u32(R.f12_words(B.P12_ONE))
    for n in SHAPES3:
        for rot in range(G):
            gs = [(u + rot) % G for u in range(n)]
            wrong = [u % 5 == 3 for u in range(n)]
            pk_st = _u8(3 if u % 7 == 4 else 0 for u in range(n))
            lines = sig_lines_of([cols[G] if wr else cols[g] for g, wr in zip(gs, wrong)], n + 1)
            want = [1 if pk_st[u] else (ST_NOT_VERIFIED if wrong[u] else ST_OK) for u in range(n)]
            status = _sent8(n)
            pp.pair3(FIN, n=n, stride=n + 1, sig_lines=lines, f_range=1, f_n=n, f_in=_u32([ml[g] for g in gs], 144),
                     pk_st=pk_st, status=status)
            assert list(status) == want, (n, rot)
            # two stored values per unit, the second one; the last unit has the first alone
            f_in = np.concatenate([np.stack([ml[g], one]) for g in gs])[:2 * n - 1]
            status = _sent8(n)
            pp.pair3(FIN, n=n, stride=n + 1, sig_lines=lines, f_range=2, f_n=2 * n - 1, f_in=f_in, status=status)
            assert list(status) == [ST_NOT_VERIFIED if wr else ST_OK for wr in wrong], (n, rot)


@pytest.mark.parametrize("n", [1, 3, 4, 7, 10, 11, 21, 22, 43])
def test_final_exponentiation_routes(pp, fin_world, n):
    """P3_FIN without sig_lines (every n), k_pair6_fin<3> (n = 1, 3, 4, 7) and k_pair6_fin<10> (n = 1, 10,
    11, 21) over the same stored values give the same bytes: a batch of two valid groups (four factors) is OK,
    a batch with one wrong member NOT_VERIFIED, a nonzero pk_st gives 1, and the last unit is a short
    tail of one group (cnt = 2 < f_range = 4)"""
    groups, cols, ml, mls = fin_world
    G = len(groups)
    for rot in range(G):
        vals, want = [], []
        for u in range(n):
            a, b = (2 * u + rot) % G, (2 * u + 1 + rot) % G
            wrong = u % 4 == 2
            vals += [ml[a], mls[a], ml[b], mls[G] if wrong else mls[b]]
            want.append(ST_NOT_VERIFIED if wrong else ST_OK)
        f_n = 4 * n - 2  # the last unit: its first group alone
        want[n - 1] = ST_OK
        f_in = _u32(np.stack(vals[:f_n]), 144)
        pk_st = _u8(2 if u % 5 == 1 else 0 for u in range(n))
        want_st = [1 if pk_st[u] else want[u] for u in range(n)]
        routes = {}
        st = _sent8(n)
        pp.pair3(FIN, n=n, f_range=4, f_n=f_n, f_in=f_in, pk_st=pk_st, status=st)
        routes["P3_FIN"] = list(st)
        if n in (1, 3, 4, 7):
            routes["pair6<3>"] = list(pp.pair6_fin(3, n, 4, f_n, f_in, pk_st))
        if n in (1, 10, 11, 21):
            routes["pair6<10>"] = list(pp.pair6_fin(10, n, 4, f_n, f_in, pk_st))
        for name, got in routes.items():
            assert got == want_st, (name, n, rot)
        if rot == 0:  # no pk_st; the guard byte 0
            assert list(pp.pair6_fin(3 if n in (1, 3, 4, 7) else 10, n, 4, f_n, f_in)) == want
            assert untouched(pp.pair6_fin(3, n, 4, f_n, f_in, pk_st, guard=0))
            assert untouched(pp.pair6_fin(10, n, 4, f_n, f_in, pk_st, guard=0))
            assert list(pp.pair6_fin(10, n, 4, f_n, f_in, pk_st, guard=1)) == want_st


# P3_FULL: (key, message entry, signer key, signed message, pk_st, sig_st, P.inf, sig_inf) -> status
FULL_CASES = [
    ((2, 0, 2, 0, 0, 0, 0, 0), ST_OK),
    ((2, 0, 3, 0, 0, 0, 0, 0), ST_NOT_VERIFIED),   # another key's signature, next to a valid one
    ((0, 1, 0, 1, 0, 0, 0, 0), ST_OK),             # P = g1
    ((1, 2, 1, 2, 0, 0, 0, 0), ST_OK),             # P = (r - 1) g1
    ((3, 3, 3, 3, 1, 0, 0, 0), ST_BAD_PUBKEY),     # each of the states over an otherwise valid unit
    ((3, 3, 3, 3, 0, 1, 0, 0), ST_BAD_SIGNATURE),
    ((3, 3, 3, 3, 7, 9, 1, 1), ST_BAD_PUBKEY),     # pk_st before sig_st before infinity
    ((3, 3, 3, 3, 0, 4, 1, 1), ST_BAD_SIGNATURE),
    ((4, 4, 4, 4, 0, 0, 1, 0), ST_NOT_VERIFIED),   # infinity before the (passing) pairing: P, S, H(m)
    ((4, 4, 4, 4, 0, 0, 0, 1), ST_NOT_VERIFIED),
    ((5, 6, 5, 0, 0, 0, 0, 0), ST_NOT_VERIFIED),
    ((4, 4, 4, 4, 0, 0, 0, 0), ST_OK),
    ((5, 3, 5, 5, 0, 0, 0, 0), ST_NOT_VERIFIED),   # a valid signature over another message
]


def _full_arrays(world, cases, upper=lambda u: u % 2 == 1):
    w = world
    c = [k for k, _ in cases]
    return dict(pk=_u32([g1a(w.P[k[0]], upper=upper(u), inf=bool(k[6])) for u, k in enumerate(c)], 28),
                msg_idx=_u32([k[1] for k in c]), pk_st=_u8(k[4] for k in c), sig_st=_u8(k[5] for k in c),
                sig_inf=_u8(k[7] for k in c))


@pytest.mark.parametrize("n", SHAPES3)
def test_pair3_full_direct(pp, world, n):
    """P3_FULL, direct mode: both loops, the exponentiation and the verdict rules, every case in every
    unit"""
    w = world
    cols = sig_columns(pp, [w.sig(k[2], k[3]) for k, _ in FULL_CASES])
    L = len(FULL_CASES)
    for rot in range(L):
        idx = [(u + rot) % L for u in range(n)]
        status = _sent8(n)
        pp.pair3(FULL, n=n, n_items=n, stride=n, sig_lines=sig_lines_of([cols[i] for i in idx]), hm=w.tab, status=status,
                 **_full_arrays(w, [FULL_CASES[i] for i in idx]))
        assert list(status) == [FULL_CASES[i][1] for i in idx], (n, rot)
    # null state arrays: the pairing and the infinity flags decide
    arr = _full_arrays(w, [FULL_CASES[i] for i in idx])
    status = _sent8(n)
    pp.pair3(FULL, n=n, n_items=n, stride=n, sig_lines=sig_lines_of([cols[i] for i in idx]), hm=w.tab, status=status,
             pk=arr["pk"], msg_idx=arr["msg_idx"])
    for u, i in enumerate(idx):
        k = FULL_CASES[i][0]
        assert status[u] == (ST_NOT_VERIFIED if (k[6] or k[1] == 6 or k[:2] != k[2:4]) else ST_OK), u


def test_pair3_full_list(pp, world):
    """P3_FULL, list mode: unit u is entry list[base + u] while base + u < *count; entries >= n_items
    are folded aggregates (agg_pk, agg_msg, agg_status: no pk_st / sig_st / sig_inf of their own);
    *count below or at base writes nothing"""
    w = world
    L = len(FULL_CASES)
    aggs = [((5, 5, 5, 5, 0, 0, 0, 0), ST_OK), ((0, 2, 1, 2, 0, 0, 0, 0), ST_NOT_VERIFIED), ((2, 1, 2, 1, 0, 0, 1, 0), ST_NOT_VERIFIED),
            ((3, 6, 3, 0, 0, 0, 0, 0), ST_NOT_VERIFIED)]
    lst = [5, L + 1, 0, 1, L + 0, 9, L + 2, 2, 12, 0, L + 3, 4, 6, 10, 3, L + 0, 11, 8, 7, L + 1, 1, 0, 2, 3, 5, 12, L + 2, 4]
    every = FULL_CASES + aggs
    cols = sig_columns(pp, [w.sig(k[2], k[3]) for k, _ in every])
    arr = _full_arrays(w, FULL_CASES)
    agg = _full_arrays(w, aggs, upper=lambda u: u == 0)
    for base, n, counts in ((3, 8, (0, 2, 3, 7, 11, 12, 28)), (0, 23, (22, 23, 28)), (1, 22, (28,))):
        for count in counts:
            avail = max(0, min(count - base, n))
            units = lst[base:base + avail]
            status, agg_status = _sent8(L), _sent8(len(aggs))
            lines = sig_lines_of([cols[e] for e in units] or [cols[0]], n)
            pp.pair3(FULL, n=n, n_items=L, base=base, count=count, list=_u32(lst), stride=n, sig_lines=lines, hm=w.tab,
                     status=status, agg_status=agg_status, agg_pk=agg["pk"], agg_msg=agg["msg_idx"], **arr)
            for e in range(len(every)):
                got = status[e] if e < L else agg_status[e - L]
                assert got == (every[e][1] if e in units else SENT8), (base, n, count, e)


def test_pair3_guard_byte_zero(pp, world, fin_world):
    """with the guard byte 0 no mode writes anything; with the byte 1 each writes what it writes
    without a guard"""
    w = world
    groups, cols, ml, mls = fin_world
    n = 2
    arr = _full_arrays(w, FULL_CASES[:n])
    lines = sig_lines_of(cols[:n])
    f_in = _u32(np.stack([ml[0], mls[0], ml[1], mls[1]]), 144)
    ev = pp.eval_lines(False, arr["pk"], None, arr["msg_idx"], w.tab)
    calls = {
        FULL: dict(n_items=n, stride=n, sig_lines=lines, hm=w.tab, **arr),
        ML: dict(hm=w.tab, pk=arr["pk"], msg_idx=arr["msg_idx"], pk_st=arr["pk_st"]),
        FIN: dict(f_range=2, f_n=4, f_in=f_in),
        PROD: dict(f_range=2, f_n=4, f_in=f_in),
        MML: dict(f_range=1, f_n=2, sig_lines=ev),
        MLS: dict(stride=n, sig_lines=lines),
    }
    for mode, kw in calls.items():
        res = []
        for guard in (0, 1, None):
            outs = dict(status=_sent8(n)) if mode in (FULL, FIN) else dict(f_out=_sent32(n, R.F12_WORDS))
            if mode == ML:
                outs["f_bad"] = _sent8(n)
            pp.pair3(mode, n=n, guard=guard, **kw, **outs)
            if guard == 0:
                assert all(untouched(o) for o in outs.values()), mode
            else:
                assert not any(untouched(o) for o in outs.values()), mode
                res.append(outs)
        assert all((res[0][k] == res[1][k]).all() for k in res[0]), mode


# ---- k_lml --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5])
def test_lml_side0(pp, world, n):
    """k_lml<0>: the (-g1, S) loop straight from a Jacobian S, exponentiated in Python: e(-g1, S)^3;
    bad = 1 for S at infinity; placement by f_stride / f_off; the guard byte"""
    w, rng = world, random.Random(500 + n)
    S = [w.sig(2, 0), w.sig(3, 1), None, w.sig(2, 0), w.sig(0, 2)][:n]
    lam = [None, R.frand(2, rng), None, R.frand(2, rng), R.frand(2, rng)]
    pts = _u32([R.jac_entry(2, s, lam[u], upper=u == 3) for u, s in enumerate(S)], 72)
    f_out, bad = pp.lml(0, n, 2 * n + 1, f_stride=2, f_off=1, pts=pts)
    assert untouched(f_out[0::2])
    for u, s in enumerate(S):
        assert bad[u] == (1 if s is None else 0)
        if s is not None:
            assert R.pow3(f12(f_out[2 * u + 1])) == R.pairing3(R.G1_NEG, s), u
    plain, none = pp.lml(0, n, n, pts=pts, bad=False, guard=1)
    assert none is None and (plain == f_out[1::2]).all()
    g, gb = pp.lml(0, n, n, pts=pts, guard=0)
    assert untouched(g) and untouched(gb)


def test_lml_side1(pp, world):
    """k_lml<1>: the (P, H(m)) loop from the table's affine H(m) (the table's lines are not read: the
    table goes up without them), exponentiated in Python: e(P, H)^3; bad for pk_st, P.inf and hm.inf
    each alone; units sharing one message"""
    w = world
    cases = [(0, 0, 0, 0), (2, 0, 0, 0), (1, 1, 0, 0), (2, 0, 3, 0), (2, 0, 0, 1), (2, 6, 0, 0), (2, 2, 0, 0)]
    n = len(cases)
    pk = _u32([g1a(w.P[i], upper=u % 2 == 1, inf=bool(pinf)) for u, (i, m, s, pinf) in enumerate(cases)], 28)
    kw = dict(pk=pk, msg_idx=_u32([c[1] for c in cases]), tab=w.tab0)
    f_out, bad = pp.lml(1, n, n + 3, f_off=3, pk_st=_u8(c[2] for c in cases), **kw)
    assert untouched(f_out[:3])
    for u, (i, m, s, pinf) in enumerate(cases):
        assert bad[u] == (1 if (s or pinf or m == 6) else 0), u
        if not bad[u]:  # a unit that fails without its pairing: its value is never used
            assert R.pow3(f12(f_out[3 + u])) == R.pairing3(w.P[i], w.H[m]), u
    f1, b1 = pp.lml(1, 1, 1, pk=pk[:1], msg_idx=_u32([1]), tab=w.tab0)  # n = 1, a null pk_st
    assert b1[0] == 0 and R.pow3(f12(f1[0])) == R.pairing3(w.P[0], w.H[1])
    g, gb = pp.lml(1, n, n, guard=0, **kw)
    assert untouched(g) and untouched(gb)
    f2, b2 = pp.lml(1, n, n, guard=1, **kw)
    assert (f2 == f_out[3:]).all() and list(b2) == [1 if (pinf or m == 6) else 0 for _, m, _, pinf in cases]


# ---- the group stage ----------------------------------------------------------------------------
_A1, _T2 = {}, {}


def A1(k):
    k %= B.R
    if k not in _A1:
        _A1[k] = B.g1_mul(B.G1_GEN, k)
    return _A1[k]


def T2(k):
    k %= B.R
    if k not in _T2:
        _T2[k] = B.g2_mul(B.G2_GEN, k)
    return _T2[k]


def item(k, m, pk_st=0, pk_inf=0, sig_st=0, sig_inf=0, pr="own", sr="own"):
    """An item: key k g1, signature (100 + k) G2 (the group stage checks no signature), message entry m,
    its states, and the scalars of its combined points pr = (3 k + 1) g1, sr = (5 k + 2) G2 -- the point
    at infinity (None) for an unusable item, as the combination kernels leave it"""
    usable = not (pk_st or pk_inf or sig_st or sig_inf)
    return dict(k=k, m=m, pk_st=pk_st, pk_inf=pk_inf, sig_st=sig_st, sig_inf=sig_inf, usable=usable,
                pr=(3 * k + 1 if usable else None) if pr == "own" else pr,
                sr=(5 * k + 2 if usable else None) if sr == "own" else sr)


def fold(k, st=0, pk_st=0, pk_inf=0, sig_inf=0):
    return dict(k=k, st=st, pk_st=pk_st, pk_inf=pk_inf, sig_inf=sig_inf, pr=7 * k + 3, sr=11 * k + 5)


def _group_cases():
    """(name, items, folded aggregate): group_scan's rules, one case per branch"""
    bad = [dict(pk_st=2), dict(sig_st=1), dict(pk_inf=1), dict(sig_inf=1)]  # the four reasons an item is unusable
    c = [("one", [item(2, 0)], None),                         # kind 0: the decoded points, copied
         ("two", [item(3, 1), item(4, 1)], None),
         ("five", [item(k, 2) for k in range(5, 10)], None),
         ("empty_group", [], None)]                            # no item at all: EMPTY, message 0
    for j, b in enumerate(bad):                               # each reason first, in the middle, last
        for pos in range(3):
            its = [item(10 + 3 * j + i, 3) for i in range(3)]
            its[pos] = item(10 + 3 * j + pos, 5, **b)         # another message: an unusable item's does not count
            c.append((f"unusable{j}.{pos}", its, None))
    c += [("all_unusable", [item(30 + j, 4 + (j == 0), **b) for j, b in enumerate(bad)], None),   # EMPTY, gmsg of item 0
          ("all_unusable_fold", [item(35, 1, sig_st=3)], fold(36)),                              # cnt = 0: the aggregate too
          ("inconsistent", [item(40, 0), item(41, 1)], None),                                    # FALLBACK
          ("inconsistent_last", [item(42, 2), item(43, 2), item(44, 2), item(45, 2), item(46, 0)], fold(47)),
          ("hm_inf", [item(50, 6), item(51, 6)], None),                                          # EMPTY unless skip_hm
          ("one_of_three", [item(52, 1, pk_st=1), item(53, 4), item(54, 1, sig_inf=1)], None),   # kind 0: copied
          ("fold", [item(55, 5), item(56, 5)], fold(57)),
          ("one_fold", [item(58, 0)], fold(59)),                                                 # summed, not copied
          ("fold_st", [item(60, 1)], fold(61, st=4)),                                            # ignored: each reason
          ("fold_pk_st", [item(62, 2)], fold(63, pk_st=1)),
          ("fold_pk_inf", [item(64, 3), item(65, 3)], fold(66, pk_inf=1)),
          ("fold_sig_inf", [item(67, 4)], fold(68, sig_inf=1)),
          ("keys_only", [item(70, 5), item(71, 5, sig_st=2, pr=3 * 71 + 1)], None),              # a key whose signature failed
          ("p_cancels", [item(72, 0, pr=777), item(73, 0, pr=-777)], None),                      # P infinite: FALLBACK
          ("s_cancels", [item(74, 1, sr=888), item(75, 1), item(76, 1, sr=-888 - (5 * 75 + 2))], None)]
    return c


def _sum(field, pts):
    acc = None
    for p in pts:
        acc = R.ec_add(field, acc, p)
    return acc


_GEXP = {}


def group_expect(pp, case, kind, keys_only, skip_hm):
    """(state, message, P, S) of a group by vgroup.hip's written rules and the oracle's group law"""
    key = (case[0], case[2] is not None, kind, keys_only, skip_hm)
    if key in _GEXP:
        return _GEXP[key]
    _, items, agg = case
    us = [it for it in items if it["usable"]]
    m = us[0]["m"] if us else (items[0]["m"] if items else 0)
    with_agg = bool(agg and us and not (agg["st"] or agg["pk_st"] or agg["pk_inf"] or agg["sig_inf"]))
    if not us or (not skip_hm and m == 6):
        res = (pp.G_EMPTY, m, None, None)
    elif any(it["m"] != m for it in us):
        res = (pp.G_FALLBACK, m, None, None)
    elif kind == 0 and len(us) == 1 and not with_agg:
        res = (pp.G_READY, m, A1(us[0]["k"]), T2(100 + us[0]["k"]))
    else:
        summed = [it for it in items if it["usable"] or not keys_only] + ([agg] if with_agg else [])
        Ps = _sum(1, [A1(it["pr"]) for it in summed if it["pr"] is not None])
        Ss = _sum(2, [T2(it["sr"]) for it in summed if it["sr"] is not None])
        if Ps is None or (kind != 2 and Ss is None):
            res = (pp.G_FALLBACK, m, None, None)
        else:
            res = (pp.G_READY, m, Ps, Ss)
    _GEXP[key] = res
    return res


def _group_arrays(world, groups, with_off, with_fold, seed):
    """the input arrays of a launch over these group cases"""
    rng = random.Random(seed)
    items = [it for _, its, _ in groups for it in its]
    off = [0]
    for _, its, _ in groups:
        off.append(off[-1] + len(its))
    if not with_off:
        assert all(len(its) == 1 for _, its, _ in groups)

    def jac(field, pt):
        return R.jac_entry(field, pt, R.frand(field, rng) if rng.random() < 0.7 else None, upper=rng.random() < 0.3)
    a = dict(grp_off=_u32(off) if with_off else None, msg_idx=_u32([it["m"] for it in items]), hm=world.tab0,
             pk=_u32([g1a(A1(it["k"]), upper=i % 2 == 1, inf=bool(it["pk_inf"])) for i, it in enumerate(items)], 28),
             pk_st=_u8(it["pk_st"] for it in items), sig_st=_u8(it["sig_st"] for it in items),
             sig=_u32([hme(T2(100 + it["k"]), upper=i % 3 == 1, inf=bool(it["sig_inf"])) for i, it in enumerate(items)], 52),
             pr=_u32([jac(1, None if it["pr"] is None else A1(it["pr"])) for it in items], 36),
             sr=_u32([jac(2, None if it["sr"] is None else T2(it["sr"])) for it in items], 72))
    if with_fold:
        fs = [f or fold(90, st=1) for _, _, f in groups]  # a group without an aggregate: one that failed
        a.update(agg_pk=_u32([g1a(A1(f["k"]), inf=bool(f["pk_inf"])) for f in fs], 28), agg_pk_st=_u8(f["pk_st"] for f in fs),
                 agg_sig=_u32([hme(T2(100 + f["k"]), inf=bool(f["sig_inf"])) for f in fs], 52), agg_st=_u8(f["st"] for f in fs),
                 agg_pr=_u32([jac(1, A1(f["pr"])) for f in fs], 36), agg_sr=_u32([jac(2, T2(f["sr"])) for f in fs], 72))
    return a


def _run_groups(pp, world, kind, groups, g0, ng, with_off=True, with_fold=True, fe_batch=0, keys_only=0, skip_hm=0, bS=True,
                seed=1):
    """one launch over groups [g0, g0 + ng) of `groups`, every output compared"""
    if not with_fold:
        groups = [(n, its, None) for n, its, _ in groups]
    a = _group_arrays(world, groups, with_off, with_fold, seed)
    fb = fe_batch or pp.fe_batch
    nb = (ng + fb - 1) // fb
    a.update(gP=_sent32(ng, 28), gmsg=_sent32(len(groups)), gst=_sent8(ng))
    if kind == 0:
        a["glines"] = _sent32(R.N_LINES, ng, R.LINE_WORDS)
    if kind == 1:
        a["gS"] = _sent32(ng, 72)
        a["bS"] = _sent32(nb, 72) if bS else None
    pp.group_prep(kind, a, g0, ng, fe_batch, keys_only, skip_hm)
    sums = [None] * nb
    for g, case in enumerate(groups):
        lg = g - g0
        if not 0 <= lg < ng:
            assert a["gmsg"][g] == SENT32, (case[0], g)
            continue
        st, m, Pw, Sw = group_expect(pp, case, kind, keys_only, skip_hm)
        tag = (kind, case[0], lg)
        assert (a["gst"][lg], a["gmsg"][g]) == (st, m), tag
        if st != pp.G_READY:
            assert untouched(a["gP"][lg]), tag
            if kind == 0:
                assert untouched(a["glines"][:, lg]), tag
            if kind == 1:
                assert below_2p(a["gS"][lg]) and R.entry_affine(2, [int(v) for v in a["gS"][lg]]) is None, tag
            continue
        gp = [int(v) for v in a["gP"][lg]]
        assert below_2p(gp[:24]) and gp[24:] == [0, 0, 0, 0], tag
        assert (R.unmont(R.from_words(gp[:12])), R.unmont(R.from_words(gp[12:24]))) == Pw, tag
        if kind == 0:
            check_chain(parse_lines(a["glines"][:, lg]), Sw, R.G1_NEG)
        if kind == 1:
            assert below_2p(a["gS"][lg]) and R.entry_affine(2, [int(v) for v in a["gS"][lg]]) == Sw, tag
            sums[lg // fb] = R.ec_add(2, sums[lg // fb], Sw)
    if kind == 1 and bS:
        for b in range(nb):
            assert below_2p(a["bS"][b]) and R.entry_affine(2, [int(v) for v in a["bS"][b]]) == sums[b], (kind, "batch", b)
    return a


def _tiled(cases, n_groups, rot):
    return [cases[(g + rot) % len(cases)] for g in range(n_groups)]


@pytest.mark.parametrize("kind", [0, 2])
def test_group_prep(pp, world, kind):
    """k_group_prep (kind 0: the lines of the group's S at -g1) and k_group_prep_p (kind 2: the key
    side and the state only) against group_scan's rules: every case alone (ng = 1, g0 > 0), 65
    groups over two waves, groups of one item without grp_off, with and without aggregates,
    keys_only and skip_hm"""
    cases = _group_cases()
    C = len(cases)
    for rot in range(C):
        _run_groups(pp, world, kind, _tiled(cases, 4, rot), 2, 1, keys_only=rot % 2, skip_hm=rot % 3 == 0, seed=rot)
    for rot, ko, sk in ((0, 0, 0), (9, 1, 1)):
        _run_groups(pp, world, kind, _tiled(cases, 68, rot), 2, 65, keys_only=ko, skip_hm=sk, seed=100 + rot)
    _run_groups(pp, world, kind, _tiled(cases, 30, 3), 0, 30, with_fold=False, seed=7)
    single = [c for c in cases if len(c[1]) == 1]
    _run_groups(pp, world, kind, _tiled(single, 9, 0), 1, 7, with_off=False, seed=8)
    _run_groups(pp, world, kind, _tiled(single, 9, 2), 1, 7, with_off=False, with_fold=False, seed=9)


@pytest.mark.parametrize("fe_batch,keys_only,skip_hm", [(0, 0, 0), (4, 1, 0), (64, 0, 1)])
@pytest.mark.parametrize("ng", [1, 63, 64, 65])
def test_group_prep_batch(pp, world, ng, fe_batch, keys_only, skip_hm):
    """k_group_prep_b: every group's S kept (infinity unless READY) and the butterfly's sum over each
    batch of fe_batch consecutive groups, the last batch and the last wave partly filled"""
    cases = _group_cases()
    for rot in (range(len(cases)) if ng == 1 else (0, 11)):
        _run_groups(pp, world, 1, _tiled(cases, ng + 3, rot), 2, ng, fe_batch=fe_batch, keys_only=keys_only, skip_hm=skip_hm,
                    seed=200 + rot)
    _run_groups(pp, world, 1, _tiled(cases, ng + 3, 5), 2, ng, fe_batch=fe_batch, bS=False, with_fold=False, seed=300)
    single = [c for c in cases if len(c[1]) == 1]
    _run_groups(pp, world, 1, _tiled(single, ng, 1), 0, ng, with_off=False, fe_batch=fe_batch, seed=301)


def test_group_prep_batch_guard(pp, world):
    cases = _group_cases()
    a = _group_arrays(world, _tiled(cases, 5, 0), True, True, 1)
    for guard in (0, 1):
        a.update(gP=_sent32(5, 28), gmsg=_sent32(5), gst=_sent8(5), gS=_sent32(5, 72), bS=_sent32(2, 72))
        pp.group_prep(1, a, 0, 5, fe_batch=4, guard=guard)
        assert all(untouched(a[k]) == (guard == 0) for k in ("gmsg", "gst", "gS", "bS")), guard


@pytest.mark.parametrize("ng,k", [(7, "MML_PAIRS"), (9, 1), (65, 1), (261, "MML_PAIRS")])
def test_batch_sum(pp, ng, k):
    """k_batch_sum: the sum of each k consecutive S_g (infinity for groups that are not READY), ng no
    multiple of k, one block and two"""
    k = pp.mml_pairs if k == "MML_PAIRS" else k
    assert ng % k or k == 1
    rng = random.Random(900 + ng)
    pts = [None if g % 7 in (0, 3) or g % 8 == 5 else T2(200 + g % 11) for g in range(ng)]
    pts[-1] = T2(3)
    for g in range(4, ng - 4, 16):  # a batch that cancels
        pts[g - g % 4:g - g % 4 + 4] = [T2(50), None, T2(-50 - 9), T2(9)]
    rec = []
    for g, s in enumerate(pts):
        w = R.jac_entry(2, s, R.frand(2, rng) if g % 3 else None, upper=g % 4 == 1)
        if s is None and g % 2:
            w = R.jac_entry(2, T2(5), R.frand(2, rng))[:48] + [0] * 24  # Z = 0 under some X, Y
        rec.append(w)
    gS = _u32(rec, 72)
    bS = pp.batch_sum(gS, k)
    for b in range(len(bS)):
        assert below_2p(bS[b]) and R.entry_affine(2, [int(v) for v in bS[b]]) == _sum(2, [s for s in pts[b * k:(b + 1) * k] if s]), b
    assert untouched(pp.batch_sum(gS, k, guard=0)) and (pp.batch_sum(gS, k, guard=1) == bS).all()
