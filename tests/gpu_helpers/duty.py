"""Duty sessions (hbls_duty_open / _add / _state / _stats / _close) beside hbls_slot_select_batch on
the same candidate stream, for tests/test_gpu_duty.py.

A *stream* is a dict of host arrays in arrival order: pks (S x 48), sigs (S x 96), msgs (S x 32),
group (S, uint32; >= G: verify only), idx (S, int64: share indices), dv (G x 48), t.  A *case* is
what tests/test_gpu_slot_host.py gives hbls_slot_select_batch (pks, sigs, msgs, src, idx, goff, dv, t).
Every output array of both calls carries PAD sentinel entries behind it, which must come back
untouched.
"""
import ctypes

import numpy as np

OK, UNCHECKED = 0, 7
NONE = 0xFFFFFFFF
PAD = 64
S8, S32 = 0xA5, 0xA5A5A5A5


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def stream_of(c, verify_only_group=NONE):
    """A case's candidates as a stream, peer-major (every group's first candidate, then every group's
    second, ...: each group's candidates keep their order), then the partials no group lists as
    verify-only entries.  A candidate listed twice is sent twice; one naming no partial is not sent
    (the one-shot call counts it as not verified)."""
    N, G = len(c["pks"]), len(c["goff"]) - 1
    ent = [(j - int(c["goff"][g]), g, int(c["src"][j]), int(c["idx"][j]))
           for g in range(G) for j in range(int(c["goff"][g]), int(c["goff"][g + 1])) if int(c["src"][j]) < N]
    ent.sort(key=lambda e: (e[0], e[1]))
    listed = {e[2] for e in ent}
    ent += [(0, verify_only_group, p, 0) for p in range(N) if p not in listed]
    part = np.asarray([e[2] for e in ent], dtype=np.int64)
    return dict(pks=np.ascontiguousarray(c["pks"][part]), sigs=np.ascontiguousarray(c["sigs"][part]),
                msgs=np.ascontiguousarray(c["msgs"][part]), group=np.asarray([e[1] for e in ent], np.uint32),
                idx=np.asarray([e[3] for e in ent], np.int64), dv=np.ascontiguousarray(c["dv"][:G]), t=c["t"])


def case_of(s):
    """The one-shot case over a stream's concatenation: group g's candidates are its stream positions,
    in stream order."""
    G = len(s["dv"])
    order = [i for g in range(G) for i in np.flatnonzero(s["group"] == g)]
    goff = np.concatenate([[0], np.cumsum([(s["group"] == g).sum() for g in range(G)])]).astype(np.uint32)
    return dict(pks=s["pks"], sigs=s["sigs"], msgs=s["msgs"], src=np.asarray(order, np.uint32),
                idx=s["idx"][order].astype(np.int64), goff=goff, dv=s["dv"], t=s["t"])


def sub_stream(s, keep):
    o = dict(s)
    for k in ("pks", "sigs", "msgs", "group", "idx"):
        o[k] = np.ascontiguousarray(s[k][keep])
    return o


def random_cuts(S, n_adds, seed):
    """n_adds adds over S partials: n_adds - 1 distinct cut points in 1 .. S - 1, seeded."""
    rng = np.random.default_rng(seed)
    cuts = sorted(rng.choice(np.arange(1, S), size=n_adds - 1, replace=False).tolist()) if n_adds > 1 else []
    return [0] + cuts + [S]


class Duty:
    def __init__(self, L, dv, t, max_stored):
        self.L, self.G, self.t = L, len(dv), t
        h = ctypes.c_uint64(0)
        dvb = np.ascontiguousarray(dv).reshape(-1) if len(dv) else np.zeros(48, np.uint8)
        rc = L.hbls_duty_open(_p(dvb), self.G, t, max_stored, ctypes.byref(h))
        assert rc == 0, L.hbls_last_error().decode()
        assert h.value != 0
        self.h = h.value

    def add(self, s, b, e, raw=False):
        """Partials [b, e) of the stream as one add -> dict(first, vst, stored, fired, chosen, out, tst, ast)."""
        L, G, t, n = self.L, self.G, self.t, e - b
        rows = min(n, G)
        pks, sigs, msgs = (np.ascontiguousarray(s[k][b:e]).reshape(-1) if n else np.zeros(96, np.uint8) for k in ("pks", "sigs", "msgs"))
        off = np.arange(max(n, 1), dtype=np.uint64) * 32
        ln = np.full(max(n, 1), 32, dtype=np.uint32)
        grp = np.ascontiguousarray(s["group"][b:e], dtype=np.uint32) if n else np.zeros(1, np.uint32)
        idx = np.ascontiguousarray(s["idx"][b:e], dtype=np.int64) if n else np.zeros(1, np.int64)
        o = dict(vst=np.full(n + PAD, S8, np.uint8), stored=np.full(n + PAD, S8, np.uint8),
                 fired=np.full(rows + PAD, S32, np.uint32), chosen=np.full(rows * t + PAD, S32, np.uint32),
                 out=np.full(96 * rows + PAD, S8, np.uint8), tst=np.full(rows + PAD, S8, np.uint8),
                 ast=np.full(rows + PAD, S8, np.uint8))
        first, nf = ctypes.c_uint32(S32), ctypes.c_size_t(12345)
        rc = L.hbls_duty_add(self.h, _p(pks), _p(sigs), _p(msgs), _p(off), _p(ln), _p(grp), _p(idx), n, _p(o["vst"]),
                             _p(o["stored"]), ctypes.byref(first), _p(o["fired"]), ctypes.byref(nf), _p(o["chosen"]),
                             _p(o["out"]), _p(o["tst"]), _p(o["ast"]))
        if raw:
            return rc
        assert rc == 0, L.hbls_last_error().decode()
        f = nf.value
        assert f <= rows
        size = dict(vst=n, stored=n, fired=f, chosen=f * t, out=96 * f, tst=f, ast=f)
        for k, a in o.items():  # rows past n_fired are not written either
            assert (a[size[k]:] == (S8 if a.dtype == np.uint8 else S32)).all(), "sentinel behind " + k
            o[k] = a[:size[k]]
        o["chosen"], o["out"], o["first"] = o["chosen"].reshape(f, t), o["out"].reshape(f, 96), first.value
        return o

    def state(self):
        cnt, fl = np.full(self.G + PAD, S32, np.uint32), np.full(self.G + PAD, S8, np.uint8)
        assert self.L.hbls_duty_state(self.h, _p(cnt), _p(fl)) == 0, self.L.hbls_last_error().decode()
        assert (cnt[self.G:] == S32).all() and (fl[self.G:] == S8).all()
        return cnt[:self.G], fl[:self.G]

    def stats(self):
        out = np.full(6 + 2, 0xA5A5A5A5A5A5A5A5, np.uint64)
        assert self.L.hbls_duty_stats(self.h, _p(out), 6) == 0, self.L.hbls_last_error().decode()
        assert (out[6:] == 0xA5A5A5A5A5A5A5A5).all()
        return [int(x) for x in out[:6]]

    def close(self):
        assert self.L.hbls_duty_close(self.h) == 0, self.L.hbls_last_error().decode()


def run(L, s, bounds, max_stored=16):
    """The stream through one duty, add k = partials [bounds[k], bounds[k + 1]) -> the union of what
    the adds return, in hbls_slot_select_batch's terms (vst, chosen, out, tst, ast per group; groups
    that never fire keep NONE / zero bytes / UNCHECKED), plus stored (S), fired_in (G: the add a group
    fired in, -1 never), count and flag (hbls_duty_state), stats, and n_fired per add."""
    G, t, S = len(s["dv"]), s["t"], len(s["pks"])
    du = Duty(L, s["dv"], t, max_stored)
    r = dict(vst=np.zeros(S, np.uint8), stored=np.zeros(S, np.uint8), chosen=np.full((G, t), NONE, np.uint32),
             out=np.zeros((G, 96), np.uint8), tst=np.full(G, UNCHECKED, np.uint8), ast=np.full(G, UNCHECKED, np.uint8),
             fired_in=np.full(G, -1, np.int64), per_add=[])
    try:
        for k in range(len(bounds) - 1):
            b, e = bounds[k], bounds[k + 1]
            a = du.add(s, b, e)
            assert a["first"] == b
            r["vst"][b:e], r["stored"][b:e] = a["vst"], a["stored"]
            f = a["fired"].astype(np.int64)
            assert (np.diff(f) > 0).all() and (f < G).all(), "fired: ascending group ids"
            assert (r["fired_in"][f] == -1).all(), "a group fires once"
            r["fired_in"][f] = k
            r["chosen"][f], r["out"][f], r["tst"][f], r["ast"][f] = a["chosen"], a["out"], a["tst"], a["ast"]
            r["per_add"].append(len(f))
        r["count"], r["flag"] = du.state()
        r["stats"] = du.stats()
    finally:
        du.close()
    return r


def check_union(r, one, s, bounds, what=""):
    """The defining property: a duty's union `r` against the one-shot result `one` over case_of(s)."""
    G, t = len(s["dv"]), s["t"]
    assert np.array_equal(r["vst"], one["vst"]), (what, "vstatus")
    fired = r["fired_in"] >= 0
    assert np.array_equal(fired, one["tst"] != UNCHECKED), (what, "fired groups")
    assert np.array_equal(r["flag"] != 0, fired), (what, "fired flags")
    for k in ("out", "tst", "ast"):
        assert np.array_equal(r[k], one[k]), (what, k)
    assert np.array_equal(r["chosen"][fired], one["chosen"][fired]), (what, "chosen")
    # each group fires in the add that holds its t-th member
    last = one["chosen"][fired][:, t - 1].astype(np.int64)
    assert np.array_equal(r["fired_in"][fired], np.searchsorted(np.asarray(bounds), last, side="right") - 1), (what, "firing add")
    # every member was stored; nothing is stored for a group after it fired
    assert r["stored"][one["chosen"][fired].reshape(-1).astype(np.int64)].all(), (what, "members stored")
    for g in np.flatnonzero(~fired):
        mine = np.flatnonzero(s["group"] == g)
        assert r["count"][g] == r["stored"][mine].sum(), (what, "stored count", g)
        if len({bytes(m) for m in s["msgs"][mine]}) <= 1:
            assert r["count"][g] == one["count"][g], (what, "count of a group over one message", g)
    assert not r["stored"][s["group"] >= G].any(), (what, "verify-only partials are not stored")
