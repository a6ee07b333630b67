"""Set-atomic duty adds (hbls_duty_add_sets / hbls_duty_set_stats) beside hbls_duty_add on the same
stream, for tests/test_gpu_duty_sets.py.  Streams, sentinels and the plain calls are tests/gpu_helpers/
duty.py's; every output array of the new call carries PAD sentinel entries behind it as well.
"""
import ctypes

import numpy as np

from duty import NONE, PAD, S8, S32, Duty, _p

OUT_KEYS = ("first", "vst", "stored", "fired", "chosen", "out", "tst", "ast")


class SetsDuty(Duty):
    def add_sets(self, s, b, e, set_off, raw=False, n_sets=None, no_set_first=False, handle=None):
        """Partials [b, e) of the stream as one call of len(set_off) - 1 sets (set_off relative to b) ->
        what Duty.add returns plus set_first.  raw: the return code of a call that must fail, having
        written nothing (set_off None: a NULL pointer with n_sets sets; no_set_first: a NULL set_first)."""
        L, G, t, n = self.L, self.G, self.t, e - b
        n_sets = len(set_off) - 1 if n_sets is None else n_sets
        rows = min(n, G)
        pks, sigs, msgs = (np.ascontiguousarray(s[k][b:e]).reshape(-1) if n else np.zeros(96, np.uint8) for k in ("pks", "sigs", "msgs"))
        off = np.arange(max(n, 1), dtype=np.uint64) * 32
        ln = np.full(max(n, 1), 32, dtype=np.uint32)
        grp = np.ascontiguousarray(s["group"][b:e], dtype=np.uint32) if n else np.zeros(1, np.uint32)
        idx = np.ascontiguousarray(s["idx"][b:e], dtype=np.int64) if n else np.zeros(1, np.int64)
        so = None if set_off is None else np.asarray(set_off, dtype=np.uint32)
        o = dict(vst=np.full(n + PAD, S8, np.uint8), stored=np.full(n + PAD, S8, np.uint8),
                 fired=np.full(rows + PAD, S32, np.uint32), chosen=np.full(rows * t + PAD, S32, np.uint32),
                 out=np.full(96 * rows + PAD, S8, np.uint8), tst=np.full(rows + PAD, S8, np.uint8),
                 ast=np.full(rows + PAD, S8, np.uint8), set_first=np.full(max(n_sets, 0) + PAD, S32, np.uint32))
        first, nf = ctypes.c_uint32(S32), ctypes.c_size_t(12345)
        rc = L.hbls_duty_add_sets(self.h if handle is None else handle, _p(pks), _p(sigs), _p(msgs), _p(off), _p(ln), _p(grp), _p(idx), n, _p(so), n_sets,
                                  _p(o["vst"]), _p(o["stored"]), ctypes.byref(first), None if no_set_first else _p(o["set_first"]), _p(o["fired"]),
                                  ctypes.byref(nf), _p(o["chosen"]), _p(o["out"]), _p(o["tst"]), _p(o["ast"]))
        if raw:
            for k, a in o.items():  # a call error writes nothing
                assert (a == (S8 if a.dtype == np.uint8 else S32)).all(), "a failed call wrote " + k
            assert first.value == S32 and nf.value == 12345
            return rc
        assert rc == 0, L.hbls_last_error().decode()
        f = nf.value
        assert f <= rows
        size = dict(vst=n, stored=n, fired=f, chosen=f * t, out=96 * f, tst=f, ast=f, set_first=n_sets)
        for k, a in o.items():
            assert (a[size[k]:] == (S8 if a.dtype == np.uint8 else S32)).all(), "sentinel behind " + k
            o[k] = a[:size[k]]
        o["chosen"], o["out"], o["first"] = o["chosen"].reshape(f, t), o["out"].reshape(f, 96), first.value
        return o

    def set_stats(self):
        out = np.full(3 + 2, 0xA5A5A5A5A5A5A5A5, np.uint64)
        assert self.L.hbls_duty_set_stats(self.h, _p(out), 3) == 0, self.L.hbls_last_error().decode()
        assert (out[3:] == 0xA5A5A5A5A5A5A5A5).all()
        return [int(x) for x in out[:3]]


def restated_set_first(vst, set_off):
    return [next((i for i in range(set_off[k], set_off[k + 1]) if vst[i] != 0), NONE) for k in range(len(set_off) - 1)]


def same_call(a, b, what=""):
    """every output two calls share, exactly"""
    for k in OUT_KEYS:
        assert np.array_equal(a[k], b[k]), (what, k)


def twin_stream(s, rejected):
    """the stream hbls_duty_add gets on the twin duty: no group for the partials of rejected sets"""
    g = s["group"].copy()
    g[np.asarray(rejected, dtype=bool)] = NONE
    return dict(s, group=g)


def run_pair(L, s, bounds, sets_of_call, max_stored=16, modes=None):
    """The stream through a duty driven by hbls_duty_add_sets (call k = partials [bounds[k], bounds[k + 1])
    in the sets sets_of_call[k], offsets relative to the call) and through its twin driven by
    hbls_duty_add, compared call by call and in their final state.  modes[k] == "add" sends call k of
    the first duty through hbls_duty_add as well (its partials then are singletons of their own).
    -> dict(calls, set_first (per call), rejected (S flags), count, flag, stats, set_stats)"""
    G, t, S = len(s["dv"]), s["t"], len(s["pks"])
    a, b = SetsDuty(L, s["dv"], t, max_stored), SetsDuty(L, s["dv"], t, max_stored)
    res = dict(calls=[], set_first=[], rejected=np.zeros(S, bool))
    seen = rej = lost = 0
    try:
        for k in range(len(bounds) - 1):
            lo, hi = bounds[k], bounds[k + 1]
            if modes and modes[k] == "add":
                r = a.add(s, lo, hi)
                same_call(r, b.add(s, lo, hi), k)
                res["calls"].append(r)
                res["set_first"].append(None)
                continue
            off = list(sets_of_call[k])
            r = a.add_sets(s, lo, hi, off)
            assert r["first"] == lo
            assert r["set_first"].tolist() == restated_set_first(r["vst"], off), (k, "set_first")
            for j in range(len(off) - 1):
                if r["set_first"][j] != NONE:
                    res["rejected"][lo + off[j]:lo + off[j + 1]] = True
                    rej += 1
                    lost += int((r["vst"][off[j]:off[j + 1]] == 0).sum())
            seen += len(off) - 1
            assert not r["stored"][res["rejected"][lo:hi]].any(), (k, "nothing of a rejected set is stored")
            same_call(r, b.add(twin_stream(s, res["rejected"]), lo, hi), k)
            assert a.set_stats() == [seen, rej, lost]
            res["calls"].append(r)
            res["set_first"].append(r["set_first"])
        res["count"], res["flag"] = a.state()
        cb, fb = b.state()
        assert np.array_equal(res["count"], cb) and np.array_equal(res["flag"], fb), "duty state against the twin's"
        res["stats"], sb = a.stats(), b.stats()
        # (messages hashed and lookups answered depend on the shard a verify-only partial goes to)
        assert res["stats"] == sb if L.hbls_device_count() == 1 else res["stats"][:2] + res["stats"][4:] == sb[:2] + sb[4:]
        res["set_stats"] = a.set_stats()
        assert b.set_stats() == [0, 0, 0]
    finally:
        a.close()
        b.close()
    return res
