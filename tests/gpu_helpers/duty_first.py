"""First-error duty set adds (hbls_duty_add_sets_first / hbls_duty_first_stats) beside hbls_duty_add_sets
on the same stream, for tests/test_gpu_duty_first.py.  Streams, sentinels and the calls' plumbing are
tests/gpu_helpers/duty.py's and duty_sets.py's: the new call has hbls_duty_add_sets' signature, so
SetsDuty.add_sets drives it through a library handle that answers that one name with the new entry point.
"""
import numpy as np

from duty import NONE, _p
from duty_sets import SetsDuty, same_call

OK, BAD_PUBKEY, BAD_SIGNATURE, NOT_VERIFIED, UNCHECKED = 0, 1, 2, 3, 7
ROWS = ("first", "stored", "fired", "chosen", "out", "tst", "ast")  # what the twin's call gives exactly (vst: the contract)


class _FirstEntry:
    def __init__(self, L):
        self._L = L

    def __getattr__(self, name):
        return getattr(self._L, "hbls_duty_add_sets_first" if name == "hbls_duty_add_sets" else name)


class FirstDuty(SetsDuty):
    def add_sets_first(self, *a, **kw):
        """SetsDuty.add_sets' arguments and result, through hbls_duty_add_sets_first"""
        real, self.L = self.L, _FirstEntry(self.L)
        try:
            return self.add_sets(*a, **kw)
        finally:
            self.L = real

    def first_stats(self):
        out = np.full(2 + 2, 0xA5A5A5A5A5A5A5A5, np.uint64)
        assert self.L.hbls_duty_first_stats(self.h, _p(out), 2) == 0, self.L.hbls_last_error().decode()
        assert (out[2:] == 0xA5A5A5A5A5A5A5A5).all()
        return [int(x) for x in out[:2]]


def spoiled(s, at):
    """the stream with each partial of `at` carrying a neighbour's signature: a point of G2 that verifies
    nothing here (the neighbour is another validator's partial, over another message)"""
    sigs = s["sigs"].copy()
    for i in at:
        sigs[i] = s["sigs"][i + 1 if i + 1 < len(sigs) else i - 1]
    return dict(s, sigs=sigs)


def undecodable(s, at):
    """... carrying 96 bytes that are no compressed point (the infinity flag with a nonzero body)"""
    sigs = s["sigs"].copy()
    for i in at:
        sigs[i] = 0xC1
    return dict(s, sigs=sigs)


def check_contract(r, w, off, what=""):
    """include/hipbls.h's vstatus contract of one call `r` against the twin's exact call `w` over the sets `off`"""
    assert np.array_equal(r["set_first"], w["set_first"]), (what, "set_first", r["set_first"], w["set_first"])
    for k in ROWS:
        assert np.array_equal(r[k], w[k]), (what, k)
    got, exact = r["vst"], w["vst"]
    assert set(np.unique(got).tolist()) <= set(np.unique(exact).tolist()) | {UNCHECKED}
    dec = (exact == BAD_PUBKEY) | (exact == BAD_SIGNATURE)
    assert np.array_equal(got[dec], exact[dec]), (what, "decoding failures stay exact everywhere")
    for j in range(len(off) - 1):
        b, e, f = off[j], off[j + 1], int(r["set_first"][j])
        if f == NONE:
            assert (got[b:e] == OK).all() and (exact[b:e] == OK).all(), (what, j, "an admitted set holds only OK")
            continue
        assert b <= f < e and got[f] == exact[f] != OK, (what, j, "the first failure carries its exact status")
        assert (got[b:f] == OK).all(), (what, j, "every partial before it is OK")
        rest = np.arange(f + 1, e)
        assert ((got[rest] == exact[rest]) | (got[rest] == UNCHECKED)).all(), (what, j, "exact or UNCHECKED, nothing else")
    return int((got == UNCHECKED).sum())


def run_first_pair(L, s, bounds, sets_of_call, max_stored=16, modes=None, exact=False):
    """The stream through a duty driven by hbls_duty_add_sets_first (call k = partials [bounds[k],
    bounds[k + 1]) in the sets sets_of_call[k], offsets relative to the call) and through its twin driven
    by hbls_duty_add_sets, compared call by call under the defining property and the vstatus contract, and
    in their final state and statistics.  modes[k]: "first" (the default), "sets" or "add" for the first
    duty's call k; the twin takes "add" calls as they are.  exact: every status must equal the twin's.
    -> dict(calls, twin, unchecked, first_stats, set_stats, count, flag)"""
    a, b = FirstDuty(L, s["dv"], s["t"], max_stored), FirstDuty(L, s["dv"], s["t"], max_stored)
    res = dict(calls=[], twin=[], unchecked=0)
    through = 0
    try:
        for k in range(len(bounds) - 1):
            lo, hi, off = bounds[k], bounds[k + 1], list(sets_of_call[k])
            mode = modes[k] if modes else "first"
            if mode == "add":
                r, w = a.add(s, lo, hi), b.add(s, lo, hi)
                same_call(r, w, k)
            else:
                r = a.add_sets_first(s, lo, hi, off) if mode == "first" else a.add_sets(s, lo, hi, off)
                w = b.add_sets(s, lo, hi, off)
                if mode == "first":
                    u = check_contract(r, w, off, k)
                    assert not (exact and u), (k, "below the batched final exponentiation every status is exact")
                    res["unchecked"] += u
                    through += hi - lo
                else:
                    same_call(r, w, k)
                    assert np.array_equal(r["set_first"], w["set_first"])
            assert a.first_stats() == [through, res["unchecked"]] and b.first_stats() == [0, 0]
            res["calls"].append(r)
            res["twin"].append(w)
        res["count"], res["flag"] = a.state()
        cb, fb = b.state()
        assert np.array_equal(res["count"], cb) and np.array_equal(res["flag"], fb), "hbls_duty_state against the twin's"
        assert a.stats() == b.stats(), "hbls_duty_stats against the twin's"
        sa, sb = a.set_stats(), b.set_stats()
        assert sa[:2] == sb[:2] and sb[2] - res["unchecked"] <= sa[2] <= sb[2], (sa, sb)  # out[2]: those *reported* OK
        res["set_stats"], res["first_stats"] = sa, a.first_stats()
    finally:
        a.close()
        b.close()
    return res
