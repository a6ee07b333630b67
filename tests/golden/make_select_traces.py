"""Generate tests/golden/select_traces.json: the kernel names hbls_slot_select_device,
hbls_slot_select_batch and the duty adds (hbls_duty_add, hbls_duty_add_sets, hbls_duty_add_sets_first)
enqueue, in order, on the paths where the selection-and-aggregation tail (charon_amd/csrc/hipbls.hip,
next to ta_tail) or the steps of a duty shard's add could come apart: the device entry with shared
and with distinct messages under both group checks, with key tables, without partials; the host
entry on one shard and on two; a duty add that fires nothing and one that fires every group; a set
add that is admitted and one that is rejected, through both set entry points, on one shard and on
two (the two-phase path with the merge); a duty of threshold 1.  Everything else is
make_launch_traces.py's: its clusters (Ctx: 130 validators, n = 3, t = 2), its knobs, its recording
through hbls_timing(1) / hbls_timing_read.

The fixture pins these launch sequences across changes that must not alter them.  Record it with the
library of the commit BEFORE such a change, never from the code under test: check that commit out
into a tree of its own, build it there, copy this file beside that tree's make_launch_traces.py if
it has none, and run it from that tree with HBLS_LIBRARY naming the library built there (the
default: the tree's own) and --out naming this tree's select_traces.json.  The library's build id
goes into recorded_with.  tests/test_gpu_select_trace.py runs the same cases (CASES below) against
the tree's library.  Needs the GPU.

    python tests/golden/make_select_traces.py [--out FILE]

Every case runs on device 0 (hbls_debug_split(2): on two contexts of it), makes one warm-up call and
records the second, and restores each knob it touches.  A duty case opens a fresh duty for the
warm-up and another for the recording, and brings each to the same state, so both calls find the same
partials stored.
"""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE, os.path.join(ROOT, "tests", "gpu_helpers")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402  (the HIP runtime first: charon_amd/_lib.py)

import make_launch_traces as mk  # noqa: E402
from charon_amd import _lib  # noqa: E402

PATH = os.path.join(HERE, "select_traces.json")
V, N, T = mk.V, mk.N, mk.T
MAX_STORED = 8
BAD = V + 5  # the stream position whose signature the rejected set cases corrupt: in the second peer's set
_p = mk._p


def candidates(d):
    """Every validator's n partials in share order: (ta_src, ta_idx, grp_off), as tests/gpu_helpers/slot_select.py."""
    import slot_select
    return slot_select.all_candidates(d)


# ---- slot select ----

def select_call(cx, d, tables=False, partials=True, groups=V):
    """A hbls_slot_select_device call over the whole cluster d, one verification group per validator:
    every partial of the first `groups` validators a candidate of its validator's group."""
    L, t, NP, M = cx.L, d["t"], d["NP"], d["M"]
    src, idx, goff = candidates(d)
    src, idx, goff = src[:groups * d["n"]], idx[:groups * d["n"]], goff[:groups + 1]
    g = {k: cx.up(a) for k, a in dict(msgs=d["msgs"], moff=d["moff"].view(np.int64), mlen=d["mlen"].view(np.int32),
                                      pks=d["pks"], sigs=d["sigs"], midx=d["midx"].view(np.int32),
                                      vgoff=d["vgrp_off"].view(np.int32), src=src.view(np.int32), idx=idx,
                                      goff=goff.view(np.int32), dvpk=d["dv_pks"]).items()}
    g.update(hm=torch.zeros(M * L.hbls_hm_entry_bytes(), dtype=torch.uint8, device=cx.dev),
             vst=torch.full((NP,), 255, dtype=torch.uint8, device=cx.dev),
             tout=torch.zeros(V * 96, dtype=torch.uint8, device=cx.dev),
             tst=torch.full((V,), 255, dtype=torch.uint8, device=cx.dev),
             ast=torch.full((V,), 255, dtype=torch.uint8, device=cx.dev),
             chosen=torch.zeros(V * t, dtype=torch.int32, device=cx.dev),
             count=torch.zeros(V, dtype=torch.int32, device=cx.dev))
    s = ctypes.c_void_p(cx.stream.cuda_stream)
    if tables:
        eb = L.hbls_pk_entry_bytes()
        for name, key, cnt in (("pk", "pks", NP), ("dv", "dvpk", V)):
            g[name] = torch.zeros(cnt * eb, dtype=torch.uint8, device=cx.dev)
            g[name + "_st"] = torch.zeros(cnt, dtype=torch.uint8, device=cx.dev)
        torch.cuda.synchronize(cx.dev)
        for name, key, cnt in (("pk", "pks", NP), ("dv", "dvpk", V)):
            mk.chk(L, L.hbls_decompress_pubkeys_device(_p(g[key]), cnt, _p(g[name]), _p(g[name + "_st"]), s))
        cx.sync()
    torch.cuda.synchronize(cx.dev)
    v = {k: _p(x).value for k, x in g.items()}
    slot = _lib.HblsSlot(msgs=v["msgs"], msg_off=v["moff"], msg_len=v["mlen"], n_msgs=M, hm=v["hm"], pks=v["pks"],
                         sigs=v["sigs"], msg_idx=v["midx"], n=NP if partials else 0,
                         vgrp_off=v["vgoff"], n_vgroups=V if partials else 0, vstatus=v["vst"],
                         ta_sigs=None, ta_src=v["src"], ta_idx=v["idx"], grp_off=v["goff"], n_groups=groups,
                         n_ta_partials=len(src), ta_out=v["tout"], ta_status=v["tst"], dv_pks=v["dvpk"],
                         agg_vstatus=v["ast"], pk_table=v["pk"] if tables else None,
                         pk_table_st=v["pk_st"] if tables else None, dv_pk_table=v["dv"] if tables else None,
                         dv_pk_table_st=v["dv_st"] if tables else None)

    def call():
        mk.chk(L, L.hbls_slot_select_device(ctypes.byref(slot), t, _p(g["chosen"]), _p(g["count"]), s))
    call.keep = (g, slot)
    return call


def _select_device(name, cluster, extra=None):
    """`name`_slot_wide and `name`_per_batch: the call with hbls_slot_msm(1) and with hbls_slot_msm(0)."""
    def run(cx):
        out = {}
        for tag, msm in (("slot_wide", 1), ("per_batch", 0)):
            with mk.knobs(cx.L, fe_batch=128, slot_msm=msm):
                out[name + "_" + tag] = cx.record(select_call(cx, getattr(cx, cluster)))
        if extra:
            out.update(extra(cx))
        return out
    return run


def _lines_msg(cx):
    """Aggregates for the first 100 validators only (130 verification groups >= 128 > 100 aggregates):
    the partials' verification defers the messages' lines and the aggregates' cannot, so phase 4
    computes them first."""
    with mk.knobs(cx.L, fe_batch=128, slot_msm=0):
        return {"select_device_distinct_lines_msg": cx.record(select_call(cx, cx.distinct, groups=100))}


def select_host_call(cx):
    """hbls_slot_select_batch over the one-message-per-validator cluster: 130 groups of 3 candidates."""
    L, d = cx.L, cx.distinct
    src, idx, goff = candidates(d)
    t = d["t"]
    o = dict(vst=np.full(d["NP"], 255, np.uint8), chosen=np.zeros(V * t, np.uint32), count=np.zeros(V, np.uint32),
             out=np.zeros(96 * V, np.uint8), tst=np.full(V, 255, np.uint8), ast=np.full(V, 255, np.uint8))

    def call():
        mk.chk(L, L.hbls_slot_select_batch(_p(d["pks"]), _p(d["sigs"]), _p(d["item_msgs"]), _p(d["item_off"]),
                                           _p(d["item_len"]), d["NP"], _p(src), _p(idx), _p(goff), V, _p(d["dv_pks"]), t,
                                           *(_p(o[k]) for k in ("vst", "chosen", "count", "out", "tst", "ast"))))
        assert not o["vst"].any() and not o["tst"].any() and not o["ast"].any()
    call.keep = (src, idx, goff, o)
    return call


class split2:
    """hbls_debug_split(2): two contexts of device 0, each a shard of the host calls."""

    def __init__(self, L):
        self.L = L

    def __enter__(self):
        mk.chk(self.L, self.L.hbls_debug_split(2))

    def __exit__(self, *exc):
        mk.chk(self.L, self.L.hbls_debug_split(1))


def _select_host(split):
    def run(cx):
        L = cx.L
        with mk.knobs(L, fe_batch=128, slot_msm=0):
            mk.chk(L, L.hbls_pubkey_cache_clear())
            if not split:
                return {"select_host": cx.record(select_host_call(cx))}
            with split2(L):
                return {"select_host_split2": cx.record(select_host_call(cx))}
    return run


# ---- duties ----

def duty_stream(cx):
    """The shared-message cluster as a duty's stream (tests/gpu_helpers/duty.py): peer-major, so
    partials [k V, (k + 1) V) are peer k's set, one partial per group."""
    if not hasattr(cx, "_duty_stream"):
        import duty
        d = cx.shared
        src, idx, goff = candidates(d)
        c = dict(pks=d["pks"].reshape(-1, 48), sigs=d["sigs"].reshape(-1, 96), msgs=d["msgs"].reshape(-1, 32)[d["midx"]],
                 src=src, idx=idx, goff=goff, dv=d["dv_pks"].reshape(-1, 48), t=d["t"])
        cx._duty_stream = duty.stream_of(c)
        assert (cx._duty_stream["group"][:2 * V] == np.tile(np.arange(V), 2)).all()
    return cx._duty_stream


def duty_record(cx, t, before, call):
    """The launches of call(duty) on a fresh duty of threshold t that before(duty) prepared: once as
    the warm-up, once recorded, each on a duty of its own."""
    import duty_first
    s = duty_stream(cx)
    names = None
    for recorded in (False, True):
        du = duty_first.FirstDuty(cx.L, s["dv"], t, MAX_STORED)
        try:
            before(du, s)
            if recorded:
                names = cx.record_next(lambda: call(du, s))
            else:
                call(du, s)
        finally:
            du.close()
    return names


def _nothing(du, s):
    pass


def _first_peer(du, s):
    assert len(du.add(s, 0, V)["fired"]) == 0


def _fires(r):
    assert len(r["fired"]) == V and not r["tst"].any() and not r["ast"].any()


def _fires_alone(du, s):
    """threshold 1: every group fires on its first partial, which is its own aggregate (and so no
    signature under the validator's key of a cluster split 2 of 3)"""
    r = du.add(s, 0, V)
    assert len(r["fired"]) == V and not r["tst"].any() and r["ast"].all()


def _second_peer_set(entry, bad):
    """The second peer's partials as one set through SetsDuty.add_sets / FirstDuty.add_sets_first;
    bad: one of them carries its neighbour's signature, so the set is rejected and nothing fires."""
    def call(du, s):
        import duty_first
        r = getattr(du, entry)(duty_first.spoiled(s, [BAD]) if bad else s, V, 2 * V, [0, V])
        if bad:
            assert r["set_first"].tolist() == [BAD - V] and not r["stored"].any() and len(r["fired"]) == 0
        else:
            assert r["set_first"].tolist() == [0xFFFFFFFF]
            _fires(r)
    return call


HOST = dict(fe_batch=128, slot_msm=0)


def _duty(name, t, before, call):
    def run(cx):
        with mk.knobs(cx.L, **HOST):
            mk.chk(cx.L, cx.L.hbls_pubkey_cache_clear())
            return {name: duty_record(cx, t, before, call)}
    return run


def _duty_sets(name, entry, split=False):
    """`name`_clean and `name`_rejected on a duty that holds the first peer's partials."""
    def run(cx):
        L = cx.L
        with mk.knobs(L, **HOST):
            mk.chk(L, L.hbls_pubkey_cache_clear())
            if split:
                with split2(L):  # the duty is opened over the two shards
                    return {name + "_" + tag: duty_record(cx, T, _first_peer, _second_peer_set(entry, bad))
                            for tag, bad in (("clean", False), ("rejected", True))}
            return {name + "_" + tag: duty_record(cx, T, _first_peer, _second_peer_set(entry, bad))
                    for tag, bad in (("clean", False), ("rejected", True))}
    return run


# ---- the cases: name -> function(cx) returning {trace name: [kernel names]} ----
CASES = {
    "select_device_shared": _select_device("select_device_shared", "shared"),
    "select_device_distinct": _select_device("select_device_distinct", "distinct", extra=_lines_msg),
    "select_device_tables": mk._one("select_device_tables", lambda cx: select_call(cx, cx.shared, tables=True),
                                    fe_batch=128, slot_msm=1),
    "select_device_no_partials": mk._one("select_device_no_partials", lambda cx: select_call(cx, cx.shared, partials=False),
                                         fe_batch=128, slot_msm=1),
    "select_host": _select_host(False),
    "select_host_split2": _select_host(True),
    "duty_add_no_fire": _duty("duty_add_no_fire", T, _nothing, _first_peer),
    "duty_add_fires": _duty("duty_add_fires", T, _first_peer, lambda du, s: _fires(du.add(s, V, 2 * V))),
    "duty_add_sets": _duty_sets("duty_add_sets", "add_sets"),
    "duty_add_sets_first": _duty_sets("duty_add_sets_first", "add_sets_first"),
    "duty_add_sets_split2": _duty_sets("duty_add_sets_split2", "add_sets", split=True),
    "duty_add_sets_first_split2": _duty_sets("duty_add_sets_first_split2", "add_sets_first", split=True),
    "duty_t1": _duty("duty_t1", 1, _nothing, _fires_alone),
}
# the traces each case records
TRACES = {
    "select_device_shared": ["select_device_shared_slot_wide", "select_device_shared_per_batch"],
    "select_device_distinct": ["select_device_distinct_slot_wide", "select_device_distinct_per_batch",
                               "select_device_distinct_lines_msg"],
    **{c: [c + "_clean", c + "_rejected"] for c in ("duty_add_sets", "duty_add_sets_first", "duty_add_sets_split2",
                                                     "duty_add_sets_first_split2")},
}


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    out = argv[argv.index("--out") + 1] if "--out" in argv else PATH
    L = _lib.lib()
    cx = mk.Ctx(L)
    traces = {}
    for name, run in CASES.items():
        got = run(cx)
        assert sorted(got) == sorted(TRACES.get(name, [name])), name
        traces.update(got)
    with open(out, "w") as f:
        json.dump({"recorded_with": L.hbls_build_id().decode(), "traces": traces}, f, indent=1)
    print("wrote", out, {k: len(v) for k, v in traces.items()})


if __name__ == "__main__":
    main()
