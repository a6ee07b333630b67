"""Generate tests/golden/launch_traces.json: the kernel names a verification enqueues, in order, for
every path verify_pipeline (charon_amd/csrc/hipbls.hip) can take -- the three group checks, both
combinations, several chunks of groups, the adaptive skip, the first-error mode, the variants of
hbls_slot_device and the host paths (the whole-call form, the per-device shards under
hbls_debug_split, the first-error form and, with --large, the chunks of a 2^19-item call).
hbls_timing(1) / hbls_timing_read give the names of a call
in enqueue order; the sequence depends on the shapes and the knob settings only (data decides
nothing on the host: the device guards do), the adaptive history excepted, which its case drives
itself.

The fixture pins the launch sequence across changes that must not alter it.  Record it with the
library of the commit BEFORE such a change (HBLS_LIBRARY names it, run from that commit's tree),
never from the code under test; tests/test_gpu_launch_trace.py runs the same cases (CASES below)
against the tree's library.  Needs the GPU.

    python tests/golden/make_launch_traces.py [--out FILE] [--large]

--large also records LARGE_TRACES (a 530 000-item call: a minute of signing first); without it the
file's recorded ones are kept.

Every case runs on device 0, makes one warm-up call and records the second (the first call
allocates the learned-key table and grows buffers), and restores each knob it touches.
"""
import contextlib
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402  (the HIP runtime first: charon_amd/_lib.py)

from charon_amd import _lib  # noqa: E402

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "launch_traces.json")
V, N, T = 130, 3, 2  # 130 validators (two full batches of 64 groups and a ragged one of 2), 3 partials each


def _p(x):
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        return ctypes.c_void_p(x.ctypes.data)
    return ctypes.c_void_p(x.data_ptr())


def chk(L, rc):
    assert rc == 0, L.hbls_last_error().decode()


@contextlib.contextmanager
def knobs(L, fe_batch=None, slot_msm=None, adaptive=None, rlc_lanes=None, group_chunk=None):
    """Set the given knobs, restore them afterwards (hbls_slot_msm also clears the adaptive history)."""
    undo = []
    try:
        for fn, v in ((L.hbls_fe_batch, fe_batch), (L.hbls_slot_msm, slot_msm), (L.hbls_adaptive, adaptive),
                      (L.hbls_rlc_lanes, rlc_lanes)):
            if v is not None:
                undo.append((fn, fn(v)))
        if group_chunk is not None:
            prev = ctypes.c_size_t(0)
            chk(L, L.hbls_tune(b"HBLS_GROUP_CHUNK", group_chunk, ctypes.byref(prev)))
            undo.append((lambda v: chk(L, L.hbls_tune(b"HBLS_GROUP_CHUNK", v, None)), prev.value))
        yield
    finally:
        for fn, v in reversed(undo):
            fn(v)


class Ctx:
    """The two clusters (shared messages; one message per validator), on device 0."""

    def __init__(self, L):
        import bench
        self.L = L
        self.dev = torch.device("cuda", 0)
        self.stream = torch.cuda.Stream(device=self.dev)
        self.shared = bench.setup_inputs(L, dict(validators=V, n=N, t=T, distinct=False, n_msgs=4), V, 0)
        self.distinct = bench.setup_inputs(L, dict(validators=V, n=N, t=T, distinct=True, n_msgs=0), V, 0)
        assert self.distinct["M"] == V
        self._hm = {}

    def up(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def sync(self):
        chk(self.L, self.L.hbls_sync(ctypes.c_void_p(self.stream.cuda_stream)))

    def hm(self, d):
        """d's messages hashed with their lines (device), once."""
        if id(d) not in self._hm:
            L = self.L
            hm = torch.zeros(d["M"] * L.hbls_hm_entry_bytes(), dtype=torch.uint8, device=self.dev)
            g = [self.up(d["msgs"]), self.up(d["moff"].view(np.int64)), self.up(d["mlen"].view(np.int32))]
            torch.cuda.synchronize(self.dev)
            chk(L, L.hbls_hash_to_g2_device(_p(g[0]), _p(g[1]), _p(g[2]), d["M"], _p(hm),
                                            ctypes.c_void_p(self.stream.cuda_stream)))
            self.sync()
            self._hm[id(d)] = hm
        return self._hm[id(d)]

    def record(self, call):
        """The names of call()'s launches: one warm-up call, the second recorded."""
        call()
        self.sync()
        return self.record_next(call)

    def record_next(self, call):
        L = self.L
        chk(L, L.hbls_timing(1))
        try:
            call()
            self.sync()
            return [name for name, _ in _lib.timing_read(L)]
        finally:
            chk(L, L.hbls_timing(0))


def grouped_items(d, sizes):
    """The first sizes[v] partials of validator v, one verification group each: (item indices, offsets)."""
    items = [v * d["n"] + k for v, s in enumerate(sizes) for k in range(s)]
    return np.asarray(items), np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)


MIXED = [1 + v % 3 for v in range(V)]  # 130 groups of 1, 2, 3 items: 259 items


def device_call(cx, sizes, grouped=True, first_error=False, swap=None):
    """A hbls_verify_device (or first-error) call over the shared-message cluster's groups; swap
    (i, j): item i carries item j's signature (decodable, wrong: only a pairing catches it)."""
    L, d = cx.L, cx.shared
    items, goff = grouped_items(d, sizes)
    sigs = d["sigs"].reshape(-1, 96)[items].copy()
    if swap:
        sigs[swap[0]] = sigs[swap[1]]
    n = len(items)
    g = dict(pks=cx.up(d["pks"].reshape(-1, 48)[items].reshape(-1)), sigs=cx.up(sigs.reshape(-1)),
             midx=cx.up(d["midx"][items].astype(np.uint32).view(np.int32)), goff=cx.up(goff.view(np.int32)),
             st=torch.full((n,), 255, dtype=torch.uint8, device=cx.dev),
             first=torch.zeros(1, dtype=torch.int32, device=cx.dev))
    hm = cx.hm(d)
    torch.cuda.synchronize(cx.dev)
    s = ctypes.c_void_p(cx.stream.cuda_stream)
    goff_p, ng = (_p(g["goff"]), len(sizes)) if grouped else (None, 0)

    def call():
        if first_error:
            chk(L, L.hbls_verify_device_first_error(_p(g["pks"]), _p(g["sigs"]), _p(g["midx"]), _p(hm), n, goff_p, ng,
                                                    _p(g["st"]), _p(g["first"]), s))
        else:
            chk(L, L.hbls_verify_device(_p(g["pks"]), _p(g["sigs"]), _p(g["midx"]), _p(hm), n, goff_p, ng,
                                        _p(g["st"]), s))
    call.keep = g
    return call


def slot_call(cx, d, dv=True, src=True, tables=False):
    """A hbls_slot_device call over the whole cluster d (one verification group per validator)."""
    L, t, NP, M = cx.L, d["t"], d["NP"], d["M"]
    g = {k: cx.up(a) for k, a in dict(msgs=d["msgs"], moff=d["moff"].view(np.int64), mlen=d["mlen"].view(np.int32),
                                      pks=d["pks"], sigs=d["sigs"], midx=d["midx"].view(np.int32),
                                      vgoff=d["vgrp_off"].view(np.int32), tsrc=d["ta_src"].view(np.int32),
                                      tsig=d["ta_sigs"], tidx=d["ta_idx"], goff=d["grp_off"].view(np.int32),
                                      dvpk=d["dv_pks"]).items()}
    g.update(hm=torch.zeros(M * L.hbls_hm_entry_bytes(), dtype=torch.uint8, device=cx.dev),
             vst=torch.full((NP,), 255, dtype=torch.uint8, device=cx.dev),
             tout=torch.zeros(V * 96, dtype=torch.uint8, device=cx.dev),
             tst=torch.full((V,), 255, dtype=torch.uint8, device=cx.dev),
             ast=torch.full((V,), 255, dtype=torch.uint8, device=cx.dev))
    s = ctypes.c_void_p(cx.stream.cuda_stream)
    if tables:
        eb = L.hbls_pk_entry_bytes()
        for name, key, cnt in (("pk", "pks", NP), ("dv", "dvpk", V)):
            g[name] = torch.zeros(cnt * eb, dtype=torch.uint8, device=cx.dev)
            g[name + "_st"] = torch.zeros(cnt, dtype=torch.uint8, device=cx.dev)
        torch.cuda.synchronize(cx.dev)
        for name, key, cnt in (("pk", "pks", NP), ("dv", "dvpk", V)):
            chk(L, L.hbls_decompress_pubkeys_device(_p(g[key]), cnt, _p(g[name]), _p(g[name + "_st"]), s))
        cx.sync()
    torch.cuda.synchronize(cx.dev)
    v = {k: _p(x).value for k, x in g.items()}
    slot = _lib.HblsSlot(msgs=v["msgs"], msg_off=v["moff"], msg_len=v["mlen"], n_msgs=M, hm=v["hm"], pks=v["pks"],
                         sigs=v["sigs"], msg_idx=v["midx"], n=NP, vgrp_off=v["vgoff"], n_vgroups=V, vstatus=v["vst"],
                         ta_sigs=None if src else v["tsig"], ta_src=v["tsrc"] if src else None, ta_idx=v["tidx"],
                         grp_off=v["goff"], n_groups=V, n_ta_partials=V * t, ta_out=v["tout"], ta_status=v["tst"],
                         dv_pks=v["dvpk"] if dv else None, agg_vstatus=v["ast"] if dv else None,
                         pk_table=v["pk"] if tables else None, pk_table_st=v["pk_st"] if tables else None,
                         dv_pk_table=v["dv"] if tables else None, dv_pk_table_st=v["dv_st"] if tables else None)

    def call():
        chk(L, L.hbls_slot_device(ctypes.byref(slot), s))
    call.keep = (g, slot)
    return call


def host_call(cx):
    """hbls_verify_batch over the one-message-per-validator cluster: 130 groups of 3 items."""
    L, d = cx.L, cx.distinct
    st = np.full(d["NP"], 255, dtype=np.uint8)

    def call():
        chk(L, L.hbls_verify_batch(_p(d["pks"]), _p(d["sigs"]), _p(d["item_msgs"]), _p(d["item_off"]),
                                   _p(d["item_len"]), d["NP"], _p(st)))
        assert not st.any()
    return call


# ---- the cases: name -> function(cx) returning {trace name: [kernel names]} ----

def _one(name, make, **kn):
    def run(cx):
        with knobs(cx.L, **kn):
            return {name: cx.record(make(cx))}
    return run


def _adaptive(cx):
    """A clean history, then: a call with one wrong signature (the slot-wide check runs and fails),
    the same call again (skipped: straight to the per-batch check, which fails a batch again), a
    clean call (still skipped; its outcome clears the history).  hbls_sync after each."""
    with knobs(cx.L, fe_batch=128, slot_msm=1, adaptive=1):
        bad, clean = device_call(cx, MIXED, swap=(7, 100)), device_call(cx, MIXED)
        clean()  # warm-up
        cx.sync()
        cx.L.hbls_slot_msm(1)  # a clean history
        return {"adaptive_1_failed": cx.record_next(bad), "adaptive_2_skipped": cx.record_next(bad),
                "adaptive_3_skipped_clean": cx.record_next(clean)}


def host_first_error_call(cx):
    """hbls_verify_batch_first_error over the same cluster: 130 runs of 3 items in the caller's order."""
    L, d = cx.L, cx.distinct
    st = np.full(d["NP"], 255, dtype=np.uint8)
    first, fst = ctypes.c_int64(0), ctypes.c_uint8(255)

    def call():
        chk(L, L.hbls_verify_batch_first_error(_p(d["pks"]), _p(d["sigs"]), _p(d["item_msgs"]), _p(d["item_off"]),
                                               _p(d["item_len"]), d["NP"], ctypes.byref(first), ctypes.byref(fst),
                                               _p(st)))
        assert first.value == -1 and fst.value == 0 and not st.any()
    return call


def _host(cx):
    L, d = cx.L, cx.distinct
    with knobs(L, fe_batch=128, slot_msm=0):
        chk(L, L.hbls_pubkey_cache_clear())
        out = {"host_no_key_cache": cx.record(host_call(cx)),
               "host_first_error": cx.record(host_first_error_call(cx))}
        # the per-device shards: two contexts of device 0, 65 groups each, every context's launches
        # in its own enqueue order (hbls_timing_read lists context after context)
        chk(L, L.hbls_debug_split(2))
        try:
            out["host_split2"] = cx.record(host_call(cx))
        finally:
            chk(L, L.hbls_debug_split(1))
        chk(L, L.hbls_pubkey_cache_add(_p(d["pks"]), d["NP"]))
        try:
            out["host_key_cache"] = cx.record(host_call(cx))
        finally:
            chk(L, L.hbls_pubkey_cache_clear())
        return out


BATCHED = dict(fe_batch=128, slot_msm=0)
SLOT_WIDE = dict(fe_batch=128, slot_msm=1, adaptive=0)
CASES = {
    "small_groups": _one("small_groups", lambda cx: device_call(cx, [1, 2, 2]), fe_batch=0),
    "small_ungrouped": _one("small_ungrouped", lambda cx: device_call(cx, [1, 1, 1], grouped=False), fe_batch=0),
    "per_batch": _one("per_batch", lambda cx: device_call(cx, MIXED), **BATCHED),
    "per_batch_two_chunks": _one("per_batch_two_chunks", lambda cx: device_call(cx, MIXED), group_chunk=100, **BATCHED),
    "slot_wide_per_item": _one("slot_wide_per_item", lambda cx: device_call(cx, MIXED), **SLOT_WIDE),
    "slot_wide_chunked": _one("slot_wide_chunked", lambda cx: device_call(cx, MIXED), rlc_lanes=64, **SLOT_WIDE),
    "slot_wide_two_chunks": _one("slot_wide_two_chunks", lambda cx: device_call(cx, MIXED), group_chunk=100, **SLOT_WIDE),
    "adaptive": _adaptive,
    "first_error_batched": _one("first_error_batched", lambda cx: device_call(cx, MIXED, first_error=True), **BATCHED),
    "first_error_small": _one("first_error_small", lambda cx: device_call(cx, [1, 2, 2], first_error=True), **BATCHED),
    "slot_dv_src": _one("slot_dv_src", lambda cx: slot_call(cx, cx.shared), fe_batch=128, slot_msm=1),
    "slot_ta_sigs": _one("slot_ta_sigs", lambda cx: slot_call(cx, cx.shared, src=False), fe_batch=128, slot_msm=1),
    "slot_no_dv": _one("slot_no_dv", lambda cx: slot_call(cx, cx.shared, dv=False), fe_batch=128, slot_msm=1),
    "slot_tables": _one("slot_tables", lambda cx: slot_call(cx, cx.shared, tables=True), fe_batch=128, slot_msm=1),
    "slot_deferred_slot_wide": _one("slot_deferred_slot_wide", lambda cx: slot_call(cx, cx.distinct),
                                    fe_batch=128, slot_msm=1),
    "slot_deferred_per_batch": _one("slot_deferred_per_batch", lambda cx: slot_call(cx, cx.distinct), **BATCHED),
    "host": _host,
}


LARGE_TRACES = {"verify_large_deferred": None, "verify_large_chunk_lines": 40_000}  # name -> hbls_fe_batch


def large_traces(L, d):
    """The launches of hbls_verify_batch over d, bench.setup_inputs' 53 000 x 10 cluster with one
    message per validator (tests/test_gpu_robustness.py `large`): 2^19 items and more, so verify_large
    runs it as two chunks on two host-call contexts of device 0, in chunk order.  With the default
    knobs every chunk defers its messages' lines (no k_lines_msg); with hbls_fe_batch(40 000) the
    call defers and each chunk of ~26 500 groups does not, so computes them."""
    cx = Ctx.__new__(Ctx)
    cx.L, cx.dev = L, torch.device("cuda", 0)
    cx.stream = torch.cuda.Stream(device=cx.dev)
    st = np.full(d["NP"], 255, dtype=np.uint8)

    def call():
        chk(L, L.hbls_verify_batch(_p(d["pks"]), _p(d["sigs"]), _p(d["item_msgs"]), _p(d["item_off"]),
                                   _p(d["item_len"]), d["NP"], _p(st)))
        assert not st.any()
    out = {}
    for name, fe in LARGE_TRACES.items():
        L.hbls_slot_msm(L.hbls_slot_msm(0))  # the same value again: a clean adaptive history
        with knobs(L, fe_batch=fe):
            out[name] = cx.record(call)
    return out


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    out = argv[argv.index("--out") + 1] if "--out" in argv else PATH
    L = _lib.lib()
    cx = Ctx(L)
    traces = {}
    for name, run in CASES.items():
        traces.update(run(cx))
    if "--large" in argv:
        import bench
        wl = dict(validators=53_000, n=10, t=7, distinct=True, n_msgs=0)
        large = large_traces(L, bench.setup_inputs(L, wl, wl["validators"], 0))
    else:
        with open(PATH) as f:
            large = json.load(f)["traces_large"]
    with open(out, "w") as f:
        json.dump({"recorded_with": L.hbls_build_id().decode(), "traces": traces, "traces_large": large}, f, indent=1)
    print("wrote", out, {k: len(v) for k, v in {**traces, **large}.items()})


if __name__ == "__main__":
    main()
