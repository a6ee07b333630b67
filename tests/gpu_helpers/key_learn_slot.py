"""Shared by tests/test_gpu_key_learn.py and its child process: a small synthetic cluster run
through hbls_slot_device (the benchmarked entry point), with the key arrays replaceable, several
slots enqueued with or without a synchronisation between them, and the learned key cache's
counters.  Run as a script it is the child of the environment test: HBLS_KEY_LEARN comes from the
environment, the slot runs three times, and one JSON line reports the outputs' digests and the
counters."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (the HIP runtime first: charon_amd/_lib.py)

from charon_amd import _lib  # noqa: E402

# 24 validators of a 4-operator threshold-3 cluster: 96 pubshares (one full wave and a partial
# one) + 24 DV keys (a partial wave)
WL = dict(validators=24, n=4, t=3, distinct=False, n_msgs=4)


def _p(x):
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        return ctypes.c_void_p(x.ctypes.data)
    return ctypes.c_void_p(x.data_ptr())


def chk(L, rc):
    assert rc == 0, L.hbls_last_error().decode()


def tune(L, name, value):
    prev = ctypes.c_size_t(0)
    chk(L, L.hbls_tune(name.encode(), value, ctypes.byref(prev)))
    return prev.value


def stats(L):
    """Device 0's {size, capacity, hits, misses}."""
    return _lib.key_learn_stats(L)[0]


def make_inputs(L, wl=None):
    import bench
    wl = wl or WL
    return bench.setup_inputs(L, wl, wl["validators"], 0)


def fresh_keys(L, count, seed):
    """count valid public keys (count x 48 uint8) of secrets derived from the seed."""
    sks = np.frombuffer(b"".join(hashlib.sha256(b"key learn %d %d" % (seed, k)).digest() for k in range(count)),
                        dtype=np.uint8).reshape(count, 32).copy()
    sks[:, 0] &= 0x3F  # < 2^254 < r
    sks[:, 31] |= 1
    pks = np.zeros(48 * count, dtype=np.uint8)
    st = np.zeros(count, dtype=np.uint8)
    chk(L, L.hbls_secret_to_public_key_batch(_p(sks.reshape(-1)), count, _p(pks), _p(st)))
    assert not st.any()
    return pks.reshape(count, 48)


def run_slots(L, d, pks=None, dv_pks=None, calls=1, sync_between=True, tables=False):
    """`calls` hbls_slot_device calls on the cluster d with the given key arrays (default: the
    cluster's own), each on a stream and an output set of its own; sync_between False: all of them
    enqueued before anything is waited for.  tables: the keys come as decompressed tables
    (pk_table / dv_pk_table).  Returns one (vstatus, ta_status, agg_status, aggregates) of bytes
    per call."""
    dev = torch.device("cuda", 0)
    n, t, V, NP, M = d["n"], d["t"], d["V"], d["NP"], d["M"]
    pks = d["pks"] if pks is None else np.ascontiguousarray(pks).reshape(-1)
    dv_pks = d["dv_pks"] if dv_pks is None else np.ascontiguousarray(dv_pks).reshape(-1)
    assert pks.size == 48 * NP and dv_pks.size == 48 * V

    def up(a):
        return torch.from_numpy(a).to(dev)

    g = {k: up(a) for k, a in dict(msgs=d["msgs"], moff=d["moff"].view(np.int64), mlen=d["mlen"].view(np.int32),
                                   pks=pks, sigs=d["sigs"], midx=d["midx"].view(np.int32),
                                   vgoff=d["vgrp_off"].view(np.int32), tsrc=d["ta_src"].view(np.int32),
                                   tidx=d["ta_idx"], goff=d["grp_off"].view(np.int32), dvpk=dv_pks).items()}
    tab = {}
    if tables:
        eb = L.hbls_pk_entry_bytes()
        s0 = torch.cuda.Stream(device=dev)
        for name, src, cnt in (("pk", g["pks"], NP), ("dv", g["dvpk"], V)):
            tab[name] = torch.zeros(cnt * eb, dtype=torch.uint8, device=dev)
            tab[name + "_st"] = torch.zeros(cnt, dtype=torch.uint8, device=dev)
            chk(L, L.hbls_decompress_pubkeys_device(_p(src), cnt, _p(tab[name]), _p(tab[name + "_st"]),
                                                    ctypes.c_void_p(s0.cuda_stream)))
        s0.synchronize()
    outs = []
    for _ in range(calls):
        o = dict(hm=torch.zeros(M * L.hbls_hm_entry_bytes(), dtype=torch.uint8, device=dev),
                 vst=torch.full((NP,), 255, dtype=torch.uint8, device=dev),
                 tout=torch.zeros(V * 96, dtype=torch.uint8, device=dev),
                 tst=torch.full((V,), 255, dtype=torch.uint8, device=dev),
                 ast=torch.full((V,), 255, dtype=torch.uint8, device=dev),
                 stream=torch.cuda.Stream(device=dev))
        outs.append(o)
    torch.cuda.synchronize(dev)  # the uploads and fills, before the slots' own streams read them
    for o in outs:
        slot = _lib.HblsSlot(msgs=_p(g["msgs"]).value, msg_off=_p(g["moff"]).value, msg_len=_p(g["mlen"]).value,
                             n_msgs=M, hm=_p(o["hm"]).value, pks=_p(g["pks"]).value, sigs=_p(g["sigs"]).value,
                             msg_idx=_p(g["midx"]).value, n=NP, vgrp_off=_p(g["vgoff"]).value, n_vgroups=V,
                             vstatus=_p(o["vst"]).value, ta_sigs=None, ta_src=_p(g["tsrc"]).value,
                             ta_idx=_p(g["tidx"]).value, grp_off=_p(g["goff"]).value, n_groups=V,
                             n_ta_partials=V * t, ta_out=_p(o["tout"]).value, ta_status=_p(o["tst"]).value,
                             dv_pks=_p(g["dvpk"]).value, agg_vstatus=_p(o["ast"]).value,
                             pk_table=_p(tab["pk"]).value if tables else None,
                             pk_table_st=_p(tab["pk_st"]).value if tables else None,
                             dv_pk_table=_p(tab["dv"]).value if tables else None,
                             dv_pk_table_st=_p(tab["dv_st"]).value if tables else None)
        chk(L, L.hbls_slot_device(ctypes.byref(slot), ctypes.c_void_p(o["stream"].cuda_stream)))
        if sync_between:
            o["stream"].synchronize()
    for o in outs:
        o["stream"].synchronize()
    return [tuple(o[k].cpu().numpy().tobytes() for k in ("vst", "tst", "ast", "tout")) for o in outs]


def digest(out):
    h = hashlib.sha256()
    for part in out:
        h.update(part)
    return h.hexdigest()


def main():
    L = _lib.lib()
    d = make_inputs(L)
    outs = run_slots(L, d, calls=3)
    print(json.dumps({"env": os.environ.get("HBLS_KEY_LEARN"), "digests": [digest(o) for o in outs],
                      "vstatus_all_ok": all(not any(o[0]) for o in outs), "stats": stats(L)}))


if __name__ == "__main__":
    main()
