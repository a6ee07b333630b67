"""hbls_slot_select_device against what a caller has to do without it, on one GPU in one run.

    python tools/slot_select_bench.py [--out profiles/slot_select_bench.json] [--rounds 3]

Per configuration (the C5 shard, 125 k validators 5 of 7, clean and at 1 % and 10 % corrupted
partials; C3, 100 k validators 7 of 10, at 10 %; bench.corrupt's mix) three legs, alternating, medians reported:
  a  hbls_slot_select_device
  b  today's repair outside the library: hbls_hash_to_g2_device, hbls_verify_device, the statuses to
     the host, the members picked with numpy, uploaded, hbls_threshold_aggregate_device on their
     bytes (decompressed a second time), hbls_verify_device over the aggregates
  c  hbls_slot_device with the fixed members on the same bytes (context: it returns fewer aggregates)
Per leg: ms per slot (wall clock from the first call to the last result on the device, host steps
included) and the validators that end with a verified aggregate; for (a) also the share of
groups the small-scalar path aggregated (hbls_slot_select_stats).  bench.py is unchanged and its C5
headline still measures the fixed-member slot.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = [("c5_clean", "c5", 0.0), ("c5_1pct", "c5", 0.01), ("c5_10pct", "c5", 0.10), ("c3_10pct", "c3", 0.10)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slot_select_bench.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--validators", type=int, default=0, help="override the shard size (smoke runs)")
    ap.add_argument("--configs", default=",".join(c[0] for c in CONFIGS))
    args = ap.parse_args(argv)
    import torch

    import bench
    from bench import _chk, _p
    from charon_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    result = {"tool": "tools/slot_select_bench.py", "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
              "configs": {}}
    for name, wl_name, frac in CONFIGS:
        if name not in args.configs.split(","):
            continue
        wl = bench.WORKLOADS[wl_name]
        V = args.validators or wl["validators"]
        d = bench.setup_inputs(L, wl, V, 0)
        bench.corrupt(L, d, frac, seed=7)
        n, t, NP, M = d["n"], d["t"], d["NP"], d["M"]
        good = d["exp_v"].reshape(V, n) == 0
        want_a = int((good.sum(axis=1) >= t).sum())
        want_c = int((d["exp_agg"] == 0).sum())

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

        g = dict(msgs=up(d["msgs"]), moff=up(d["moff"].view(np.int64)), mlen=up(d["mlen"].view(np.int32)),
                 pks=up(d["pks"]), sigs=up(d["sigs"]), midx=up(d["midx"].view(np.int32)),
                 vgoff=up(d["vgrp_off"].view(np.int32)), dvpk=up(d["dv_pks"]),
                 csrc=up(np.arange(NP, dtype=np.int32)), cidx=up(np.tile(np.arange(1, n + 1, dtype=np.int64), V)),
                 cgoff=up((np.arange(V + 1, dtype=np.uint32) * n).view(np.int32)),
                 fsrc=up(d["ta_src"].view(np.int32)), fidx=up(d["ta_idx"]), fgoff=up(d["grp_off"].view(np.int32)))
        hm = torch.zeros(M * L.hbls_hm_entry_bytes(), dtype=torch.uint8, device=dev)
        vst = torch.full((NP,), 255, dtype=torch.uint8, device=dev)
        tout = torch.zeros(V * 96, dtype=torch.uint8, device=dev)
        tst = torch.full((V,), 255, dtype=torch.uint8, device=dev)
        ast = torch.full((V,), 255, dtype=torch.uint8, device=dev)
        chosen = torch.zeros(V * t, dtype=torch.int32, device=dev)
        count = torch.zeros(V, dtype=torch.int32, device=dev)
        msg_of_v = d["midx"].reshape(V, n)[:, 0].copy()
        root = d["root_sigs"].reshape(V, 96)

        def slot(src, idx, goff, n_members):
            return _lib.HblsSlot(msgs=_p(g["msgs"]).value, msg_off=_p(g["moff"]).value, msg_len=_p(g["mlen"]).value,
                                 n_msgs=M, hm=_p(hm).value, pks=_p(g["pks"]).value, sigs=_p(g["sigs"]).value,
                                 msg_idx=_p(g["midx"]).value, n=NP, vgrp_off=_p(g["vgoff"]).value, n_vgroups=V,
                                 vstatus=_p(vst).value, ta_sigs=None, ta_src=_p(src).value, ta_idx=_p(idx).value,
                                 grp_off=_p(goff).value, n_groups=V, n_ta_partials=n_members, ta_out=_p(tout).value,
                                 ta_status=_p(tst).value, dv_pks=_p(g["dvpk"]).value, agg_vstatus=_p(ast).value)

        slot_a, slot_c = slot(g["csrc"], g["cidx"], g["cgoff"], NP), slot(g["fsrc"], g["fidx"], g["fgoff"], V * t)

        def leg_a():
            t0 = time.perf_counter()
            _chk(L, L.hbls_slot_select_device(ctypes.byref(slot_a), t, _p(chosen), _p(count), sp))
            stream.synchronize()
            ms_ = (time.perf_counter() - t0) * 1e3
            a, o = ast.cpu().numpy(), tout.cpu().numpy().reshape(V, 96)
            ok = a == 0
            assert np.array_equal(o[ok], root[ok])
            return ms_, int(ok.sum())

        def leg_b():
            t0 = time.perf_counter()
            _chk(L, L.hbls_hash_to_g2_device(_p(g["msgs"]), _p(g["moff"]), _p(g["mlen"]), M, _p(hm), sp))
            _chk(L, L.hbls_verify_device(_p(g["pks"]), _p(g["sigs"]), _p(g["midx"]), _p(hm), NP, _p(g["vgoff"]), V,
                                         _p(vst), sp))
            stream.synchronize()
            ok_p = vst.cpu().numpy().reshape(V, n) == 0
            have = np.nonzero(ok_p.sum(axis=1) >= t)[0]
            pos = np.argsort(~ok_p[have], axis=1, kind="stable")[:, :t]
            mem = (have[:, None] * n + pos).reshape(-1)
            K = len(have)
            with torch.cuda.stream(stream):
                d_mem = up(mem.astype(np.int64))
                d_msig = g["sigs"].view(NP, 96).index_select(0, d_mem).reshape(-1)
                d_midx = up((pos + 1).astype(np.int64).reshape(-1))
                d_goff = up((np.arange(K + 1, dtype=np.uint32) * t).view(np.int32))
                d_out = torch.zeros(K * 96, dtype=torch.uint8, device=dev)
                d_tst = torch.full((K,), 255, dtype=torch.uint8, device=dev)
                d_ast = torch.full((K,), 255, dtype=torch.uint8, device=dev)
                d_have = up(have.astype(np.int64))
                d_dv = g["dvpk"].view(V, 48).index_select(0, d_have).reshape(-1)
                d_am = up(msg_of_v[have].view(np.int32))
            _chk(L, L.hbls_threshold_aggregate_device(_p(d_msig), _p(d_midx), _p(d_goff), K, K * t, _p(d_out), _p(d_tst),
                                                      sp))
            _chk(L, L.hbls_verify_device(_p(d_dv), _p(d_out), _p(d_am), _p(hm), K, None, K, _p(d_ast), sp))
            stream.synchronize()
            ms_ = (time.perf_counter() - t0) * 1e3
            ok = (d_tst.cpu().numpy() == 0) & (d_ast.cpu().numpy() == 0)
            assert np.array_equal(d_out.cpu().numpy().reshape(K, 96)[ok], root[have][ok])
            return ms_, int(ok.sum())

        def leg_c():
            t0 = time.perf_counter()
            _chk(L, L.hbls_slot_device(ctypes.byref(slot_c), sp))
            stream.synchronize()
            return (time.perf_counter() - t0) * 1e3, int((ast.cpu().numpy() == 0).sum())

        legs = (("a", leg_a), ("b", leg_b), ("c", leg_c))
        for _, fn in legs:  # warm-up: workspaces, learned keys
            fn()
        _lib.slot_select_stats(L)
        ms = {k: [] for k, _ in legs}
        got = {}
        for _ in range(args.rounds):
            for k, fn in legs:
                torch.cuda.synchronize(dev)
                one, got[k] = fn()
                ms[k].append(one)
        st = _lib.slot_select_stats(L)
        assert got["a"] == want_a and got["b"] == want_a and got["c"] == want_c, (got, want_a, want_c)
        result["configs"][name] = {
            "workload": wl_name, "validators": V, "n": n, "t": t, "messages": M, "corrupted_fraction": frac,
            "validators_with_t_good_partials": want_a,
            "legs": {k: {"ms_per_slot_median": round(statistics.median(ms[k]), 3),
                         "ms_per_slot_runs": [round(x, 3) for x in ms[k]], "verified_aggregates": got[k]} for k, _ in legs},
            "a_small_path_share": round(st["small_path"] / max(1, st["groups"] - st["too_few"]), 4),
            "a_select_stats": st,
        }
        print(name, json.dumps(result["configs"][name]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
