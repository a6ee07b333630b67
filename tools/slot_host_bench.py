"""hbls_slot_select_batch against what the Go shim has to do without it, on one GPU in one run.

    python tools/slot_host_bench.py [--out profiles/slot_host_bench.json] [--rounds 3]

Inputs in host memory, peer-major (item = share V + validator, the way parsigex receives them): the
C5 shard, 125 k validators 5 of 7, clean and at 1 % corrupted partials; C3, 100 k validators 7 of 10,
clean (bench.corrupt's mix).  Three legs, alternating, one call at a time, medians reported:
  a  hbls_slot_select_batch
  b  the three-call route: hbls_verify_batch, the members picked with numpy,
     hbls_threshold_aggregate_batch over their bytes (the signature cache at its default),
     hbls_verify_batch over the aggregates
  c  hbls_slot_select_device on resident inputs (validator-major, one verification group per
     validator): the floor, no transfer and no host preparation
Then (a) and (b) again from three threads at once (three buffer sets): ms per slot = wall clock / 3.
Per leg: ms per slot (wall clock of the blocking calls, host steps included), the spread of the runs,
and the validators that end with a verified aggregate.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = [("c5_clean", "c5", 0.0), ("c5_1pct", "c5", 0.01), ("c3_clean", "c3", 0.0)]
THREADS = 3


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slot_host_bench.json"))
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
    result = {"tool": "tools/slot_host_bench.py", "rounds": args.rounds, "threads": THREADS,
              "device": torch.cuda.get_device_name(0), "configs": {}}
    for name, wl_name, frac in CONFIGS:
        if name not in args.configs.split(","):
            continue
        wl = bench.WORKLOADS[wl_name]
        V = args.validators or wl["validators"]
        d = bench.setup_inputs(L, wl, V, 0)
        bench.corrupt(L, d, frac, seed=7)
        n, t, NP, M = d["n"], d["t"], d["NP"], d["M"]
        want = int(((d["exp_v"].reshape(V, n) == 0).sum(axis=1) >= t).sum())
        root = d["root_sigs"].reshape(V, 96)

        def peer(a, w):  # validator-major rows -> peer-major
            return np.ascontiguousarray(a.reshape(V, n, w).transpose(1, 0, 2)).reshape(-1)

        h_pks, h_sigs, h_msgs = peer(d["pks"], 48), peer(d["sigs"], 96), peer(d["item_msgs"], 32)
        h_off, h_len = np.arange(NP, dtype=np.uint64) * 32, np.full(NP, 32, dtype=np.uint32)
        h_cand = (np.arange(V, dtype=np.uint32)[:, None] + np.arange(n, dtype=np.uint32)[None, :] * V).reshape(-1)
        h_cidx = np.tile(np.arange(1, n + 1, dtype=np.int64), V)
        h_goff = np.arange(V + 1, dtype=np.uint32) * n
        v_msgs = d["item_msgs"].reshape(V, n, 32)[:, 0].copy()

        def buffers():
            return dict(vst=np.full(NP, 255, np.uint8), chosen=np.zeros(V * t, np.uint32), count=np.zeros(V, np.uint32),
                        out=np.zeros(V * 96, np.uint8), tst=np.full(V, 255, np.uint8), ast=np.full(V, 255, np.uint8))

        bufs = [buffers() for _ in range(THREADS)]

        def leg_a(b=bufs[0]):
            t0 = time.perf_counter()
            _chk(L, L.hbls_slot_select_batch(_p(h_pks), _p(h_sigs), _p(h_msgs), _p(h_off), _p(h_len), NP, _p(h_cand),
                                             _p(h_cidx), _p(h_goff), V, _p(d["dv_pks"]), t, _p(b["vst"]), _p(b["chosen"]),
                                             _p(b["count"]), _p(b["out"]), _p(b["tst"]), _p(b["ast"])))
            ms_ = (time.perf_counter() - t0) * 1e3
            ok = b["ast"] == 0
            assert np.array_equal(b["out"].reshape(V, 96)[ok], root[ok])
            return ms_, int(ok.sum())

        def leg_b(b=bufs[0]):
            t0 = time.perf_counter()
            _chk(L, L.hbls_verify_batch(_p(h_pks), _p(h_sigs), _p(h_msgs), _p(h_off), _p(h_len), NP, _p(b["vst"])))
            ok_p = (b["vst"].reshape(n, V) == 0).T
            have = np.nonzero(ok_p.sum(axis=1) >= t)[0]
            pos = np.argsort(~ok_p[have], axis=1, kind="stable")[:, :t]
            K = len(have)
            m_sigs = np.ascontiguousarray(h_sigs.reshape(NP, 96)[(pos * V + have[:, None]).reshape(-1)]).reshape(-1)
            m_idx = (pos + 1).astype(np.int64).reshape(-1)
            m_goff = np.arange(K + 1, dtype=np.uint32) * t
            out, tst, ast = np.zeros(K * 96, np.uint8), np.full(K, 255, np.uint8), np.full(K, 255, np.uint8)
            _chk(L, L.hbls_threshold_aggregate_batch(_p(m_sigs), _p(m_idx), _p(m_goff), K, _p(out), _p(tst)))
            a_pks = np.ascontiguousarray(d["dv_pks"].reshape(V, 48)[have]).reshape(-1)
            a_msgs = np.ascontiguousarray(v_msgs[have]).reshape(-1)
            a_off, a_len = np.arange(K, dtype=np.uint64) * 32, np.full(K, 32, dtype=np.uint32)
            _chk(L, L.hbls_verify_batch(_p(a_pks), _p(out), _p(a_msgs), _p(a_off), _p(a_len), K, _p(ast)))
            ms_ = (time.perf_counter() - t0) * 1e3
            ok = (tst == 0) & (ast == 0)
            assert np.array_equal(out.reshape(K, 96)[ok], root[have][ok])
            return ms_, int(ok.sum())

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

        g = dict(msgs=up(d["msgs"]), moff=up(d["moff"].view(np.int64)), mlen=up(d["mlen"].view(np.int32)),
                 pks=up(d["pks"]), sigs=up(d["sigs"]), midx=up(d["midx"].view(np.int32)),
                 vgoff=up(d["vgrp_off"].view(np.int32)), dvpk=up(d["dv_pks"]), csrc=up(np.arange(NP, dtype=np.int32)),
                 cidx=up(h_cidx), cgoff=up(h_goff.view(np.int32)))
        hm = torch.zeros(M * L.hbls_hm_entry_bytes(), dtype=torch.uint8, device=dev)
        vst = torch.full((NP,), 255, dtype=torch.uint8, device=dev)
        tout = torch.zeros(V * 96, dtype=torch.uint8, device=dev)
        tst = torch.full((V,), 255, dtype=torch.uint8, device=dev)
        ast = torch.full((V,), 255, dtype=torch.uint8, device=dev)
        chosen = torch.zeros(V * t, dtype=torch.int32, device=dev)
        count = torch.zeros(V, dtype=torch.int32, device=dev)
        slot = _lib.HblsSlot(msgs=_p(g["msgs"]).value, msg_off=_p(g["moff"]).value, msg_len=_p(g["mlen"]).value, n_msgs=M,
                             hm=_p(hm).value, pks=_p(g["pks"]).value, sigs=_p(g["sigs"]).value,
                             msg_idx=_p(g["midx"]).value, n=NP, vgrp_off=_p(g["vgoff"]).value, n_vgroups=V,
                             vstatus=_p(vst).value, ta_sigs=None, ta_src=_p(g["csrc"]).value, ta_idx=_p(g["cidx"]).value,
                             grp_off=_p(g["cgoff"]).value, n_groups=V, n_ta_partials=NP, ta_out=_p(tout).value,
                             ta_status=_p(tst).value, dv_pks=_p(g["dvpk"]).value, agg_vstatus=_p(ast).value)

        def leg_c():
            t0 = time.perf_counter()
            _chk(L, L.hbls_slot_select_device(ctypes.byref(slot), t, _p(chosen), _p(count), sp))
            stream.synchronize()
            return (time.perf_counter() - t0) * 1e3, int((ast.cpu().numpy() == 0).sum())

        def threaded(fn):
            got, errs = [None] * THREADS, []

            def work(k):
                try:
                    got[k] = fn(bufs[k])
                except BaseException as e:  # noqa: BLE001 -- reported by the main thread
                    errs.append(repr(e))

            th = [threading.Thread(target=work, args=(k,)) for k in range(THREADS)]
            t0 = time.perf_counter()
            for x in th:
                x.start()
            for x in th:
                x.join()
            ms_ = (time.perf_counter() - t0) * 1e3 / THREADS
            assert not errs, errs
            assert all(x[1] == got[0][1] for x in got)
            return ms_, got[0][1]

        legs = (("a", leg_a), ("b", leg_b), ("c", leg_c), ("a_3_threads", lambda: threaded(leg_a)),
                ("b_3_threads", lambda: threaded(leg_b)))
        for _, fn in legs:  # warm-up: workspaces, staging buffers, learned keys
            fn()
        ms = {k: [] for k, _ in legs}
        got = {}
        for group in (legs[:3], legs[3:]):
            for _ in range(args.rounds):
                for k, fn in group:
                    torch.cuda.synchronize(dev)
                    one, got[k] = fn()
                    ms[k].append(one)
        assert all(v == want for v in got.values()), (got, want)
        result["configs"][name] = {
            "workload": wl_name, "validators": V, "n": n, "t": t, "messages": M, "corrupted_fraction": frac,
            "validators_with_t_good_partials": want, "bytes_per_call_144_per_partial": 144 * NP,
            "legs": {k: {"ms_per_slot_median": round(statistics.median(ms[k]), 3),
                         "ms_per_slot_runs": [round(x, 3) for x in ms[k]],
                         "ms_per_slot_spread": round(max(ms[k]) - min(ms[k]), 3), "verified_aggregates": got[k]}
                     for k, _ in legs},
        }
        print(name, json.dumps(result["configs"][name]), flush=True)
        del g, hm, vst, tout, tst, ast, chosen, count
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
