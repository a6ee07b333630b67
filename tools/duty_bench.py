"""Duty sessions against the route a node has today under the same arrival, on one GPU in one run.

    python tools/duty_bench.py [--out profiles/duty_bench.json] [--rounds 3] [--legs a,b,c]

Inputs in host memory, arriving as n peer-major sets of V partials (set k = every validator's share
k + 1, the way parsigex receives them): C3, 100 k validators 7 of 10, clean; the C5 shard, 125 k
validators 5 of 7, at 1 % corrupted partials (bench.corrupt's mix).  Three legs, alternating, one
call at a time, medians reported:
  a  one duty session: hbls_duty_open, n hbls_duty_add, hbls_duty_close
  b  today's route: per set one hbls_verify_batch; from the set that brings a validator its t-th
     verified partial on, the members picked with numpy, hbls_threshold_aggregate_batch over their
     bytes (the signature cache at its default) and hbls_verify_batch over the aggregates
  c  one hbls_slot_select_batch over everything: the floor, which cannot start before the last set
Per leg: the total call time per duty, the time of the firing call (set t arrives -> aggregates
returned), the time of every call, and the validators ending with a verified aggregate (equal across
legs).  Leg b uses only entry points older than the duty sessions: --legs b runs on a checkout
without them.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = [("c3_clean", "c3", 0.0), ("c5_1pct", "c5", 0.01)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "duty_bench.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--validators", type=int, default=0, help="override the shard size (smoke runs)")
    ap.add_argument("--configs", default=",".join(c[0] for c in CONFIGS))
    ap.add_argument("--legs", default="a,b,c")
    args = ap.parse_args(argv)
    import ctypes

    import torch

    import bench
    from bench import _chk, _p
    from charon_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    want_legs = args.legs.split(",")
    result = {"tool": "tools/duty_bench.py", "rounds": args.rounds, "legs": want_legs,
              "library": L.hbls_build_id().decode() if hasattr(L, "hbls_build_id") else "",
              "device": torch.cuda.get_device_name(0), "configs": {}}
    for name, wl_name, frac in CONFIGS:
        if name not in args.configs.split(","):
            continue
        wl = bench.WORKLOADS[wl_name]
        V = args.validators or wl["validators"]
        d = bench.setup_inputs(L, wl, V, 0)
        bench.corrupt(L, d, frac, seed=7)
        n, t, NP = d["n"], d["t"], d["NP"]
        want = int(((d["exp_v"].reshape(V, n) == 0).sum(axis=1) >= t).sum())
        root = d["root_sigs"].reshape(V, 96)

        def peer(a, w):  # validator-major rows -> peer-major
            return np.ascontiguousarray(a.reshape(V, n, w).transpose(1, 0, 2)).reshape(-1)

        h_pks, h_sigs, h_msgs = peer(d["pks"], 48), peer(d["sigs"], 96), peer(d["item_msgs"], 32)
        h_off, h_len = np.arange(NP, dtype=np.uint64) * 32, np.full(NP, 32, dtype=np.uint32)
        v_msgs = d["item_msgs"].reshape(V, n, 32)[:, 0].copy()
        grp = np.arange(V, dtype=np.uint32)
        dv = d["dv_pks"].reshape(V, 48)

        def leg_a():
            vst, stored = np.full(V, 255, np.uint8), np.zeros(V, np.uint8)
            fired, chosen = np.zeros(V, np.uint32), np.zeros(V * t, np.uint32)
            out, tst, ast = np.zeros(V * 96, np.uint8), np.full(V, 255, np.uint8), np.full(V, 255, np.uint8)
            first, nf, h = ctypes.c_uint32(0), ctypes.c_size_t(0), ctypes.c_uint64(0)
            calls, good = [], 0
            t0 = time.perf_counter()
            _chk(L, L.hbls_duty_open(_p(d["dv_pks"]), V, t, n, ctypes.byref(h)))
            t_open = (time.perf_counter() - t0) * 1e3
            for k in range(n):
                sidx = np.full(V, k + 1, dtype=np.int64)
                t1 = time.perf_counter()
                _chk(L, L.hbls_duty_add(h.value, _p(h_pks[48 * V * k:]), _p(h_sigs[96 * V * k:]), _p(h_msgs[32 * V * k:]),
                                        _p(h_off), _p(h_len), _p(grp), _p(sidx), V, _p(vst), _p(stored), ctypes.byref(first),
                                        _p(fired), ctypes.byref(nf), _p(chosen), _p(out), _p(tst), _p(ast)))
                calls.append((time.perf_counter() - t1) * 1e3)
                f = nf.value
                ok = (tst[:f] == 0) & (ast[:f] == 0)
                assert np.array_equal(out.reshape(V, 96)[:f][ok], root[fired[:f]][ok])
                good += int(ok.sum())
            t2 = time.perf_counter()
            _chk(L, L.hbls_duty_close(h.value))
            t_close = (time.perf_counter() - t2) * 1e3
            return dict(total=sum(calls) + t_open + t_close, firing=calls[t - 1], calls=calls, open=t_open, close=t_close), good

        def leg_b():
            ok_p = np.zeros((V, n), dtype=bool)  # validator x set: verified
            done = np.zeros(V, dtype=bool)
            calls, good = [], 0
            for k in range(n):
                vst = np.full(V, 255, np.uint8)
                t1 = time.perf_counter()
                _chk(L, L.hbls_verify_batch(_p(h_pks[48 * V * k:]), _p(h_sigs[96 * V * k:]), _p(h_msgs[32 * V * k:]), _p(h_off),
                                            _p(h_len), V, _p(vst)))
                ok_p[:, k] = vst == 0
                if k >= t - 1:
                    have = np.nonzero(~done & (ok_p[:, :k + 1].sum(axis=1) >= t))[0]
                    K = len(have)
                    if K:
                        pos = np.argsort(~ok_p[have, :k + 1], axis=1, kind="stable")[:, :t]
                        m_sigs = np.ascontiguousarray(h_sigs.reshape(NP, 96)[(pos * V + have[:, None]).reshape(-1)]).reshape(-1)
                        m_idx = (pos + 1).astype(np.int64).reshape(-1)
                        m_goff = np.arange(K + 1, dtype=np.uint32) * t
                        out, tst, ast = np.zeros(K * 96, np.uint8), np.full(K, 255, np.uint8), np.full(K, 255, np.uint8)
                        _chk(L, L.hbls_threshold_aggregate_batch(_p(m_sigs), _p(m_idx), _p(m_goff), K, _p(out), _p(tst)))
                        a_pks = np.ascontiguousarray(dv[have]).reshape(-1)
                        a_msgs = np.ascontiguousarray(v_msgs[have]).reshape(-1)
                        a_off, a_len = np.arange(K, dtype=np.uint64) * 32, np.full(K, 32, dtype=np.uint32)
                        _chk(L, L.hbls_verify_batch(_p(a_pks), _p(out), _p(a_msgs), _p(a_off), _p(a_len), K, _p(ast)))
                        done[have] = True
                calls.append((time.perf_counter() - t1) * 1e3)
                if k >= t - 1 and K:
                    ok = (tst == 0) & (ast == 0)
                    assert np.array_equal(out.reshape(K, 96)[ok], root[have][ok])
                    good += int(ok.sum())
            return dict(total=sum(calls), firing=calls[t - 1], calls=calls), good

        h_cand = (np.arange(V, dtype=np.uint32)[:, None] + np.arange(n, dtype=np.uint32)[None, :] * V).reshape(-1)
        h_cidx = np.tile(np.arange(1, n + 1, dtype=np.int64), V)
        h_goff = np.arange(V + 1, dtype=np.uint32) * n

        def leg_c():
            vst, chosen, count = np.full(NP, 255, np.uint8), np.zeros(V * t, np.uint32), np.zeros(V, np.uint32)
            out, tst, ast = np.zeros(V * 96, np.uint8), np.full(V, 255, np.uint8), np.full(V, 255, np.uint8)
            t0 = time.perf_counter()
            _chk(L, L.hbls_slot_select_batch(_p(h_pks), _p(h_sigs), _p(h_msgs), _p(h_off), _p(h_len), NP, _p(h_cand),
                                             _p(h_cidx), _p(h_goff), V, _p(d["dv_pks"]), t, _p(vst), _p(chosen), _p(count),
                                             _p(out), _p(tst), _p(ast)))
            ms_ = (time.perf_counter() - t0) * 1e3
            ok = ast == 0
            assert np.array_equal(out.reshape(V, 96)[ok], root[ok])
            return dict(total=ms_, firing=ms_, calls=[ms_]), int(ok.sum())

        legs = [(k, fn) for k, fn in (("a", leg_a), ("b", leg_b), ("c", leg_c)) if k in want_legs]
        for _, fn in legs:  # warm-up: workspaces, staging buffers, learned keys
            fn()
        runs = {k: [] for k, _ in legs}
        got = {}
        for _ in range(args.rounds):
            for k, fn in legs:
                torch.cuda.synchronize(dev)
                one, got[k] = fn()
                runs[k].append(one)
        assert all(v == want for v in got.values()), (got, want)

        def summary(rs, key):
            xs = [r[key] for r in rs]
            return {"median": round(statistics.median(xs), 3), "runs": [round(x, 3) for x in xs],
                    "spread": round(max(xs) - min(xs), 3)}

        result["configs"][name] = {
            "workload": wl_name, "validators": V, "n": n, "t": t, "messages": d["M"], "corrupted_fraction": frac,
            "validators_with_t_good_partials": want,
            "legs": {k: {"total_ms": summary(runs[k], "total"), "firing_call_ms": summary(runs[k], "firing"),
                         "calls_ms_median": [round(statistics.median(r["calls"][j] for r in runs[k]), 3)
                                             for j in range(len(runs[k][0]["calls"]))],
                         "verified_aggregates": got[k]} for k, _ in legs},
        }
        print(name, json.dumps(result["configs"][name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
