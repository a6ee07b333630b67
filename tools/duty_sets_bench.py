"""Set-atomic duty adds (hbls_duty_add_sets, hbls_duty_add_sets_first) against hbls_duty_add on the same
arrival, on one GPU.

    python tools/duty_sets_bench.py --tag new    [--rounds 3] [--legs add,sets,window,first,first_window] --out new_1.json
    python tools/duty_sets_bench.py --tag parent  --legs add                            --out parent_1.json
    python tools/duty_sets_bench.py --merge parent_1.json new_1.json ... --out profiles/duty_sets_bench.json

Inputs as tools/duty_bench.py's (whose output this tool leaves alone): C3, 100 k validators 7 of 10,
clean; the C5 shard, 125 k validators 5 of 7, clean and at 1 % and 10 % corrupted partials, arriving as n
peer-major sets of V partials.  One duty per leg and round, one call at a time, legs alternating:
  add     n hbls_duty_add, one per peer's set (runs on a library without the set-atomic call: --tag
          parent under HBLS_LIBRARY is the parent commit's figure)
  sets    n hbls_duty_add_sets, one set per call
  window  every peer's set of the duty as ONE hbls_duty_add_sets call of n sets
  first, first_window  as sets and window, through hbls_duty_add_sets_first: a rejected set stops at its first
          failure (reported with them: the partials it left HBLS_UNCHECKED, hbls_duty_first_stats)
Per leg: the time per duty (open and close included), the time of every call, the validators that
fired and the sets rejected.  On the clean streams every leg must end with every validator's
aggregate; at 1 % and 10 % corrupted every set of 125 k partials holds a bad one, so every leg but `add`
rejects every set and fires nothing -- what is measured there is the cost of a rejected set.
--split N runs the legs over N contexts of the one GPU (hbls_debug_split): a duty of N shards, where
hbls_duty_add_sets takes its two-phase path; give such a run a tag of its own (--tag new_split2).
--merge puts the runs of several processes (alternating libraries) side by side: medians and spreads
over all their rounds, per tag.
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

CONFIGS = [("c3_clean", "c3", 0.0), ("c5_clean", "c5", 0.0), ("c5_1pct", "c5", 0.01), ("c5_10pct", "c5", 0.1)]
LEGS = ("add", "sets", "window", "first", "first_window")


def summary(xs):
    return {"median": round(statistics.median(xs), 3), "runs": [round(x, 3) for x in xs], "spread": round(max(xs) - min(xs), 3)}


def merge(paths, out):
    res = {"tool": "tools/duty_sets_bench.py --merge", "processes": [], "configs": {}}
    for p in paths:
        with open(p) as f:
            d = json.load(f)
        res["processes"].append({"tag": d["tag"], "split": d.get("split", 1), "library": d["library"], "device": d["device"],
                                 "rounds": d["rounds"]})
        for name, c in d["configs"].items():
            m = res["configs"].setdefault(name, {k: c[k] for k in ("workload", "validators", "n", "t", "corrupted_fraction")})
            for leg, v in c["legs"].items():
                e = m.setdefault("legs", {}).setdefault(d["tag"] + ":" + leg, {"total": [], "calls": [], "fired": v["fired"],
                                                                              "sets_rejected": v["sets_rejected"]})
                if "unchecked" in v:
                    e["unchecked"] = v["unchecked"]
                e["total"] += v["total_ms"]["runs"]
                e["calls"] += v["calls_ms_runs"]
    for c in res["configs"].values():
        for leg, e in c["legs"].items():
            calls = e.pop("calls")
            e["total_ms"] = summary(e.pop("total"))
            e["calls_ms_median"] = [round(statistics.median(r[j] for r in calls), 3) for j in range(len(calls[0]))]
            e["per_call_ms"] = summary([sum(r) / len(r) for r in calls])
    with open(out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "duty_sets_bench.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--validators", type=int, default=0, help="override the shard size (smoke runs)")
    ap.add_argument("--configs", default=",".join(c[0] for c in CONFIGS))
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--tag", default="new")
    ap.add_argument("--split", type=int, default=1, help="hbls_debug_split(N): N contexts (shards) on the one GPU")
    ap.add_argument("--merge", nargs="+")
    args = ap.parse_args(argv)
    if args.merge:
        return merge(args.merge, args.out)
    import ctypes

    import torch

    import bench
    from bench import _chk, _p
    from charon_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    want_legs = args.legs.split(",")
    if args.split != 1:
        _chk(L, L.hbls_debug_split(args.split))
    result = {"tool": "tools/duty_sets_bench.py", "tag": args.tag, "split": args.split, "rounds": args.rounds, "legs": want_legs,
              "library": L.hbls_build_id().decode(), "device": torch.cuda.get_device_name(0), "configs": {}}
    for name, wl_name, frac in CONFIGS:
        if name not in args.configs.split(","):
            continue
        wl = bench.WORKLOADS[wl_name]
        V = args.validators or wl["validators"]
        d = bench.setup_inputs(L, wl, V, 0)
        bench.corrupt(L, d, frac, seed=7)
        n, t, NP = d["n"], d["t"], d["NP"]
        root = d["root_sigs"].reshape(V, 96)

        def peer(a, w):  # validator-major rows -> peer-major
            return np.ascontiguousarray(a.reshape(V, n, w).transpose(1, 0, 2)).reshape(-1)

        h_pks, h_sigs, h_msgs = peer(d["pks"], 48), peer(d["sigs"], 96), peer(d["item_msgs"], 32)
        h_off, h_len = np.arange(NP, dtype=np.uint64) * 32, np.full(NP, 32, dtype=np.uint32)
        grp_all = np.tile(np.arange(V, dtype=np.uint32), n)
        sidx_all = np.repeat(np.arange(1, n + 1, dtype=np.int64), V)
        bad_sets = int((d["exp_v"].reshape(V, n) != 0).any(axis=0).sum())  # peer k's set holds a bad partial

        def duty(mode):
            """mode: add / sets / first (one call per peer's set) or window / first_window (one call)"""
            per = NP if mode.endswith("window") else V
            n_calls = NP // per
            vst, stored = np.full(per, 255, np.uint8), np.zeros(per, np.uint8)
            rows = min(per, V)
            fired, chosen = np.zeros(rows, np.uint32), np.zeros(rows * t, np.uint32)
            out, tst, ast = np.zeros(rows * 96, np.uint8), np.full(rows, 255, np.uint8), np.full(rows, 255, np.uint8)
            n_sets = per // V
            set_off, set_first = np.arange(n_sets + 1, dtype=np.uint32) * V, np.zeros(n_sets, np.uint32)
            first, nf, h = ctypes.c_uint32(0), ctypes.c_size_t(0), ctypes.c_uint64(0)
            calls, good, rejected = [], 0, 0
            add_sets = L.hbls_duty_add_sets_first if mode.startswith("first") else L.hbls_duty_add_sets
            t0 = time.perf_counter()
            _chk(L, L.hbls_duty_open(_p(d["dv_pks"]), V, t, n, ctypes.byref(h)))
            t_open = (time.perf_counter() - t0) * 1e3
            for k in range(n_calls):
                a = (h.value, _p(h_pks[48 * per * k:]), _p(h_sigs[96 * per * k:]), _p(h_msgs[32 * per * k:]), _p(h_off), _p(h_len),
                     _p(grp_all[per * k:]), _p(sidx_all[per * k:]), per)
                b = (_p(fired), ctypes.byref(nf), _p(chosen), _p(out), _p(tst), _p(ast))
                t1 = time.perf_counter()
                if mode == "add":
                    _chk(L, L.hbls_duty_add(*a, _p(vst), _p(stored), ctypes.byref(first), *b))
                else:
                    _chk(L, add_sets(*a, _p(set_off), n_sets, _p(vst), _p(stored), ctypes.byref(first), _p(set_first), *b))
                calls.append((time.perf_counter() - t1) * 1e3)
                f = nf.value
                ok = (tst[:f] == 0) & (ast[:f] == 0)
                assert np.array_equal(out.reshape(rows, 96)[:f][ok], root[fired[:f]][ok])
                good += int(ok.sum())
                if mode != "add":
                    rejected += int((set_first != 0xFFFFFFFF).sum())
            if mode.startswith("first"):
                fs = np.zeros(2, np.uint64)
                _chk(L, L.hbls_duty_first_stats(h.value, _p(fs), 2))
                unchecked[mode] = int(fs[1])
            t2 = time.perf_counter()
            _chk(L, L.hbls_duty_close(h.value))
            t_close = (time.perf_counter() - t2) * 1e3
            return dict(total=sum(calls) + t_open + t_close, calls=calls), good, rejected

        unchecked = {}
        legs = [k for k in LEGS if k in want_legs]
        for k in legs:  # warm-up: workspaces, staging buffers, learned keys
            duty(k)
        runs, got, rej = {k: [] for k in legs}, {}, {}
        for _ in range(args.rounds):
            for k in legs:
                torch.cuda.synchronize(dev)
                one, got[k], rej[k] = duty(k)
                runs[k].append(one)
        want_add = int(((d["exp_v"].reshape(V, n) == 0).sum(axis=1) >= t).sum())
        for k in legs:
            if k == "add":
                assert got[k] == want_add, (k, got[k], want_add)
            else:
                assert rej[k] == bad_sets, (k, rej[k], bad_sets)
                assert got[k] == (V if n - bad_sets >= t else 0), (k, got[k])
        result["configs"][name] = {
            "workload": wl_name, "validators": V, "n": n, "t": t, "corrupted_fraction": frac,
            "legs": {k: {"total_ms": summary([r["total"] for r in runs[k]]), "calls_ms_runs": [r["calls"] for r in runs[k]],
                         "fired": got[k], "sets_rejected": rej[k], **({"unchecked": unchecked[k]} if k in unchecked else {})}
                     for k in legs},
        }
        print(name, json.dumps({k: result["configs"][name]["legs"][k]["total_ms"] for k in legs}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
