"""Cluster duties against plain duties under the same arrival, on one GPU in one run.

    python tools/cluster_bench.py [--out profiles/cluster_bench.json] [--rounds 3] [--legs a,b,c]

The C3 stream: 100 k validators 7 of 10, clean, in host memory, arriving as n peer-major sets of V
partials (set k = every validator's share k + 1), one set per call through hbls_duty_add_sets_first.
Three legs, alternating in one process, one call at a time, medians with spread (max - min) reported:
  a  a plain duty, the learned key cache warm: every call gathers and uploads 48 bytes per partial and
     finds them again by their bytes (k_pk_lookup)
  b  a duty on a cluster with ladder tables: no keys passed, k_cluster_keys resolves them
  c  a duty on a cluster without ladder tables
Per leg: the total call time per duty (open and close included), the per-call times, and the validators
ending with a verified aggregate (equal across legs, compared with the root keys' signatures).  Leg a uses
only entry points older than the cluster handles: --legs a runs on a checkout without them.
For the clusters: wall time, device bytes allocated and kernel times (hbls_timing) of hbls_cluster_open,
with and without tables.  --trace-calls N (with hbls_timing): the library's own per-kernel times of N
calls of legs a and b, k_cluster_keys beside k_pk_lookup.

What other runs of the same visit measured is merged into the profile by this tool as well, either with
the run or afterwards into an existing profile (--merge-into FILE: no GPU, nothing else is touched):
  --parent-json FILE    this tool's --legs a output on a checkout of the parent commit -> "parent_commit",
                        and "verdict": the two margins (plain duty against the parent's, cluster duty with
                        tables against the plain duty), each against the larger of the two spreads
  --kernel-stats FILE   the kernel statistics CSV of one `rocprofv3 --kernel-trace --stats --output-format
                        csv -- python tools/cluster_bench.py --rounds 1 --legs a,b` run -> "kernel_trace"
                        (the key phase's kernels only)
  --bench-this FILE / --bench-parent FILE (repeatable)   outputs of `bench.py --gpus 1 --steps K --warmup W`
                        on this tree / the parent checkout -> "bench_py_c3_ms_per_step"
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


KEY_PHASE_KERNELS = ("k_cluster_keys", "k_cluster_wide", "k_pk_lookup", "k_pk_miss_dec", "k_pk_miss_subgroup", "k_pk_learn",
                     "k_pk_wide")


def merge_sections(result, args):
    """The sections other runs contribute (the module docstring), into `result`."""
    if args.parent_json:
        with open(args.parent_json) as f:
            par = json.load(f)
        result["parent_commit"] = {"library": par["library"], "results": par["results"],
                                   "note": "leg a on a checkout of the parent commit, same visit, same tool"}
    if "parent_commit" in result and "a" in result.get("results", {}):
        a, pa = result["results"]["a"]["total_ms"], result["parent_commit"]["results"]["a"]["total_ms"]
        v = {"plain_duty_vs_parent_ms": round(a["median"] - pa["median"], 3),
             "margin_larger_spread_ms": max(a["spread"], pa["spread"])}
        v["plain_within_margin"] = abs(v["plain_duty_vs_parent_ms"]) <= v["margin_larger_spread_ms"]
        if "b" in result["results"]:
            b = result["results"]["b"]["total_ms"]
            v["cluster_tables_vs_plain_ms"] = round(b["median"] - a["median"], 3)
            v["margin_b_vs_a_ms"] = max(a["spread"], b["spread"])
            v["cluster_within_margin"] = v["cluster_tables_vs_plain_ms"] <= v["margin_b_vs_a_ms"]
        if "c" in result["results"]:
            v["cluster_no_tables_vs_plain_ms"] = round(result["results"]["c"]["total_ms"]["median"] - a["median"], 3)
        result["verdict"] = v
    if args.kernel_stats:
        import csv
        kern = {}
        with open(args.kernel_stats) as f:
            for r in csv.DictReader(f):
                name = r["Name"].split("(")[0].replace("hb::", "")
                if name in KEY_PHASE_KERNELS:
                    kern[name] = {"calls": int(r["Calls"]), "total_us": round(int(r["TotalDurationNs"]) / 1e3, 1),
                                  "average_us": round(float(r["AverageNs"]) / 1e3, 2), "min_us": round(int(r["MinNs"]) / 1e3, 2),
                                  "max_us": round(int(r["MaxNs"]) / 1e3, 2)}
        result["kernel_trace"] = {"tool": "rocprofv3 --kernel-trace --stats, a run of its own: legs a and b, one warm-up duty "
                                          "(leg a learns the keys cold in it) and one timed duty each", "kernels": kern}
    if args.bench_this or args.bench_parent:
        def line(path):
            with open(path) as f:
                return json.loads([ln for ln in f if ln.startswith("{")][-1])
        lines = {"this_tree": [line(x) for x in args.bench_this], "parent_commit": [line(x) for x in args.bench_parent]}
        one = (lines["this_tree"] + lines["parent_commit"])[0]
        result["bench_py_c3_ms_per_step"] = {k: [x["ms_per_step"] for x in v] for k, v in lines.items()}
        result["bench_py_c3_ms_per_step"]["command"] = \
            f"bench.py --gpus {one['n_gpus']} --steps {one['steps']} --warmup {one['warmup']}, alternating in one visit"


def write(result, out):
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge-into", default="", help="add the sections below to this existing profile and stop (no GPU)")
    ap.add_argument("--parent-json", default="")
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--bench-this", action="append", default=[])
    ap.add_argument("--bench-parent", action="append", default=[])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_bench.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--validators", type=int, default=0, help="override the shard size (smoke runs)")
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--trace-calls", type=int, default=0, help="per-kernel times of this many calls of legs a and b")
    args = ap.parse_args(argv)
    if args.merge_into:
        with open(args.merge_into) as f:
            result = json.load(f)
        merge_sections(result, args)
        write(result, args.merge_into)
        return 0
    import ctypes

    import torch

    import bench
    from bench import _chk, _p
    from charon_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    want_legs = args.legs.split(",")
    have_cluster = hasattr(L, "hbls_cluster_open")
    assert have_cluster or want_legs == ["a"], "this library has no cluster handles: --legs a"
    wl = bench.WORKLOADS["c3"]
    V = args.validators or wl["validators"]
    d = bench.setup_inputs(L, wl, V, 0)
    n, t, NP = d["n"], d["t"], d["NP"]
    root = d["root_sigs"].reshape(V, 96)

    def peer(a, w):  # validator-major rows -> peer-major
        return np.ascontiguousarray(a.reshape(V, n, w).transpose(1, 0, 2)).reshape(-1)

    h_pks, h_sigs, h_msgs = peer(d["pks"], 48), peer(d["sigs"], 96), peer(d["item_msgs"], 32)
    h_off, h_len = np.arange(NP, dtype=np.uint64) * 32, np.full(NP, 32, dtype=np.uint32)
    grp = np.arange(V, dtype=np.uint32)
    set_off = np.asarray([0, V], dtype=np.uint32)
    result = {"tool": "tools/cluster_bench.py", "rounds": args.rounds, "legs": want_legs,
              "library": L.hbls_build_id().decode(), "device": torch.cuda.get_device_name(0), "workload": "c3",
              "validators": V, "n": n, "t": t, "entry": "hbls_duty_add_sets_first, one set per call"}

    def open_cluster(tables):
        """-> (handle, dict(wall_ms, device_bytes, kernels_ms))"""
        st = np.zeros(V * (1 + n), np.uint8)
        h = ctypes.c_uint64(0)
        torch.cuda.synchronize(dev)
        free0 = torch.cuda.mem_get_info(dev)[0]
        _chk(L, L.hbls_timing(1))
        t0 = time.perf_counter()
        _chk(L, L.hbls_cluster_open(_p(d["dv_pks"]), _p(d["pks"]), V, n, tables, _p(st), ctypes.byref(h)))
        wall = (time.perf_counter() - t0) * 1e3
        kern = {}
        for name, ms in _lib.timing_read(L):
            kern[name] = round(kern.get(name, 0.0) + ms, 3)
        _chk(L, L.hbls_timing(0))
        assert not st.any()
        stats = (ctypes.c_uint64 * 6)()
        _chk(L, L.hbls_cluster_stats(h.value, stats, 6))
        return h.value, dict(wall_ms=round(wall, 3), device_bytes=int(free0 - torch.cuda.mem_get_info(dev)[0]),
                             kernels_ms=kern, keys=int(stats[0]), ladder_tables=int(stats[2]))

    clusters = {}
    if have_cluster:
        result["cluster_open"] = {}
        for leg, tables in (("b", 1), ("c", 0)):
            if leg in want_legs:
                clusters[leg], result["cluster_open"]["tables" if tables else "no_tables"] = open_cluster(tables)

    def duty(cluster):
        """one duty over the stream: cluster None -> a plain duty with keys"""
        vst, stored = np.full(V, 255, np.uint8), np.zeros(V, np.uint8)
        fired, chosen = np.zeros(V, np.uint32), np.zeros(V * t, np.uint32)
        out, tst, ast = np.zeros(V * 96, np.uint8), np.full(V, 255, np.uint8), np.full(V, 255, np.uint8)
        first, nf, h, sf = ctypes.c_uint32(0), ctypes.c_size_t(0), ctypes.c_uint64(0), np.zeros(1, np.uint32)
        calls, good = [], 0
        t0 = time.perf_counter()
        if cluster is None:
            _chk(L, L.hbls_duty_open(_p(d["dv_pks"]), V, t, n, ctypes.byref(h)))
        else:
            _chk(L, L.hbls_duty_open_cluster(cluster, t, n, ctypes.byref(h)))
        t_open = (time.perf_counter() - t0) * 1e3
        for k in range(n):
            sidx = np.full(V, k + 1, dtype=np.int64)
            t1 = time.perf_counter()
            _chk(L, L.hbls_duty_add_sets_first(h.value, None if cluster is not None else _p(h_pks[48 * V * k:]),
                                               _p(h_sigs[96 * V * k:]), _p(h_msgs[32 * V * k:]), _p(h_off), _p(h_len), _p(grp),
                                               _p(sidx), V, _p(set_off), 1, _p(vst), _p(stored), ctypes.byref(first), _p(sf),
                                               _p(fired), ctypes.byref(nf), _p(chosen), _p(out), _p(tst), _p(ast)))
            calls.append((time.perf_counter() - t1) * 1e3)
            f = nf.value
            ok = (tst[:f] == 0) & (ast[:f] == 0)
            assert not vst.any() and np.array_equal(out.reshape(V, 96)[:f][ok], root[fired[:f]][ok])
            good += int(ok.sum())
        t2 = time.perf_counter()
        _chk(L, L.hbls_duty_close(h.value))
        t_close = (time.perf_counter() - t2) * 1e3
        return dict(total=sum(calls) + t_open + t_close, calls=calls, open=t_open, close=t_close), good

    legs = [(k, (lambda k=k: duty(clusters.get(k)))) for k in ("a", "b", "c") if k in want_legs]
    for _, fn in legs:  # warm-up: workspaces, staging buffers, learned keys
        fn()
    runs = {k: [] for k, _ in legs}
    got = {}
    for _ in range(args.rounds):
        for k, fn in legs:
            torch.cuda.synchronize(dev)
            one, got[k] = fn()
            runs[k].append(one)
    assert all(v == V for v in got.values()), got

    def summary(xs):
        return {"median": round(statistics.median(xs), 3), "runs": [round(x, 3) for x in xs], "spread": round(max(xs) - min(xs), 3)}

    result["results"] = {
        k: {"total_ms": summary([r["total"] for r in runs[k]]),
            "per_call_ms": summary([statistics.median(r["calls"]) for r in runs[k]]),
            "open_ms": summary([r["open"] for r in runs[k]]),
            "calls_ms_median": [round(statistics.median(r["calls"][j] for r in runs[k]), 3) for j in range(n)],
            "verified_aggregates": got[k]} for k, _ in legs}
    if args.trace_calls:  # the library's own events around every launch (serialises nothing; a run of its own leg by leg)
        result["kernels_ms_per_duty"] = {}
        for k, fn in legs:
            if k == "c":
                continue
            _chk(L, L.hbls_timing(1))
            for _ in range(args.trace_calls):
                fn()
            kern = {}
            for name, ms in _lib.timing_read(L, 1 << 18):
                kern[name] = kern.get(name, 0.0) + ms / args.trace_calls
            _chk(L, L.hbls_timing(0))
            result["kernels_ms_per_duty"][k] = {name: round(ms, 3) for name, ms in sorted(kern.items())}
    for h in clusters.values():
        _chk(L, L.hbls_cluster_close(h))
    merge_sections(result, args)
    print(json.dumps(result), flush=True)
    write(result, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
