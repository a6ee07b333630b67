"""The cluster verifies against the routes that send the keys, on the same lock, on one GPU in one run.

    python tools/cluster_verify_bench.py [--out profiles/cluster_verify_bench.json] [--runs 5] [--validators V]

The C3 lock: 100 k validators x 11 keys (the DV key and 10 pubshares), derived on the GPU from the synthetic
cluster's secrets (bench.py's cluster).  One synchronised call at a time, the routes alternating, medians
with the spread (max - min) reported:
  the lock aggregate (cluster/lock.go:185): one signature of every share secret over one hash
    bytes    hbls_verify_aggregate_batch over the V n compressed pubshares -- the existing route, which this
             commit does not change: it is the parent's too
    cluster  hbls_cluster_verify_aggregate (every share, no DV key) on the open cluster
  the registrations (lock.go:235-281): V verifications under the DV keys over V distinct messages
    bytes cold / cached   hbls_verify_batch with the DV keys' bytes, the host public-key cache empty / holding
                          them (hbls_pubkey_cache_add)
    cluster / cluster tables   hbls_cluster_verify_batch on clusters without / with ladder tables
and, from one more call of each under hbls_timing, the library's own kernel times.  A route is called
faster only where the medians differ by more than the larger of the two spreads.
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


def summary(xs):
    return {"median": round(statistics.median(xs), 3), "runs": [round(x, 3) for x in xs], "spread": round(max(xs) - min(xs), 3)}


def compare(a, b):
    """which of two summaries is faster, by the rule of the docstring"""
    d, bound = a["median"] - b["median"], max(a["spread"], b["spread"])
    return {"difference_ms": round(d, 3), "larger_spread_ms": bound,
            "verdict": "within the spread" if abs(d) <= bound else ("second faster" if d > 0 else "first faster")}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_verify_bench.json"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--validators", type=int, default=0, help="override the lock's size (smoke runs)")
    args = ap.parse_args(argv)

    import torch

    import bench
    from bench import _chk, _p
    from charon_amd import _lib, synth
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    wl = bench.WORKLOADS["c3"]
    V, n, t = args.validators or wl["validators"], wl["n"], wl["t"]
    cl = synth.make_cluster(V, n, t, first_validator=0, n_msgs=64, distinct_messages=False)
    share_sks = np.frombuffer(b"".join(cl.share_sks), dtype=np.uint8).copy()
    root_sks = np.frombuffer(b"".join(cl.root_sks), dtype=np.uint8).copy()
    sks = np.concatenate([share_sks, root_sks])
    keys, st = np.zeros((V * n + V) * 48, np.uint8), np.zeros(V * n + V, np.uint8)
    _chk(L, L.hbls_secret_to_public_key_batch(_p(sks), V * n + V, _p(keys), _p(st)))
    assert not st.any(), "key derivation failed"
    pubshares, dv_pks = keys[:V * n * 48].copy(), keys[V * n * 48:].copy()

    def sign(secrets, count, msgs, off, length):
        out, sst = np.zeros(96 * count, np.uint8), np.zeros(count, np.uint8)
        _chk(L, L.hbls_sign_batch(_p(secrets), _p(msgs), _p(off), _p(length), count, _p(out), _p(sst)))
        assert not sst.any()
        return out

    # the lock aggregate: every share secret signs the hash; one aggregate
    lock_hash = np.frombuffer(bytes(range(32)), np.uint8).copy()
    part = sign(share_sks, V * n, lock_hash, np.zeros(V * n, np.uint64), np.full(V * n, 32, np.uint32))
    agg, ast = np.zeros(96, np.uint8), np.zeros(1, np.uint8)
    _chk(L, L.hbls_aggregate_batch(_p(part), _p(np.array([0, V * n], np.uint32)), 1, _p(agg), _p(ast)))
    assert not ast.any()
    del part
    # the registrations: validator v's DV secret signs message v
    reg_msgs = np.zeros((V, 32), np.uint8)
    reg_msgs[:, :8] = np.arange(V, dtype=np.uint64).view(np.uint8).reshape(V, 8)
    reg_msgs[:, 31] = 0x7E
    reg_msgs = reg_msgs.reshape(-1)
    reg_off, reg_len = (np.arange(V, dtype=np.uint64) * 32), np.full(V, 32, np.uint32)
    reg_sigs = sign(root_sks, V, reg_msgs, reg_off, reg_len)

    def open_cluster(tables):
        kst, h = np.zeros(V * (1 + n), np.uint8), ctypes.c_uint64(0)
        _chk(L, L.hbls_cluster_open(_p(dv_pks), _p(pubshares), V, n, tables, _p(kst), ctypes.byref(h)))
        assert not kst.any()
        return h.value

    def timed(call):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        call()
        return (time.perf_counter() - t0) * 1e3

    goff, one_off, one_len = np.array([0, V * n], np.uint32), np.zeros(1, np.uint64), np.full(1, 32, np.uint32)
    status1, statusV = np.zeros(1, np.uint8), np.zeros(V, np.uint8)
    all_shares = (1 << n) - 1
    group, key0 = np.arange(V, dtype=np.uint32), np.zeros(V, np.int64)

    def agg_bytes():
        status1[:] = 9
        _chk(L, L.hbls_verify_aggregate_batch(_p(pubshares), _p(goff), _p(agg), _p(lock_hash), _p(one_off), _p(one_len), 1,
                                              _p(status1)))
        assert status1[0] == 0

    def agg_cluster(h):
        status1[:] = 9
        _chk(L, L.hbls_cluster_verify_aggregate(h, all_shares, 0, _p(agg), _p(lock_hash), 32, _p(status1)))
        assert status1[0] == 0

    def reg_bytes():
        statusV[:] = 9
        _chk(L, L.hbls_verify_batch(_p(dv_pks), _p(reg_sigs), _p(reg_msgs), _p(reg_off), _p(reg_len), V, _p(statusV)))
        assert not statusV.any()

    def reg_cluster(h):
        statusV[:] = 9
        _chk(L, L.hbls_cluster_verify_batch(h, _p(group), _p(key0), _p(reg_sigs), _p(reg_msgs), _p(reg_off), _p(reg_len), V,
                                            _p(statusV)))
        assert not statusV.any()

    def kernels(call):
        _chk(L, L.hbls_timing(1))
        call()
        kern = {}
        for name, ms in _lib.timing_read(L):
            kern[name] = round(kern.get(name, 0.0) + ms, 3)
        _chk(L, L.hbls_timing(0))
        return kern

    h0, h1 = open_cluster(0), open_cluster(1)
    _chk(L, L.hbls_pubkey_cache_clear())
    for call in (agg_bytes, lambda: agg_cluster(h0), reg_bytes, lambda: reg_cluster(h0), lambda: reg_cluster(h1)):
        call()  # warm-up: workspaces, staging, the kernels' code objects
    t_agg = {"bytes": [], "cluster": []}
    t_reg = {"bytes_cold": [], "bytes_cached": [], "cluster": [], "cluster_tables": []}
    for _ in range(args.runs):
        t_agg["bytes"].append(timed(agg_bytes))
        t_agg["cluster"].append(timed(lambda: agg_cluster(h0)))
        t_reg["bytes_cold"].append(timed(reg_bytes))
        t_reg["cluster"].append(timed(lambda: reg_cluster(h0)))
        t_reg["cluster_tables"].append(timed(lambda: reg_cluster(h1)))
        _chk(L, L.hbls_pubkey_cache_add(_p(dv_pks), V))
        t_reg["bytes_cached"].append(timed(reg_bytes))
        _chk(L, L.hbls_pubkey_cache_clear())
    kern = {"aggregate_bytes": kernels(agg_bytes), "aggregate_cluster": kernels(lambda: agg_cluster(h0)),
            "registrations_bytes_cold": kernels(reg_bytes), "registrations_cluster": kernels(lambda: reg_cluster(h0)),
            "registrations_cluster_tables": kernels(lambda: reg_cluster(h1))}
    vs = (ctypes.c_uint64 * 5)()
    _chk(L, L.hbls_cluster_verify_stats(h0, vs, 5))
    for h in (h0, h1):
        _chk(L, L.hbls_cluster_close(h))

    s_agg = {k: summary(v) for k, v in t_agg.items()}
    s_reg = {k: summary(v) for k, v in t_reg.items()}
    result = {
        "tool": "tools/cluster_verify_bench.py", "runs": args.runs, "library": L.hbls_build_id().decode(),
        "device": torch.cuda.get_device_name(0), "workload": "c3 lock", "validators": V, "n": n,
        "pubshares": V * n, "lock_aggregate_ms": s_agg, "registrations_ms": s_reg,
        "lock_aggregate_bytes_vs_cluster": compare(s_agg["bytes"], s_agg["cluster"]),
        "registrations_bytes_cold_vs_cluster": compare(s_reg["bytes_cold"], s_reg["cluster"]),
        "registrations_bytes_cached_vs_cluster": compare(s_reg["bytes_cached"], s_reg["cluster"]),
        "registrations_cluster_vs_cluster_tables": compare(s_reg["cluster"], s_reg["cluster_tables"]),
        "kernels_ms": kern, "cluster_verify_stats_no_tables": [int(x) for x in vs],
        "note": "wall times of one blocking call each, host buffers, the routes alternating within each run; the bytes "
                "routes upload 48 B per key, the cluster routes 12 B per item (verify) or nothing per key (aggregate)",
    }
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
