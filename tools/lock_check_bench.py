"""hbls_cluster_check against hbls_cluster_open on the same lock, on one GPU in one run.

    python tools/lock_check_bench.py [--out profiles/lock_check_bench.json] [--runs 5] [--validators V]

The C3 lock: 100 k validators x 11 keys (the DV key and 10 pubshares), threshold 7, derived on the GPU from
the synthetic cluster's share secrets (bench.py's cluster, without its signatures).  One synchronised call
at a time, medians with the spread (max - min) reported:
  open   hbls_cluster_open without ladder tables -- the parent commit's code, and the only yardstick there
         is: neither the reference nor the parent has the check
  check  hbls_cluster_check at the lock's threshold on that cluster, every row asserted HBLS_OK
and, from one more call of each under hbls_timing, the library's own kernel times.  The profile states the
check's Fp products per validator by count (lockcheck.hip: per window 6 doublings of 7 products and 19 mixed
additions of 11, the first addition into the identity being free) beside the open's, and the measured ratio
beside the counted one.
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

DBL_PRODUCTS, MADD_PRODUCTS = 7, 11  # ec28.h g1l_dbl; g1l_madd with g1l_add_tail
OPEN_PRODUCTS_PER_VALIDATOR = 24_000  # 11 square roots and 126-step membership ladders, by count


def check_products_per_validator(n, t):
    """by count: per window one doubling per bit plane and one mixed addition per set coefficient bit but the first"""
    import math
    c = [math.comb(t, i) for i in range(t + 1)]
    bits, adds = max(c).bit_length(), sum(bin(x).count("1") for x in c)
    return (n - t + 1) * (bits * DBL_PRODUCTS + (adds - 1) * MADD_PRODUCTS)


def summary(xs):
    return {"median": round(statistics.median(xs), 3), "runs": [round(x, 3) for x in xs], "spread": round(max(xs) - min(xs), 3)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lock_check_bench.json"))
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
    sks = np.frombuffer(b"".join(cl.share_sks) + b"".join(cl.root_sks), dtype=np.uint8).copy()
    keys, st = np.zeros((V * n + V) * 48, np.uint8), np.zeros(V * n + V, np.uint8)
    _chk(L, L.hbls_secret_to_public_key_batch(_p(sks), V * n + V, _p(keys), _p(st)))
    assert not st.any(), "key derivation failed"
    pubshares, dv_pks = keys[:V * n * 48].copy(), keys[V * n * 48:].copy()

    def kernels(call):
        _chk(L, L.hbls_timing(1))
        call()
        kern = {}
        for name, ms in _lib.timing_read(L):
            kern[name] = round(kern.get(name, 0.0) + ms, 3)
        _chk(L, L.hbls_timing(0))
        return kern

    def open_cluster():
        """-> (handle, wall ms)"""
        kst = np.zeros(V * (1 + n), np.uint8)
        h = ctypes.c_uint64(0)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        _chk(L, L.hbls_cluster_open(_p(dv_pks), _p(pubshares), V, n, 0, _p(kst), ctypes.byref(h)))
        wall = (time.perf_counter() - t0) * 1e3
        assert not kst.any()
        return h.value, wall

    row_status, row_windows, n_bad = np.zeros(V, np.uint8), np.zeros(V, np.uint64), ctypes.c_size_t(0)

    def check(h, threshold=t):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        _chk(L, L.hbls_cluster_check(h, threshold, _p(row_status), _p(row_windows), ctypes.byref(n_bad)))
        return (time.perf_counter() - t0) * 1e3

    h, _ = open_cluster()  # warm-up: workspaces, the kernels' code objects
    check(h)
    assert n_bad.value == 0 and not row_status.any() and not row_windows.any(), "the synthetic lock is consistent"
    check(h, t - 1)
    assert n_bad.value == V and (row_status == 3).all(), "degree t - 1 rows fail at t - 1"
    _chk(L, L.hbls_cluster_close(h))
    opens, checks = [], []
    for _ in range(args.runs):
        h, ms = open_cluster()
        opens.append(ms)
        checks.append(check(h))
        assert n_bad.value == 0
        _chk(L, L.hbls_cluster_close(h))
    hs = []
    open_kern = kernels(lambda: hs.append(open_cluster()[0]))
    check_kern = kernels(lambda: check(hs[0]))
    _chk(L, L.hbls_cluster_close(hs[0]))

    counted = check_products_per_validator(n, t)
    result = {
        "tool": "tools/lock_check_bench.py", "runs": args.runs, "library": L.hbls_build_id().decode(),
        "device": torch.cuda.get_device_name(0), "workload": "c3 lock", "validators": V, "n": n, "t": t,
        "keys": V * (1 + n), "windows_per_validator": n - t + 1,
        "open_no_tables_ms": summary(opens), "check_ms": summary(checks),
        "open_kernels_ms": open_kern, "check_kernels_ms": check_kern,
        "fp_products_per_validator_by_count": {"check": counted, "open": OPEN_PRODUCTS_PER_VALIDATOR,
                                               "ratio": round(counted / OPEN_PRODUCTS_PER_VALIDATOR, 4)},
        "measured_ratio_check_over_open": round(statistics.median(checks) / statistics.median(opens), 4),
        "note": "wall times of one blocking call each, host buffers; the open uploads 48 B per key and returns one status "
                "byte per key, the check returns 9 B per validator",
    }
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
