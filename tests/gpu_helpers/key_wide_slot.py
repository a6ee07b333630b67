"""Shared by tests/test_gpu_key_wide.py and its child process: the slot of 64 validators of a
10-operator threshold-7 cluster over distinct messages, the knobs that make the slot-wide check and
the chunked combination run at that size, and the ladder tables' counters.  The slot itself runs
through key_learn_slot.run_slots.  Run as a script it is the child of the HBLS_STATS test: two
calls from a cold cache, then one JSON line with the second call's counters."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import key_learn_slot as ks  # noqa: E402  (torch first, then the library)

from charon_amd import _lib  # noqa: E402

# 640 pubshares (ten waves of key lookups, 64 chunks of 10 items: one wave of k_rlc_msm) + 64 DV keys
WL = dict(validators=64, n=10, t=7, distinct=True, n_msgs=0)


def make_inputs(L, wl=None, rank=0):
    import bench
    wl = wl or WL
    return bench.setup_inputs(L, wl, wl["validators"], rank)


def set_knobs(L):
    """Batched final exponentiation from 2 groups, the slot-wide check from 1 item (which also
    clears the adaptive history), no adaptive skipping, chunks of 10 items at 640 items."""
    return (L.hbls_fe_batch(2), L.hbls_slot_msm(1), L.hbls_adaptive(0), L.hbls_rlc_lanes(64))


def restore_knobs(L, prev):
    L.hbls_fe_batch(prev[0])
    L.hbls_slot_msm(prev[1])
    L.hbls_adaptive(prev[2])
    L.hbls_rlc_lanes(prev[3])


def wide_stats(L):
    """Device 0's {built, wide_chunks, narrow_chunks, wide_items, narrow_items}, cumulative."""
    return _lib.key_wide_stats(L)[0]


def main():
    L = _lib.lib()
    set_knobs(L)
    d = make_inputs(L)
    first = ks.run_slots(L, d)[0]
    w1 = wide_stats(L)
    s1 = (ctypes.c_uint64 * 6)()
    assert L.hbls_stats(s1, 6) == 0, L.hbls_last_error()
    second = ks.run_slots(L, d)[0]
    w2 = wide_stats(L)
    s2 = (ctypes.c_uint64 * 6)()
    assert L.hbls_stats(s2, 6) == 0, L.hbls_last_error()
    print(json.dumps({"second_call_wide": {k: w2[k] - w1[k] for k in w1},
                      "second_call_stats": [int(s2[k] - s1[k]) for k in range(6)],
                      "equal": first == second,
                      "all_ok": not any(second[0]) and not any(second[1]) and not any(second[2]) and
                      second[3] == d["root_sigs"].tobytes()}))


if __name__ == "__main__":
    main()
