"""Generate tests/golden/cluster_traces.json: the kernel names the cluster calls enqueue, in order --
hbls_cluster_open without and with ladder tables, hbls_cluster_check, hbls_cluster_verify_batch (over
batch_items of tests/gpu_helpers/cluster_verify_cases.py, without and with ladder tables),
hbls_cluster_verify_aggregate with every share selected and with nothing selected, the adds of one
cluster duty up to its threshold (the last one fires every group), and the two verifies again on a
cluster opened under hbls_debug_split(2).  The lock is the 6-validator,
4-share one of tests/gpu_helpers/lock_check_cases.py; the recording is make_launch_traces.py's
(hbls_timing(1) / hbls_timing_read, one warm-up call, the second recorded, the knobs set and restored).

The fixture pins these launch sequences across changes that must not alter them.  Record it with the
library of the commit BEFORE such a change, never from the code under test: check that commit out into
a tree of its own, build it there, copy this file and what it imports from tests/ there if that tree
has none, and run it from that tree with --out naming this tree's cluster_traces.json.  The library's
build id goes into recorded_with.  test_launch_traces of tests/gpu_helpers/cluster_verify_cases.py runs
the same cases (CASES below) against the tree's library.  Needs the GPU.

    python tests/golden/make_cluster_traces.py [--out FILE]

A case opens the clusters it needs and closes them; a duty case opens a fresh duty for the warm-up and
another for the recording, and takes each through the same adds.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE, os.path.join(ROOT, "tests", "gpu_helpers")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402,F401  (the HIP runtime first: charon_amd/_lib.py)

import cluster_verify_cases as cv  # noqa: E402
import make_launch_traces as mk  # noqa: E402
from charon_amd import _lib  # noqa: E402
from lock_check_cases import N, T, V, make_lock  # noqa: E402

PATH = os.path.join(HERE, "cluster_traces.json")
KNOBS = dict(fe_batch=128, slot_msm=0, adaptive=0)
ALL_SHARES = (1 << N) - 1
# the two-shard traces: the shard threads race, so these are compared as sorted lists (the same
# kernels, each as often), as tests/test_gpu_select_trace.py compares select_host_split2
SORTED = {"cluster_verify_batch_split2", "cluster_verify_aggregate_split2"}


class Ctx:
    """The lock, its signatures, and the recording"""

    def __init__(self, L, hipbls, lock=None, signed=None):
        self.L, self.hipbls = L, hipbls
        self.lock = lock if lock is not None else make_lock(hipbls)
        self.signed = signed if signed is not None else cv.make_signed(hipbls, self.lock)
        self.items, self.want = cv.batch_items(self.signed)
        self.agg_msg = cv.M[2]
        self.agg_sig = cv.agg_sig(hipbls, self.lock, [(g, j) for g in range(V) for j in range(1, N + 1)], self.agg_msg)

    def cluster(self, tables):
        return cv.Cl(self.L, self.lock["dv"], self.lock["pub"], tables)

    def record(self, call):
        """The names of call()'s launches: one warm-up call, the second recorded (every call here is
        complete when it returns)."""
        call()
        return self.record_next(call)

    def record_next(self, call):
        L = self.L
        mk.chk(L, L.hbls_timing(1))
        try:
            call()
            return [name for name, _ in _lib.timing_read(L)]
        finally:
            mk.chk(L, L.hbls_timing(0))


def _open(cx):
    return {f"cluster_open_tables{tables}": cx.record(lambda: cx.cluster(tables).close()) for tables in (0, 1)}


def _check(cx):
    import lock_check_cases as lk
    cl = lk.Cl(cx.L, cx.lock, 1)
    try:
        def call():
            rc, st, _, n_bad = cl.check(T)
            assert rc == 0 and not any(st) and n_bad == 0
        return {"cluster_check": cx.record(call)}
    finally:
        cl.close()


def verify_call(cl, items, want):
    def call():
        rc, st = cl.verify(items)
        assert rc == 0 and st == want
    return call


def aggregate_call(cx, cl, mask, want):
    def call():
        assert cl.aggregate(mask, 0, cx.agg_sig, cx.agg_msg) == (0, want)
    return call


def _verify_batch(cx):
    out = {}
    for tables in (0, 1):
        cl = cx.cluster(tables)
        try:
            out[f"cluster_verify_batch_tables{tables}"] = cx.record(verify_call(cl, cx.items, cx.want))
        finally:
            cl.close()
    return out


def _verify_aggregate(cx):
    cl = cx.cluster(1)
    try:
        return {"cluster_verify_aggregate_all": cx.record(aggregate_call(cx, cl, ALL_SHARES, cv.OK)),
                "cluster_verify_aggregate_empty": cx.record(aggregate_call(cx, cl, 0, cv.NOT_VERIFIED))}
    finally:
        cl.close()


def _duty(cx):
    """Every validator's partials of share indices 1 .. T, one add per index: the last fires every group"""
    from charon_amd.tbls import Duty
    msgs = [bytes([0x40 + v]) * 32 for v in range(V)]
    sigs = [cx.hipbls.sign_batch([cx.lock["shares"][v][j - 1] for v in range(V)], msgs) for j in range(1, T + 1)]
    cl = cx.cluster(1)
    out = {}
    try:
        for recorded in (False, True):
            with Duty(cx.L, (), T, 16, cluster=(cl.h, V)) as du:
                for j in range(1, T + 1):
                    def call():
                        r = du.add(None, msgs, sigs[j - 1], list(range(V)), [j] * V)
                        assert not any(r.vstatus) and len(r.fired) == (V if j == T else 0)
                    if recorded:
                        out[f"cluster_duty_add_{j}"] = cx.record_next(call)
                    else:
                        call()
    finally:
        cl.close()
    return out


def _split2(cx):
    """The two verifies on a cluster opened over two contexts of device 0: three validators a shard"""
    L = cx.L
    mk.chk(L, L.hbls_debug_split(2))
    try:
        cl = cx.cluster(1)
        try:
            return {"cluster_verify_batch_split2": cx.record(verify_call(cl, cx.items, cx.want)),
                    "cluster_verify_aggregate_split2": cx.record(aggregate_call(cx, cl, ALL_SHARES, cv.OK))}
        finally:
            cl.close()
    finally:
        mk.chk(L, L.hbls_debug_split(1))


# ---- the cases: name -> function(cx) returning {trace name: [kernel names]} ----
CASES = {"open": _open, "check": _check, "verify_batch": _verify_batch, "verify_aggregate": _verify_aggregate,
         "duty": _duty, "split2": _split2}
# the traces each case records
TRACES = {
    "open": ["cluster_open_tables0", "cluster_open_tables1"],
    "check": ["cluster_check"],
    "verify_batch": ["cluster_verify_batch_tables0", "cluster_verify_batch_tables1"],
    "verify_aggregate": ["cluster_verify_aggregate_all", "cluster_verify_aggregate_empty"],
    "duty": [f"cluster_duty_add_{j}" for j in range(1, T + 1)],
    "split2": sorted(SORTED),
}


def run_cases(cx):
    """Every case's traces, under the knobs the fixture was recorded with"""
    traces = {}
    with mk.knobs(cx.L, **KNOBS):
        for name, run in CASES.items():
            got = run(cx)
            assert sorted(got) == sorted(TRACES[name]), name
            traces.update(got)
    return traces


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    out = argv[argv.index("--out") + 1] if "--out" in argv else PATH
    from charon_amd import tbls
    hipbls = tbls.HIPBLS()
    L = hipbls._L
    traces = run_cases(Ctx(L, hipbls))
    with open(out, "w") as f:
        json.dump({"recorded_with": L.hbls_build_id().decode(), "traces": traces}, f, indent=1)
    print("wrote", out, {k: len(v) for k, v in traces.items()})


if __name__ == "__main__":
    main()
