"""The calls of tests/test_gpu_hash.py into the hash harness (tests/native/devblocks_h2c.hip,
devblocks_h2c_std.hip) and into hbls_hash_to_g2_device -- and, run as a program, a child process that
makes the scratch-heavy ones of them.

Why a child.  The runtime reserves scratch per hardware queue for the largest kernel the queue has run:
bytes per lane x 64 lanes x (2 waves x 4 SIMDs x 256 CUs), the sizing hash.hip's header gives; its data
point is that two queues of the 21 KB inlined hashing (2 x 2.75 GB) exhausted the device's scratch.
The standard-convention kernels here (the harness's std unit, and hash.hip's k_hash_to_g2 /
k_hash_to_g2_1 behind HBLS_HASH_SPLIT=0) keep their building blocks as separate functions and need
3.4 - 3.6 KB per lane by the compiler's resource report: about 0.47 GB on the queue that runs one.
tests/test_gpu_hash.py runs before tests/test_gpu_multi.py in the suite's process, and that file's
hbls_debug_split(3) opens 48 library streams (dev_create: 16 per context) whose kernels need 1.1 - 1.5 KB
per lane, 0.14 - 0.2 GB a queue.  In a run of the whole tests/ directory, tests/test_bench_launcher.py
imports bench.py before HIP starts, which sets GPU_MAX_HW_QUEUES=32, so those streams fill 32 queues:
4.6 - 6.4 GB, at the level of that data point with nothing to spare.  So this file adds no half
gigabyte of its own to that process: the standard-convention calls are made here, in a process that
ends with them -- a job file in (JSON: calls by name), the raw output words out (one JSON line) -- and
the in-process calls stay on the null stream with the product's default kernels (at most 1.4 KB per
lane).  Only the device calls are made here; the reference and every comparison stay with the test."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

U32P = ctypes.POINTER(ctypes.c_uint32)
U64P = ctypes.POINTER(ctypes.c_uint64)
U8P = ctypes.POINTER(ctypes.c_uint8)
I32P = ctypes.POINTER(ctypes.c_int)
SZ = ctypes.c_size_t

L_OPS = {n: i for i, n in enumerate("pow_P_MINUS_2 pow_SQRT pow_P_M3_4 pow_LEGENDRE fp_sqrt fp_is_square f2_sqrt f2_sgn0 "
                                    "f2_lex from_mont from_be512 xmd_bi sswu_iso".split())}
S_MAP, S_CLEAR, S_PSI, S_PSI2 = range(4)
M_FIELD, M_HASH = 0, 1
ST_FIELD, ST_MAP, ST_CLEAR1, ST_CLEAR1B, ST_CLEAR2, ST_CLEAR3 = range(6)
MAX_CASES = 256
GPU_ERRORS = (-5, -6)  # devblocks.h DB_E_LAUNCH, DB_E_SYNC


def u32(a):
    return np.ascontiguousarray(np.array(a, dtype=np.uint64).astype(np.uint32))


def pack_messages(msgs):
    """one buffer, the messages back to back (unaligned offsets): (bytes, offsets, lengths)"""
    off, at = [], 0
    for m in msgs:
        off.append(at)
        at += len(m)
    return b"".join(msgs), off, [len(m) for m in msgs]


def _msg_args(msgs):
    buf, off, ln = pack_messages(msgs)
    b = np.frombuffer(buf + b"\0", dtype=np.uint8).copy()  # one byte past the last message: never empty
    return b, len(b), np.array(off, dtype=np.uint64), np.array(ln, dtype=np.uint32)  # the whole buffer is uploaded


class Hash:
    """check(rc, what) is called with every entry point's return code"""

    def __init__(self, lib, check):
        self.lib, self.check = lib, check
        lib.db_h2c_leaf.argtypes = [ctypes.c_int, ctypes.c_int, U32P, U32P, I32P]
        lib.db_h2c_b0.argtypes = [ctypes.c_int, U8P, SZ, U64P, U32P, U32P]
        lib.db_h2c_stages.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, U8P, SZ, U64P, U32P, U32P,
                                      U32P, U32P, U32P]
        lib.db_h2c_std.argtypes = [ctypes.c_int, ctypes.c_int, U32P, U32P]
        lib.db_h2c_std_msg.argtypes = [ctypes.c_int, ctypes.c_int, U8P, SZ, U64P, U32P, U32P]
        assert lib.db_h2c_max() == MAX_CASES

    def leaf(self, op, rows):
        """rows: n <= 256 cases of up to 24 words -> ([72 output words], [flag]), one launch"""
        n = len(rows)
        assert 1 <= n <= MAX_CASES
        inp = u32([list(r) + [0] * (24 - len(r)) for r in rows])
        out, fl = np.zeros((n, 72), dtype=np.uint32), np.zeros(n, dtype=np.int32)
        self.check(self.lib.db_h2c_leaf(L_OPS[op], n, inp.ctypes.data_as(U32P), out.ctypes.data_as(U32P),
                                        fl.ctypes.data_as(I32P)), f"db_h2c_leaf({op})")
        return [[int(v) for v in row] for row in out], [int(v) for v in fl]

    def b0(self, msgs):
        b, nbytes, off, ln = _msg_args(msgs)
        out = np.zeros((len(msgs), 8), dtype=np.uint32)
        self.check(self.lib.db_h2c_b0(len(msgs), b.ctypes.data_as(U8P), nbytes, off.ctypes.data_as(U64P),
                                      ln.ctypes.data_as(U32P), out.ctypes.data_as(U32P)), "db_h2c_b0")
        return [b"".join(int(w).to_bytes(4, "big") for w in row) for row in out]

    def stages(self, first, last, pair, msgs=None, inp=None):
        """-> per message (u: 48 words, q: 216 words, h: 52 words)"""
        n = len(msgs) if msgs is not None else len(inp)
        assert 1 <= n <= MAX_CASES
        u, q, h = (np.zeros((n, k), dtype=np.uint32) for k in (48, 216, 52))
        if msgs is not None:
            b, nbytes, off, ln = _msg_args(msgs)
            rc = self.lib.db_h2c_stages(first, last, pair, n, b.ctypes.data_as(U8P), nbytes, off.ctypes.data_as(U64P),
                                        ln.ctypes.data_as(U32P), None, u.ctypes.data_as(U32P), q.ctypes.data_as(U32P),
                                        h.ctypes.data_as(U32P))
        else:
            a = u32(inp)
            assert a.shape == (n, 48 if first == ST_MAP else 144)
            rc = self.lib.db_h2c_stages(first, last, pair, n, None, 0, None, None, a.ctypes.data_as(U32P),
                                        u.ctypes.data_as(U32P), q.ctypes.data_as(U32P), h.ctypes.data_as(U32P))
        self.check(rc, f"db_h2c_stages({first}, {last}, pair={pair})")
        return u, q, h

    def std(self, op, rows):
        """rows: n cases of up to 144 words -> [72 words]"""
        n = len(rows)
        assert 1 <= n <= MAX_CASES
        inp = u32([list(r) + [0] * (144 - len(r)) for r in rows])
        out = np.zeros((n, 72), dtype=np.uint32)
        self.check(self.lib.db_h2c_std(op, n, inp.ctypes.data_as(U32P), out.ctypes.data_as(U32P)), f"db_h2c_std({op})")
        return [[int(v) for v in row] for row in out]

    def std_msg(self, op, msgs):
        b, nbytes, off, ln = _msg_args(msgs)
        out = np.zeros((len(msgs), 72), dtype=np.uint32)
        self.check(self.lib.db_h2c_std_msg(op, len(msgs), b.ctypes.data_as(U8P), nbytes, off.ctypes.data_as(U64P),
                                           ln.ctypes.data_as(U32P), out.ctypes.data_as(U32P)), f"db_h2c_std_msg({op})")
        return [[int(v) for v in row] for row in out]


def tune(L, name, value):
    """hbls_tune: set a kernel-path knob by name, return the previous value"""
    prev = ctypes.c_size_t(0)
    assert L.hbls_tune(name.encode(), value, ctypes.byref(prev)) == 0, L.hbls_last_error().decode()
    return prev.value


def library_hash(L, msgs, knobs):
    """hbls_hash_to_g2_device over msgs packed back to back, on the null stream (no further hardware
    queue), with the knobs that choose the kernel path set for the call -> [52 HmEntry words]"""
    import torch
    dev = torch.device("cuda", 0)
    buf, off, ln = pack_messages(msgs)
    n, E = len(msgs), L.hbls_hm_entry_bytes()
    dm = torch.from_numpy(np.frombuffer(buf + b"\0", dtype=np.uint8).copy()).to(dev)
    doff = torch.from_numpy(np.array(off, dtype=np.uint64).view(np.int64)).to(dev)
    dln = torch.from_numpy(np.array(ln, dtype=np.uint32).view(np.int32)).to(dev)
    hm = torch.zeros(n * E, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    prev = {}
    try:
        for k, v in knobs.items():
            prev[k] = tune(L, k, v)
        rc = L.hbls_hash_to_g2_device(ctypes.c_void_p(dm.data_ptr()), ctypes.c_void_p(doff.data_ptr()),
                                      ctypes.c_void_p(dln.data_ptr()), n, ctypes.c_void_p(hm.data_ptr()), None)
        assert rc == 0, L.hbls_last_error().decode()
        torch.cuda.synchronize(dev)
    finally:
        for k, v in prev.items():
            tune(L, k, v)
    rows = hm.cpu().numpy().reshape(n, E)[:, :208].copy().view(np.uint32)
    return [[int(v) for v in row] for row in rows]


def load_library():
    from charon_amd import _lib, tbls
    tbls.HIPBLS()  # initialises the library on its devices
    return _lib.load_library()


def run_child(jobs, timeout=240):
    """the calls `jobs` ({name: call}) made in a child process -> {name: output rows}; a call is
    {"kind": "std", "op", "rows"}, {"kind": "std_msg", "op", "msgs": [hex]} or
    {"kind": "library", "knobs", "msgs": [hex]}.  Returns (return code, results or the child's output);
    the return code is 124 if the child ran into the time limit."""
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "jobs.json")
        with open(path, "w") as f:
            json.dump(jobs, f)
        try:
            p = subprocess.run([sys.executable, "-u", os.path.abspath(__file__), path], capture_output=True, text=True,
                               timeout=timeout)
        except subprocess.TimeoutExpired as e:  # the child is killed: a hang
            return 124, (str(e.stdout)[-2000:], str(e.stderr)[-2000:])
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    if p.returncode != 0 or not lines:
        return p.returncode or 1, (p.stdout[-2000:], p.stderr[-2000:])
    return 0, json.loads(lines[-1])


def gpu_trouble(rc):
    """a child's return code that means the card faulted, aborted or hung: the child's own 3 (a failed
    launch or synchronise), a signal (negative: abort -6, segmentation fault -11, ...), 134 / 139 (the
    same seen through a shell), 124 / 137 (a time limit)"""
    return rc < 0 or rc in (3, 124, 134, 137, 139)


def main(argv):
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (the HIP runtime first: charon_amd/_lib.py)
    from charon_amd import build
    with open(argv[1]) as f:
        jobs = json.load(f)

    def check(rc, what):
        if rc != 0:
            print(f"{what} returned {rc}", flush=True)
            sys.exit(3 if rc in GPU_ERRORS else 1)  # nothing more is started on the card
    path = build.devblocks_path(build.DEVBLOCKS_HASH)
    assert build.embedded_devblocks_id(path) == build.devblocks_build_id(build.DEVBLOCKS_HASH), "stale hash harness"
    hh, L, out = Hash(ctypes.CDLL(path), check), None, {}
    for name, job in jobs.items():
        if job["kind"] == "std":
            out[name] = hh.std(job["op"], job["rows"])
        elif job["kind"] == "std_msg":
            out[name] = hh.std_msg(job["op"], [bytes.fromhex(m) for m in job["msgs"]])
        else:
            L = L or load_library()
            out[name] = library_hash(L, [bytes.fromhex(m) for m in job["msgs"]], job["knobs"])
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
