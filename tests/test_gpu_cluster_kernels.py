"""The kernels of the cluster handles on the GPU, one launcher at a time, through the device harness
tests/native/clusterdev.hip (which compiles the product's charon_amd/csrc/cluster.hip): k_cluster_keys
on explicit words against a Python restatement of include/hipbls.h, exactly, and k_cluster_wide's 15
table points per key against the oracle's multiples, in the order ec28.h g1_wide_build documents.
Every output array carries sentinel entries behind it.
"""
import ctypes

import numpy as np
import pytest

from oracle import bls12381 as B

pytestmark = pytest.mark.gpu

NO_KEY = 0xFFFFFFFF  # cluster.h CLUSTER_NO_KEY; also ec28.h KEY_WIDE_NONE
BAD_PUBKEY = 1
PAD = 8
S8, S32 = 0xA5, 0xA5A5A5A5
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
LAM = (-B.X_PARAM ** 2) % B.R  # phi(P) = [lambda] P on G1 (rlc.h)


@pytest.fixture(scope="module")
def D(hipbls):
    from gpu_helpers import harness
    lib = harness.load("clusterdev")
    I, V, U32 = ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32
    lib.cd_keys.argtypes = [I, V, V, U32, U32, U32, U32, U32, V, V, I, V, V, V]
    lib.cd_wide.argtypes = [I, V, V, I, V, V]
    return lib


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


# ---------------------------------------------------------------------------------------------
# k_cluster_keys
# ---------------------------------------------------------------------------------------------
GROUP_BASE, N_GROUPS, N_SHARES = 5, 3, 4
N_KEYS = N_GROUPS * (1 + N_SHARES)
BAD_KEY, INF_KEY = 7, 11  # (group 6, share 2) has status 1; (group 7, share 1) is at infinity


def cluster_key(group, share_idx, dv):
    if not GROUP_BASE <= group < GROUP_BASE + N_GROUPS:
        return NO_KEY
    if not (0 if dv else 1) <= share_idx <= N_SHARES:
        return NO_KEY
    return (group - GROUP_BASE) * (1 + N_SHARES) + share_idx


@pytest.fixture(scope="module")
def table(D):
    """3 groups x (1 + 4) recognisable entries (word j of key k is 1000 (k + 1) + j; the infinity flag is
    the first word of the entry's last 16 bytes), one with status 1 and one at infinity"""
    words = D.cd_entry_bytes() // 4
    assert D.cd_entry_bytes() % 16 == 0
    ent = np.array([[1000 * (k + 1) + j for j in range(words)] for k in range(N_KEYS)], dtype=np.uint32)
    ent[:, words - 4:] = 0  # inf, pad[3]
    ent[INF_KEY, words - 4] = 1
    st = np.zeros(N_KEYS, np.uint8)
    st[BAD_KEY] = 1
    return ent, st


def items(n, seed):
    """n (group, share) pairs: the edge values of every comparison mixed among good ones"""
    rng = np.random.default_rng(seed)
    gedge = [GROUP_BASE - 1, GROUP_BASE, GROUP_BASE + N_GROUPS - 1, GROUP_BASE + N_GROUPS, 0xFFFFFFFF, 0]
    sedge = [0, 1, N_SHARES, N_SHARES + 1, -1, 1 << 32, (1 << 32) + 1, I64_MIN, I64_MAX]
    g = rng.integers(GROUP_BASE, GROUP_BASE + N_GROUPS, n).astype(np.uint32)
    s = rng.integers(1, N_SHARES + 1, n).astype(np.int64)
    for i in range(n):
        r = rng.random()
        if r < 0.25:
            g[i] = gedge[int(rng.integers(len(gedge)))]
        elif r < 0.55:
            s[i] = sedge[int(rng.integers(len(sedge)))]
    if n >= 63:  # every edge at least once, and the two special keys
        for k, v in enumerate(gedge):
            g[k], s[k] = v, 1 + k % N_SHARES
        for k, v in enumerate(sedge):
            g[10 + k], s[10 + k] = GROUP_BASE + k % N_GROUPS, v
        g[30], s[30] = 6, 2
        g[31], s[31] = 7, 1
    return g, s


def model(ent, st, g, s, dv, tables):
    words = ent.shape[1]
    vpk, vst, went = np.zeros((len(g), words), np.uint32), np.zeros(len(g), np.uint8), np.zeros(len(g), np.uint32)
    for i in range(len(g)):
        k = cluster_key(int(g[i]), 0 if dv else int(s[i]), dv)
        if k == NO_KEY:
            vpk[i, words - 4] = 1  # the point at infinity
            vst[i] = BAD_PUBKEY
            went[i] = NO_KEY
        else:
            vpk[i] = ent[k]
            vst[i] = st[k]
            went[i] = k if tables and not st[k] and not ent[k, words - 4] else NO_KEY
    return vpk, vst, went


def run_keys(D, ent, st, g, s, dv, tables, with_went=True):
    n, words = len(g), ent.shape[1]
    vpk = np.full((n + PAD, words), S32, np.uint32)
    vst = np.full(n + PAD, S8, np.uint8)
    went = np.full(n + PAD, S32, np.uint32) if with_went else None
    g, s = np.ascontiguousarray(g, np.uint32), np.ascontiguousarray(s, np.int64)
    rc = D.cd_keys(n, _p(g), None if dv else _p(s), GROUP_BASE, N_GROUPS, N_SHARES, N_KEYS, int(tables), _p(ent), _p(st), PAD,
                   _p(vpk), _p(vst), _p(went))
    assert rc == 0
    assert (vpk[n:] == S32).all() and (vst[n:] == S8).all(), "sentinels behind vpk / vpkst"
    if with_went:
        assert (went[n:] == S32).all(), "sentinel behind ent"
    return vpk[:n], vst[:n], went[:n] if with_went else None


@pytest.mark.parametrize("dv", [False, True], ids=["partials", "dv-keys"])
@pytest.mark.parametrize("tables", [True, False], ids=["tables", "no-tables"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_cluster_keys(D, table, n, tables, dv):
    ent, st = table
    g, s = items(n, 100 + n)
    want = model(ent, st, g, s, dv, tables)
    got = run_keys(D, ent, st, g, s, dv, tables)
    for name, a, b in zip(("vpk", "vpkst", "ent"), got, want):
        assert np.array_equal(a, b), name
    if not tables:
        assert (got[2] == NO_KEY).all()
    if n >= 63 and not dv:  # the cases are what they claim to be
        assert got[1][30] == 1 and got[2][30] == NO_KEY and np.array_equal(got[0][30], ent[BAD_KEY])
        assert got[1][31] == 0 and got[2][31] == NO_KEY and got[0][31, -4] == 1
        assert (want[1] == BAD_PUBKEY).sum() > 10 and (want[1] == 0).sum() > 10
        if tables:
            assert (got[2] != NO_KEY).sum() > 10
    if dv and n >= 63:  # share indices are not read: every item of a group of the shard gets its DV key
        inside = (g >= GROUP_BASE) & (g < GROUP_BASE + N_GROUPS)
        assert np.array_equal(got[0][inside], ent[(g[inside] - GROUP_BASE) * (1 + N_SHARES)])
        assert (got[1][~inside] == BAD_PUBKEY).all()


def test_cluster_keys_without_entry_numbers(D, table):
    """ent null (a cluster without ladder tables): the entries and statuses alone"""
    ent, st = table
    g, s = items(65, 7)
    want = model(ent, st, g, s, False, False)
    got = run_keys(D, ent, st, g, s, False, False, with_went=False)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---------------------------------------------------------------------------------------------
# k_cluster_wide
# ---------------------------------------------------------------------------------------------
def wide_points(s):
    """ec28.h: T[d - 1] = [d0] P + [d1] 2^16 P + [d2] phi(P) + [d3] 2^16 phi(P), d = d0 + 2 d1 + 4 d2 + 8 d3,
    for P = [s] G: compressed multiples of the generator"""
    out = []
    for d in range(1, 16):
        k = ((d & 1) + ((d >> 1) & 1) * (1 << 16) + (((d >> 2) & 1) + ((d >> 3) & 1) * (1 << 16)) * LAM) * s % B.R
        out.append(B.g1_compress(B.g1_mul(B.G1_GEN, k)))
    return out


WIDE_SCALARS = [1, 0x1234567 * 0x89ABCDEF % B.R, B.R - 5, 424242]
WIDE_STATUS = [0, 0, 0, 1]  # the last key has a bad status: skipped, its slots untouched


def wide_child():
    """Run as a program: cd_wide on the four keys in this process, its arrays to stdout as one JSON line."""
    import json
    from charon_amd.build import build_clusterdev
    lib = ctypes.CDLL(build_clusterdev(verbose=False))
    lib.cd_wide.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    st = np.array(WIDE_STATUS, np.uint8)
    pks = np.frombuffer(b"".join(B.g1_compress(B.g1_mul(B.G1_GEN, s)) for s in WIDE_SCALARS), np.uint8).copy()
    n, wb = len(WIDE_SCALARS), lib.cd_wide_bytes()
    wide = np.full(((15 * n + PAD), wb), S8, np.uint8)
    out = np.full((15 * n, 48), S8, np.uint8)
    rc = lib.cd_wide(n, _p(pks), _p(st), PAD, _p(wide), _p(out))
    print(json.dumps(dict(rc=rc, wb=wb, wide=wide.tobytes().hex(), out=out.tobytes().hex())))


def test_cluster_wide(D):
    """In a child process (this file run as a program), which ends with the call: k_cluster_wide keeps 3 096 B
    per lane in private memory, and the runtime reserves scratch per hardware queue for the largest kernel
    the queue has run.  The suite's process sits at the device's reservations with nothing to spare
    (tests/test_gpu_duty_first.py has the account), so this launcher adds no reservation to it.  A precaution,
    not a proven remedy: DESIGN.md section 4 "Cluster handles" says what was and was not seen."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "wide-child"], cwd=root, capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, GPU_MAX_HW_QUEUES="4", PYTHONPATH=root))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert got["rc"] == 0
    scal, n, wb = WIDE_SCALARS, len(WIDE_SCALARS), got["wb"]
    assert wb == D.cd_wide_bytes()
    wide = np.frombuffer(bytes.fromhex(got["wide"]), np.uint8).reshape(15 * n + PAD, wb)
    out = np.frombuffer(bytes.fromhex(got["out"]), np.uint8).reshape(15 * n, 48)
    assert (wide[15 * n:] == S8).all(), "sentinel behind the tables"
    assert (wide[15 * 3:15 * 4] == S8).all(), "the bad key's slots are untouched"
    for i in range(3):
        assert (wide[15 * i:15 * (i + 1)] != S8).any(axis=1).all(), "every slot of a good key is written"
        assert [bytes(out[15 * i + d]) for d in range(15)] == wide_points(scal[i]), f"key {i}"


if __name__ == "__main__":
    import sys
    assert sys.argv[1:] == ["wide-child"], sys.argv
    import torch  # noqa: F401 -- PyTorch's HIP runtime first, as tests/conftest.py loads it
    wide_child()
