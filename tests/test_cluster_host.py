"""The key rule of a cluster handle on the CPU, through the g++ harness tests/native/clustercheck.cpp:
charon_amd/csrc/cluster.h cluster_key -- the one function cluster.hip's k_cluster_keys runs per item and
hipbls.hip counts hbls_cluster_stats with -- against a Python restatement of include/hipbls.h, over
seeded inputs and the edges of every comparison it makes.  And the binding: charon_amd/_lib.py declares
the four entry points with the header's argument counts.
"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_KEY = 0xFFFFFFFF
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def cluster_key(group, share_idx, group_base, n_groups, n_shares, dv=False):
    """include/hipbls.h: a partial has a key iff its group is one of the shard's and 1 <= share_idx <=
    n_shares (the DV key: share 0 allowed too); the key's number is row-major, 1 + n_shares per group."""
    if not group_base <= group < group_base + n_groups:
        return NO_KEY
    if not (0 if dv else 1) <= share_idx <= n_shares:
        return NO_KEY
    return (group - group_base) * (1 + n_shares) + share_idx


@pytest.fixture(scope="module")
def H():
    from gpu_helpers import harness
    lib = harness.load("clustercheck")
    V, SZ, U32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    lib.cc_no_key.restype = U32
    lib.cc_max_shares.restype = U32
    lib.cc_keys.argtypes = [V, V, SZ, U32, U32, U32, ctypes.c_int, V]
    lib.cc_keys.restype = None
    return lib


def run(H, group, share, group_base, n_groups, n_shares, dv):
    g, s = np.asarray(group, np.uint32), np.asarray(share, np.int64)
    out = np.full(len(g) + 1, 0x5A5A5A5A, np.uint32)
    H.cc_keys(g.ctypes.data, s.ctypes.data, len(g), group_base, n_groups, n_shares, int(dv), out.ctypes.data)
    assert out[len(g)] == 0x5A5A5A5A, "sentinel"
    return out[:len(g)].tolist()


def share_edges(n_shares):
    return [0, 1, n_shares, n_shares + 1, -1, 1 << 32, (1 << 32) + 1, I64_MIN, I64_MAX, (1 << 32) + n_shares,
            -(1 << 32) + 1, 2, n_shares - 1 if n_shares > 1 else 1]


def group_edges(group_base, n_groups):
    last = group_base + n_groups - 1
    return [(group_base - 1) & 0xFFFFFFFF, group_base, last & 0xFFFFFFFF, (last + 1) & 0xFFFFFFFF, 0xFFFFFFFF, 0,
            (group_base + n_groups // 2) & 0xFFFFFFFF]


def test_constants(H):
    assert H.cc_no_key() == NO_KEY
    assert H.cc_max_shares() == 64


@pytest.mark.parametrize("dv", [False, True])
@pytest.mark.parametrize("n_shares", [1, 4, 10, 64])
@pytest.mark.parametrize("group_base,n_groups", [(5, 3), (0, 1), (0, 7), (1000, 256), (7, 0), (0, 0), (0xFFFFFFF0, 15)])
def test_edges(H, group_base, n_groups, n_shares, dv):
    """Every share edge under every group edge: share 0, 1, n_shares, n_shares + 1, -1, 2^32, 2^32 + 1,
    INT64_MIN, INT64_MAX; group_base - 1, group_base, the last group, the one behind it, 0xffffffff; a
    shard with no groups."""
    groups, shares = [], []
    for g in group_edges(group_base, n_groups):
        for s in share_edges(n_shares):
            groups.append(g)
            shares.append(s)
    want = [cluster_key(g, s, group_base, n_groups, n_shares, dv) for g, s in zip(groups, shares)]
    got = run(H, groups, shares, group_base, n_groups, n_shares, dv)
    assert got == want
    if n_groups == 0:
        assert set(got) == {NO_KEY}
    else:  # the edges do hit keys, and both kinds of miss
        assert any(k != NO_KEY for k in got) and NO_KEY in got
        assert max(k for k in got if k != NO_KEY) == n_groups * (1 + n_shares) - 1  # the shard's last key


def test_truncation_is_never_a_key(H):
    """Values whose low 32 bits are a valid share index have no key: the comparison is on 64 bits."""
    n_shares = 10
    shares = [(k << 32) + j for k in (1, 2, -1, -(1 << 31), (1 << 31) - 1) for j in range(0, n_shares + 2)]
    for dv in (False, True):
        assert set(run(H, [6] * len(shares), shares, 5, 3, n_shares, dv)) == {NO_KEY}


def test_dv_mode_differs_only_at_share_zero(H):
    groups = [g for g in range(3, 10) for _ in range(14)]
    shares = [s for _ in range(3, 10) for s in range(-1, 13)]
    a, b = run(H, groups, shares, 5, 3, 10, False), run(H, groups, shares, 5, 3, 10, True)
    for g, s, x, y in zip(groups, shares, a, b):
        if s == 0 and 5 <= g < 8:
            assert x == NO_KEY and y == (g - 5) * 11
        else:
            assert x == y


@pytest.mark.parametrize("seed", range(6))
def test_seeded(H, seed):
    rng = np.random.default_rng(1000 + seed)
    n_shares = int(rng.choice([1, 3, 4, 7, 10, 64]))
    n_groups = int(rng.integers(0, 300))
    group_base = int(rng.integers(0, 1000))
    n = 4000
    groups = rng.integers(max(group_base - 20, 0), group_base + n_groups + 20, n).astype(np.uint32)
    shares = rng.integers(-3, n_shares + 4, n).astype(np.int64)
    wild = rng.random(n) < 0.1
    shares[wild] = rng.integers(I64_MIN, I64_MAX, int(wild.sum()), dtype=np.int64)
    wildg = rng.random(n) < 0.05
    groups[wildg] = rng.integers(0, 1 << 32, int(wildg.sum()), dtype=np.uint64).astype(np.uint32)
    for dv in (False, True):
        want = [cluster_key(int(g), int(s), group_base, n_groups, n_shares, dv) for g, s in zip(groups, shares)]
        assert run(H, groups, shares, group_base, n_groups, n_shares, dv) == want


def test_keys_of_a_shard_are_a_bijection(H):
    """Every (group, share 0 .. n_shares) of a shard in the DV mode: the numbers 0 .. n_keys - 1, each once."""
    gb, ng, ns = 11, 9, 5
    groups = [g for g in range(gb, gb + ng) for _ in range(ns + 1)]
    shares = [s for _ in range(ng) for s in range(ns + 1)]
    assert run(H, groups, shares, gb, ng, ns, True) == list(range(ng * (ns + 1)))


# ---- the binding

def header_arg_counts():
    src = open(os.path.join(ROOT, "include", "hipbls.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(hbls_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_binding_declares_the_entry_points():
    from charon_amd import _lib

    class Fn:
        pass

    class Lib:
        def __getattr__(self, name):
            fn = Fn()
            self.__dict__[name] = fn
            return fn

    fake = Lib()
    _lib._declare(fake)
    counts = header_arg_counts()
    want = {"hbls_cluster_open": 7, "hbls_cluster_close": 1, "hbls_cluster_stats": 3, "hbls_duty_open_cluster": 4}
    for name, k in want.items():
        assert counts.get(name) == k, (name, counts.get(name))
        assert name in _lib.EXPORTS
        fn = fake.__dict__.get(name)
        assert fn is not None, name + " is not declared in _lib._declare"
        assert len(fn.argtypes) == k and fn.restype is ctypes.c_int
    # handles are 64-bit by value, not pointers
    assert fake.hbls_cluster_close.argtypes[0] is ctypes.c_uint64
    assert fake.hbls_duty_open_cluster.argtypes[0] is ctypes.c_uint64
    assert fake.hbls_cluster_stats.argtypes[0] is ctypes.c_uint64
