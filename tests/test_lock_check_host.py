"""The rule of hbls_cluster_check on the CPU, through the g++ harness tests/native/lockcheckhost.cpp:
charon_amd/csrc/lockcheck.h -- the signed binomial coefficients of a threshold, their common bit length
and the plan lockcheck.hip's k_lock_check takes as its argument -- against Python's math.comb for every
allowed threshold, and the refusals.  And the binding: charon_amd/_lib.py declares the entry points with
the header's argument counts.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S64 = -0x5A5A5A5A5A5A5A5B


@pytest.fixture(scope="module")
def H():
    from gpu_helpers import harness
    lib = harness.load("lockcheckhost")
    V, U32 = ctypes.c_void_p, ctypes.c_uint32
    lib.lk_max_t.restype = U32
    lib.lk_coeffs.argtypes = [U32, V]
    lib.lk_bits.argtypes = [U32]
    lib.lk_bits.restype = U32
    lib.lk_plan.argtypes = [U32, U32, V]
    return lib


def coeffs(H, t):
    c = np.full(max(t, 0) + 2 if t <= 64 else 70, S64, np.int64)
    rc = H.lk_coeffs(t, c.ctypes.data)
    return rc, c


def test_max_threshold(H):
    assert H.lk_max_t() == 64


@pytest.mark.parametrize("t", range(1, 65))
def test_coefficients_and_bit_length(H, t):
    rc, c = coeffs(H, t)
    assert rc == 1 and c[t + 1] == S64, "sentinel behind c[t]"
    assert [int(x) for x in c[:t + 1]] == [(-1) ** (t - i) * math.comb(t, i) for i in range(t + 1)]
    assert H.lk_bits(t) == math.comb(t, t // 2).bit_length()
    assert max(abs(int(x)) for x in c[:t + 1]) < 1 << 63
    assert sum(int(x) for x in c[:t + 1]) == 0, "a t-th difference annihilates constants"


@pytest.mark.parametrize("t", [0, 65, 66, 1 << 31, 0xFFFFFFFF])
def test_refused_thresholds_write_nothing(H, t):
    rc, c = coeffs(H, t)
    assert rc == 0 and (c == S64).all()
    assert H.lk_bits(t) == 0


def test_the_sizes_the_issue_names(H):
    assert H.lk_bits(7) == 6 and max(math.comb(7, i) for i in range(8)) == 35
    assert H.lk_bits(64) == 61 and H.lk_bits(33) == 31 and H.lk_bits(1) == 1


@pytest.mark.parametrize("n,t", [(4, 3), (4, 4), (3, 2), (5, 1), (10, 7), (64, 33), (64, 64), (1, 1)])
def test_plan(H, n, t):
    out = np.full(4 + 65 + 1, S64, np.int64)
    assert H.lk_plan(n, t, out.ctypes.data) == 1 and out[-1] == S64
    assert out[:4].tolist() == [n, t, n - t + 1, math.comb(t, t // 2).bit_length()]
    assert [int(x) for x in out[4:4 + t + 1]] == [(-1) ** (t - i) * math.comb(t, i) for i in range(t + 1)]
    assert not out[4 + t + 1:-1].any(), "the words behind c[t] are zero"
    assert n - t + 1 <= 64, "a row's verdicts fit one mask"


@pytest.mark.parametrize("n,t", [(4, 0), (4, 5), (64, 65), (65, 3), (65, 65), (0, 0), (0, 1), (0xFFFFFFFF, 1)])
def test_refused_plans_write_nothing(H, n, t):
    out = np.full(70, S64, np.int64)
    assert H.lk_plan(n, t, out.ctypes.data) == 0 and (out == S64).all()


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
    for name, k in {"hbls_cluster_check": 5, "hbls_cluster_check_stats": 3}.items():
        assert counts.get(name) == k, (name, counts.get(name))
        assert name in _lib.EXPORTS
        fn = fake.__dict__.get(name)
        assert fn is not None, name + " is not declared in _lib._declare"
        assert len(fn.argtypes) == k and fn.restype is ctypes.c_int
        assert fn.argtypes[0] is ctypes.c_uint64, "handles are 64-bit by value"
    assert fake.hbls_cluster_check.argtypes[1] is ctypes.c_uint32
