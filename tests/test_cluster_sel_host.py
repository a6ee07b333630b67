"""The selection rule of hbls_cluster_verify_aggregate on the CPU, through the g++ harness
tests/native/more/clusterselcheck.cpp: charon_amd/csrc/clustersel.h -- the functions cluster.hip's
k_cluster_row_sum selects a row's entries with and hipbls.hip refuses and counts a call with -- against a
Python restatement of include/hipbls.h, compared exactly.  And the binding: charon_amd/_lib.py declares
the three cluster-verify entry points with the header's argument counts.

The item-key rule of hbls_cluster_verify_batch (key index 0 allowed; -1, n_shares + 1, 2^32, 2^32 + 1 and
INT64_MIN name no key) is cluster.h cluster_key with dv = true, which tests/test_cluster_host.py already
pins through the clustercheck harness at every one of those values (test_edges with dv = True over
share_edges, test_truncation_is_never_a_key, test_dv_mode_differs_only_at_share_zero): nothing is added
for it here.
"""
import ctypes

import pytest

ALL64 = (1 << 64) - 1
N_SHARES = [1, 4, 64]


def sel_all(n_shares):
    return (1 << n_shares) - 1 if 1 <= n_shares <= 64 else 0


def sel_valid(mask, with_dv, n_shares):
    """include/hipbls.h: a mask bit at or above n_shares, or with_dv > 1, is a call error"""
    return 1 <= n_shares <= 64 and (mask >> n_shares) == 0 and with_dv in (0, 1)


def sel_entry(j, mask, with_dv):
    """entry 0 is the DV key (with_dv), entry j in 1 .. 64 the pubshare of share index j (bit j - 1)"""
    if j == 0:
        return with_dv == 1
    return 1 <= j <= 64 and bool((mask >> (j - 1)) & 1)


def masks(n_shares):
    """0, all ones, every single bit, the highest valid bit, bit n_shares (a call error), a mixed mask"""
    out = [0, sel_all(n_shares)] + [1 << b for b in range(n_shares)] + [1 << (n_shares - 1)]
    if n_shares < 64:
        out += [1 << n_shares, sel_all(n_shares) | (1 << n_shares), 1 << 63, ALL64]
    out.append(0x5A5A5A5A5A5A5A5A & sel_all(n_shares))
    return out


@pytest.fixture(scope="module")
def H():
    from gpu_helpers import more_harness
    lib = more_harness.load("clusterselcheck")
    U32, U64 = ctypes.c_uint32, ctypes.c_uint64
    lib.cs_max_shares.restype = U32
    lib.cs_all.argtypes, lib.cs_all.restype = [U32], U64
    lib.cs_valid.argtypes, lib.cs_valid.restype = [U64, U32, U32], ctypes.c_int
    lib.cs_entry.argtypes, lib.cs_entry.restype = [U32, U64, U32], ctypes.c_int
    lib.cs_count.argtypes, lib.cs_count.restype = [U64, U32], U32
    return lib


def test_constants(H):
    assert H.cs_max_shares() == 64
    assert [H.cs_all(n) for n in (0, 1, 4, 63, 64, 65, 0xFFFFFFFF)] == [0, 1, 15, (1 << 63) - 1, ALL64, 0, 0]


@pytest.mark.parametrize("n_shares", N_SHARES)
def test_which_pairs_are_call_errors(H, n_shares):
    for mask in masks(n_shares):
        for with_dv in (0, 1, 2, 0xFFFFFFFF):
            assert H.cs_valid(mask, with_dv, n_shares) == int(sel_valid(mask, with_dv, n_shares)), (hex(mask), with_dv)
    # the highest valid bit is valid, the one above it is not
    assert H.cs_valid(1 << (n_shares - 1), 0, n_shares) == 1
    if n_shares < 64:
        assert H.cs_valid(1 << n_shares, 0, n_shares) == 0
    assert H.cs_valid(0, 0, n_shares) == 1, "the empty selection is a status, not a call error"
    assert H.cs_valid(0, 2, n_shares) == 0 and H.cs_valid(sel_all(n_shares), 2, n_shares) == 0


def test_bit_63_at_64_shares(H):
    assert H.cs_valid(1 << 63, 0, 64) == 1 and H.cs_valid(ALL64, 1, 64) == 1
    assert H.cs_entry(64, 1 << 63, 0) == 1 and H.cs_entry(63, 1 << 63, 0) == 0
    assert H.cs_count(1 << 63, 0) == 1 and H.cs_count(ALL64, 1) == 65


def test_no_cluster_has_zero_or_65_shares(H):
    for n_shares in (0, 65, 0xFFFFFFFF):
        assert H.cs_valid(0, 0, n_shares) == 0 and H.cs_valid(1, 1, n_shares) == 0


@pytest.mark.parametrize("n_shares", N_SHARES)
def test_selected_entries_and_their_count(H, n_shares):
    for mask in masks(n_shares):
        for with_dv in (0, 1, 2):
            got = [H.cs_entry(j, mask, with_dv) for j in range(0, 68)]
            assert got == [int(sel_entry(j, mask, with_dv)) for j in range(0, 68)], (hex(mask), with_dv)
            if sel_valid(mask, with_dv, n_shares):
                # the selected count per row is the count of the row's selected entries
                assert H.cs_count(mask, with_dv) == sum(got[:n_shares + 1]) == bin(mask).count("1") + with_dv
    assert H.cs_entry(0xFFFFFFFF, ALL64, 1) == 0 and H.cs_entry(65, ALL64, 1) == 0


# ---- the binding

def test_binding_declares_the_entry_points():
    from charon_amd import _lib
    from test_cluster_host import header_arg_counts

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
    want = {"hbls_cluster_verify_batch": 9, "hbls_cluster_verify_aggregate": 7, "hbls_cluster_verify_stats": 3}
    for name, k in want.items():
        assert counts.get(name) == k, (name, counts.get(name))
        assert name in _lib.EXPORTS
        fn = fake.__dict__.get(name)
        assert fn is not None, name + " is not declared in _lib._declare"
        assert len(fn.argtypes) == k and fn.restype is ctypes.c_int
        assert fn.argtypes[0] is ctypes.c_uint64, "handles are 64-bit by value"
    assert fake.hbls_cluster_verify_aggregate.argtypes[1] is ctypes.c_uint64, "the mask is 64 bits by value"
