"""The verified-member selection rule of hbls_slot_select_device (charon_amd/csrc/tasel.h ta_select,
what threshold.hip's k_ta_select runs per lane) on the CPU, through the g++ harness
tests/native/taselcheck.cpp.

Expected values are hand-written rows, or come from rule() below: the rule as include/hipbls.h states
it -- a group's members are its first t candidates, in order, whose status is OK and whose share index
differs from every member already chosen -- never from the header.
"""
import ctypes
import itertools

import numpy as np
import pytest

OK, BAD_PUBKEY, BAD_SIGNATURE, NOT_VERIFIED = 0, 1, 2, 3
NONE = 0xFFFFFFFF
ST_OK, ST_FEW, ST_MIXED = 0, 1, 2


@pytest.fixture(scope="module")
def ts():
    from gpu_helpers import harness
    lib = harness.load("taselcheck")
    P, U = ctypes.c_void_p, ctypes.c_uint32
    lib.ts_select.argtypes, lib.ts_select.restype = [P, P, U, P, P, U, U, U, P, P, P], None
    lib.ts_max.restype = lib.ts_key_none.restype = U
    return lib


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def select(ts, vstatus, cand, t, msg_idx=None, b=None, e=None):
    """cand: [(partial, share index)] of one group.  -> dict(chosen, cidx, count, key, msg, state, shifted)"""
    vst = np.asarray(vstatus, dtype=np.uint8)
    n = len(vst)
    mid = np.asarray(msg_idx if msg_idx is not None else [0] * n, dtype=np.uint32)
    src = np.asarray([c[0] for c in cand] or [0], dtype=np.uint32)
    idx = np.asarray([c[1] for c in cand] or [0], dtype=np.int64)
    chosen, cidx, res = np.full(t, 12345, np.uint32), np.full(t, 12345, np.int64), np.zeros(5, np.uint32)
    ts.ts_select(_p(vst if n else np.zeros(1, np.uint8)), _p(mid if n else np.zeros(1, np.uint32)), n, _p(src), _p(idx),
                 0 if b is None else b, len(cand) if e is None else e, t, _p(chosen), _p(cidx), _p(res))
    return dict(chosen=[int(x) for x in chosen], cidx=[int(x) for x in cidx], count=int(res[0]), key=int(res[1]),
                msg=int(res[2]), state=int(res[3]), shifted=int(res[4]))


def rule(vstatus, cand, t):
    """(members as partial indices, their candidate positions)"""
    mem, pos, seen = [], [], set()
    for k, (p, x) in enumerate(cand):
        if len(mem) < t and p < len(vstatus) and vstatus[p] == OK and x not in seen:
            mem.append(p)
            pos.append(k)
            seen.add(x)
    return mem, pos


def shares(n, first=0):
    """The n partials first .. first + n - 1 under share indices 1 .. n"""
    return [(first + k, k + 1) for k in range(n)]


def test_all_ok(ts):
    r = select(ts, [OK] * 7, shares(7), 5)
    assert r["chosen"] == [0, 1, 2, 3, 4] and r["cidx"] == [1, 2, 3, 4, 5]
    assert (r["count"], r["state"], r["shifted"], r["key"]) == (5, ST_OK, 0, 0b11111)


@pytest.mark.parametrize("bad, chosen, key", [(0, [1, 2, 3, 4, 5], 0b111110), (2, [0, 1, 3, 4, 5], 0b111011),
                                              (6, [0, 1, 2, 3, 4], 0b011111)])
def test_bad_first_middle_last(ts, bad, chosen, key):
    vst = [OK] * 7
    vst[bad] = NOT_VERIFIED
    r = select(ts, vst, shares(7), 5)
    assert r["chosen"] == chosen and r["cidx"] == [c + 1 for c in chosen]
    assert (r["count"], r["state"], r["key"]) == (5, ST_OK, key)
    assert r["shifted"] == (0 if bad == 6 else 1)


def test_exactly_t_good_the_last_t(ts):
    r = select(ts, [BAD_SIGNATURE, NOT_VERIFIED, OK, OK, OK, OK, OK], shares(7), 5)
    assert r["chosen"] == [2, 3, 4, 5, 6] and (r["count"], r["state"], r["shifted"]) == (5, ST_OK, 1)


def test_t_minus_one_good(ts):
    r = select(ts, [OK, BAD_SIGNATURE, OK, NOT_VERIFIED, OK, BAD_PUBKEY, OK], shares(7), 5)
    assert r["chosen"] == [0, 2, 4, 6, NONE] and r["cidx"] == [1, 3, 5, 7, 0]
    assert (r["count"], r["state"], r["shifted"], r["key"]) == (4, ST_FEW, 0, ts.ts_key_none())


def test_none_good_and_no_candidates(ts):
    r = select(ts, [NOT_VERIFIED] * 7, shares(7), 5)
    assert r["chosen"] == [NONE] * 5 and (r["count"], r["state"]) == (0, ST_FEW)
    r = select(ts, [OK] * 7, [], 5)
    assert r["chosen"] == [NONE] * 5 and (r["count"], r["state"], r["msg"]) == (0, ST_FEW, 0)
    r = select(ts, [], [], 3)  # a call without partials
    assert r["chosen"] == [NONE] * 3 and (r["count"], r["state"]) == (0, ST_FEW)


def test_group_in_the_middle_of_the_arrays(ts):
    """Candidates [b, e) of a longer list; the members index the partials, not the candidates."""
    cand = shares(4, 0) + shares(4, 4) + shares(4, 8)
    vst = [OK] * 12
    vst[5] = NOT_VERIFIED
    r = select(ts, vst, cand, 3, b=4, e=8)
    assert r["chosen"] == [4, 6, 7] and r["cidx"] == [1, 3, 4] and r["key"] == 0b1101 and r["shifted"] == 1


def test_repeated_share_index_skips_the_second(ts):
    # partial 1 arrives twice (a replay), and partial 3 claims share index 1 again
    cand = [(0, 1), (1, 2), (1, 2), (3, 1), (4, 5), (5, 6)]
    r = select(ts, [OK] * 6, cand, 4)
    assert r["chosen"] == [0, 1, 4, 5] and r["cidx"] == [1, 2, 5, 6]
    assert (r["count"], r["state"], r["shifted"], r["key"]) == (4, ST_OK, 1, 0b110011)
    # a failed partial does not reserve its share index
    r = select(ts, [NOT_VERIFIED, OK, OK], [(0, 1), (1, 1), (2, 2)], 2)
    assert r["chosen"] == [1, 2] and r["cidx"] == [1, 2]


def test_candidate_naming_no_partial_counts_as_not_verified(ts):
    r = select(ts, [OK] * 3, [(0, 1), (7, 2), (NONE, 3), (2, 4)], 2)
    assert r["chosen"] == [0, 2] and r["cidx"] == [1, 4] and r["state"] == ST_OK


def test_mixed_messages(ts):
    r = select(ts, [OK] * 4, shares(4), 3, msg_idx=[2, 2, 5, 2])
    assert r["state"] == ST_MIXED and r["key"] == ts.ts_key_none() and r["msg"] == 2
    # the differing candidate need not be a verified one, and mixed wins over too few
    r = select(ts, [OK, OK, OK, NOT_VERIFIED], shares(4), 3, msg_idx=[1, 1, 1, 0])
    assert r["state"] == ST_MIXED and r["chosen"] == [0, 1, 2]
    r = select(ts, [OK, NOT_VERIFIED, NOT_VERIFIED, NOT_VERIFIED], shares(4), 3, msg_idx=[1, 1, 1, 0])
    assert r["state"] == ST_MIXED and r["count"] == 1
    r = select(ts, [OK] * 4, shares(4), 3, msg_idx=[3, 3, 3, 3])
    assert r["state"] == ST_OK and r["msg"] == 3


def test_threshold_one_and_the_maximum(ts):
    assert ts.ts_max() == 16
    r = select(ts, [NOT_VERIFIED, OK], shares(2), 1)
    assert r["chosen"] == [1] and (r["state"], r["shifted"]) == (ST_OK, 1)
    vst = [OK] * 20
    vst[3] = NOT_VERIFIED
    r = select(ts, vst, shares(20), 16)
    assert r["chosen"] == [k for k in range(17) if k != 3] and r["state"] == ST_OK


def test_class_keys_equal_exactly_when_the_positions_are(ts):
    """Every status pattern of 7 and of 16 candidates with at least t good: the key is a function of
    the chosen positions and distinct position sets get distinct keys (<= 16 candidates)."""
    for n, t, patterns in ((7, 5, itertools.product((OK, NOT_VERIFIED), repeat=7)),
                           (16, 3, ([OK if (m >> k) & 1 else BAD_SIGNATURE for k in range(16)] for m in range(0, 65536, 37)))):
        by_key = {}
        for vst in patterns:
            vst = list(vst)
            mem, pos = rule(vst, shares(n), t)
            if len(mem) < t:
                continue
            r = select(ts, vst, shares(n), t)
            assert r["chosen"] == mem and r["state"] == ST_OK
            assert r["shifted"] == (pos != list(range(t)))
            assert by_key.setdefault(r["key"], tuple(pos)) == tuple(pos)
            assert r["key"] < 65536
        assert len(set(by_key.values())) == len(by_key) > 1


def test_wide_groups_fold_the_key(ts):
    """More than 16 candidates: positions p and p + 16 share a key bit (a collision is allowed)."""
    vst = [OK] * 20
    a = select(ts, vst, shares(20), 2)
    assert a["key"] == 0b11
    vst[0] = NOT_VERIFIED
    vst[2:16] = [NOT_VERIFIED] * 14
    b = select(ts, vst, shares(20), 2)  # positions 1 and 16
    assert b["chosen"] == [1, 16] and b["key"] == 0b11 and b["shifted"] == 1


def test_random_rows_against_the_rule(ts):
    rng = np.random.default_rng(5)
    for _ in range(300):
        n, t = int(rng.integers(1, 12)), int(rng.integers(1, 8))
        vst = [int(x) for x in rng.choice([OK, OK, OK, NOT_VERIFIED, BAD_SIGNATURE], size=n)]
        cand = [(int(rng.integers(0, n)), int(rng.integers(1, 6))) for _ in range(int(rng.integers(0, 12)))]
        mem, pos = rule(vst, cand, t)
        r = select(ts, vst, cand, t)
        assert r["chosen"] == mem + [NONE] * (t - len(mem)) and r["count"] == len(mem)
        assert r["state"] == (ST_OK if len(mem) == t else ST_FEW)
