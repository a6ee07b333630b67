"""hbls_cluster_check's criterion restated over the oracle (oracle/bls12381.py), and the rows the lock
check's tests share.  No GPU, no library: tests/test_lock_check_oracle.py holds this file to the
properties include/hipbls.h states, and the GPU tests compare the kernels and the ABI with it exactly.

A row is P_x = [f(x) mod r] H for x = 0 .. n (P_0 the DV key, P_1 .. P_n the pubshares), H one fixed
multiple of the generator and f a polynomial with small integer coefficients, so each oracle
multiplication is short.  A row is kept as its scalars AND its points: `check_points` restates the
criterion with the oracle's group law alone (the reference of every small shape); `check_scalars` is the
construction -- D_k = [sum_i c_i s_{k+i} mod r] H, which is O iff the sum is 0 mod r since H has order
r -- and serves the shapes with 64 shares, where the oracle's affine arithmetic would take minutes
(tests/test_lock_check_oracle.py checks the two against each other on every small row).
"""
import json
import math
import os

from oracle import bls12381 as B

OK, BAD_PUBKEY, NOT_VERIFIED = 0, 1, 3
H_SCALAR = 0x5EED1E55
H = B.g1_mul(B.G1_GEN, H_SCALAR)
INF = bytes([0xC0]) + bytes(47)

_points = {}


def point(s):
    """[s mod r] H (None: infinity), cached: rows share most of their points"""
    s %= B.R
    if s not in _points:
        _points[s] = B.g1_mul(H, s) if s else None
    return _points[s]


def coeffs(t):
    return [(-1) ** (t - i) * math.comb(t, i) for i in range(t + 1)]


def window_mask(n, t, p):
    """the windows a single wrong key at position p fails: {k : k <= p <= k + t}"""
    return sum(1 << k for k in range(n - t + 1) if k <= p <= k + t)


def poly_scalars(n, coef):
    """f(x) mod r for x = 0 .. n, f = coef[0] + coef[1] x + ..."""
    return [sum(c * x ** j for j, c in enumerate(coef)) % B.R for x in range(n + 1)]


def honest(n, t, seed, degree=None):
    """the scalars of a row of degree exactly `degree` (default t - 1): small non-zero coefficients"""
    d = t - 1 if degree is None else degree
    return poly_scalars(n, [((seed * 7 + 3 * j) % 11) + 1 for j in range(d + 1)])


def check_points(points, statuses, t):
    """(row_status, row_windows) of include/hipbls.h by the oracle's group law"""
    n = len(points) - 1
    if any(statuses):
        return BAD_PUBKEY, 0
    c, mask = coeffs(t), 0
    for k in range(n - t + 1):
        D = None
        for i in range(t + 1):
            D = B.g1_add(D, B.g1_mul(points[k + i], c[i]))
        if D is not None:
            mask |= 1 << k
    return (NOT_VERIFIED if mask else OK), mask


def check_scalars(scalars, statuses, t):
    """the same from the construction: D_k = [sum_i c_i s_{k+i}] H"""
    n = len(scalars) - 1
    if any(statuses):
        return BAD_PUBKEY, 0
    c, mask = coeffs(t), 0
    for k in range(n - t + 1):
        if sum(c[i] * scalars[k + i] for i in range(t + 1)) % B.R:
            mask |= 1 << k
    return (NOT_VERIFIED if mask else OK), mask


GOLDEN_ROWS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "lock_rows.json")
_golden = None


def golden_keys():
    """{scalar: compressed [scalar] H} of tests/golden/lock_rows.json (tests/golden/make_lock_rows.py
    writes it with this file and the oracle alone): the full-size scalars of the 64-share rows, each a
    255-step oracle ladder otherwise"""
    global _golden
    if _golden is None:
        with open(GOLDEN_ROWS) as f:
            d = json.load(f)
        assert d["h_scalar"] == hex(H_SCALAR)
        _golden = {int(s, 16): bytes.fromhex(k) for s, k in d["keys"].items()}
    return _golden


def key(s, cached=True):
    s %= B.R
    if cached and s.bit_length() > 64 and s in golden_keys():
        return golden_keys()[s]
    return B.g1_compress(point(s))


def compress(scalars):
    return b"".join(key(s) for s in scalars)


def shape_rows(n, t, honest_rows=4, one_base=False):
    """The rows every shape of the kernel tests includes, as [(name, scalars, statuses)]: honest rows,
    one key replaced at p = 0, at p = n and at an interior p, two pubshares swapped, a row whose key p
    has status 1, and a finite key of an honest row replaced by infinity.  one_base: every row is made
    from the same honest row (the 64-share shapes, whose points are full-size oracle ladders)."""
    def base(seed):
        return honest(n, t, 0 if one_base else seed)

    rows = [(f"honest{j}", base(j), [0] * (n + 1)) for j in range(honest_rows)]
    mid = max(1, n // 2)
    for name, p in (("replace0", 0), ("replace_n", n), ("replace_mid", mid)):
        s = base(20 + p)
        s[p] = (s[p] + 1000003) % B.R
        rows.append((name, s, [0] * (n + 1)))
    s = base(31)
    a, b = (1, n) if n > 1 else (0, 1)
    s[a], s[b] = s[b], s[a]
    rows.append(("swapped", s, [0] * (n + 1)))
    st = [0] * (n + 1)
    st[mid] = 1
    rows.append(("status1", base(32), st))
    s = base(33)
    s[mid] = 0
    rows.append(("infinity", s, [0] * (n + 1)))
    return rows


BIG_SHAPES = [(64, 33), (64, 64)]


def big_rows(n, t):
    return shape_rows(n, t, honest_rows=1, one_base=True)
