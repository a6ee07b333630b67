"""The chunk cases of the ladder tables of learned keys, shared by tests/test_key_wide_host.py (the
CPU build) and tests/test_gpu_key_wide.py (the same cases on the device), and their oracle sums.

The test keys are known multiples of the generator, so the oracle's sum over a chunk is ONE
multiplication of the generator by sum (a_i + b_i lambda) s_i mod r."""
import random

from oracle import bls12381 as B

LAM = (-B.X_PARAM ** 2) % B.R  # phi(P) = [lambda] P on G1 (rlc.h)

SCALAR = {B.G1_GEN: 1}  # point -> its discrete logarithm
_KEYS = []


def keys():
    """8 random keys (computed once); they and their negatives are in SCALAR"""
    if not _KEYS:
        rng = random.Random(1615)
        for _ in range(8):
            s = rng.randrange(1, B.R)
            p = B.g1_mul(B.G1_GEN, s)
            SCALAR[p] = s
            SCALAR[B.g1_neg(p)] = B.R - s
            _KEYS.append(p)
    return list(_KEYS)


_WANT = {}  # scalar -> compressed multiple of the generator (many cases share their first item)


def want(pts, ab):
    """compressed sum (a_i + b_i lambda) P_i"""
    k = sum((a + b * LAM) * SCALAR[p] for p, (a, b) in zip(pts, ab)) % B.R
    if k not in _WANT:
        _WANT[k] = B.g1_compress(B.g1_mul(B.G1_GEN, k) if k else None)
    return _WANT[k]


# the coefficient pairs every chunk size runs (the last: both low halves zero)
FIXED = [(1, 0), (0, 1), (0xFFFFFFFF, 0xFFFFFFFF), (0x00010001, 0x00010001), (0x80000000, 0),
         (0xABCD0000, 0x12340000)]
SIZES = (1, 2, 10, 16)
PER_SIZE = len(FIXED) + 3


def cases():
    """(points, coefficient pairs): for each chunk size the fixed pairs, random pairs, (0, 0) on one
    item and the fixed pairs side by side; then the degenerate chunks"""
    ks = keys()
    rng = random.Random(404)
    out = []
    for k in SIZES:
        for c in FIXED:  # the fixed pair on every item of the chunk
            out.append(([ks[j % len(ks)] for j in range(k)], [c] * k))
        pts = [ks[rng.randrange(len(ks))] for _ in range(k)]
        out.append((pts, [(rng.getrandbits(32), rng.getrandbits(32)) for _ in range(k)]))  # random pairs
        ab = [(rng.getrandbits(32), rng.getrandbits(32)) for _ in range(k)]
        ab[k // 2] = (0, 0)  # an unusable item: contributes nothing
        out.append((pts, ab))
        out.append((pts, [FIXED[j % len(FIXED)] for j in range(k)]))
    # the same key twice (the ladder meets its own table point: a doubling inside the mixed
    # addition), P and -P with equal coefficients (the sum is at infinity)
    out.append(([ks[0], ks[0]], [(1, 0), (1, 0)]))
    out.append(([ks[0], ks[0]], [(0x00010001, 0x00010001)] * 2))
    out.append(([ks[3]] * 4, [(1, 0), (1, 0), (0xFFFFFFFF, 0), (0, 1)]))
    out.append(([ks[1], B.g1_neg(ks[1])], [(5, 0), (5, 0)]))
    out.append(([ks[1], B.g1_neg(ks[1])], [(0xDEADBEEF, 0x01234567)] * 2))
    out.append(([ks[2]] * 3, [(0xFFFFFFFF, 0xFFFFFFFF)] * 3))
    return out
