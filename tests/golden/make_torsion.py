"""Generate tests/golden/torsion_points.json: compressed points of E(Fp) and of the twist E'(Fp2)
whose order is a small (or the one large) prime factor of the cofactor -- on the curve, outside the
r-torsion subgroup, and with exceptional steps (R = +-T, R = infinity) all along a subgroup ladder,
which a random curve point (off_subgroup_g2.json) never has.  Drawn with a fixed seed by the oracle.

The cofactors are computed from the curve parameter and factored here (trial division, then a
Miller-Rabin test of what is left); nothing is transcribed.  For every prime q of a cofactor h:
  T     a point of exact order q: [r h / q^e] (random curve point), multiplied by q until the next
        step would vanish;
  -T;
  G+T   for a nonzero subgroup point G (order q r);
  T2    a point of order q^2 where one of "q2_draws" random draws found one; "q2_found" records
        which q have one.  (None has: every q with q^2 | h gave only points of order q in all
        draws -- the q-part of the group is Z_q x Z_q, not cyclic -- so the file holds no T2 entry.)

    python tests/golden/make_torsion.py
"""
import json
import math
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import bls12381 as B  # noqa: E402

X = B.X_PARAM
H1 = B.H1
_h2n = X ** 8 - 4 * X ** 7 + 5 * X ** 6 - 4 * X ** 4 + 6 * X ** 3 - 4 * X ** 2 - 4 * X + 13
assert _h2n % 9 == 0
H2 = _h2n // 9
TRIAL = 1 << 20


def is_probable_prime(n, rng, rounds=40):
    if n < 4:
        return n in (2, 3)
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for _ in range(rounds):
        x = pow(rng.randrange(2, n - 1), d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def factor(n, rng):
    """[(q, e)]: trial division to TRIAL, the rest must be 1 or a (probable) prime"""
    out, q = [], 2
    while q < TRIAL and n > 1:
        if n % q == 0:
            e = 0
            while n % q == 0:
                n, e = n // q, e + 1
            out.append((q, e))
        q += 1 if q == 2 else 2
    if n > 1:
        s = math.isqrt(n)
        if s * s == n:  # h1 = (x - 1)^2 / 3: its largest prime appears squared
            n, e = s, 2
        else:
            e = 1
        assert is_probable_prime(n, rng), "a composite factor above the trial division bound"
        out.append((n, e))
    return out


def random_g1(rng):
    while True:
        x = rng.randrange(B.P)
        y = B.fp_sqrt((x * x * x + B.B_G1) % B.P)
        if y is not None:
            return (x, y if rng.random() < 0.5 else (-y) % B.P)


def random_g2(rng):
    while True:
        x = (rng.randrange(B.P), rng.randrange(B.P))
        y = B.f2_sqrt(B.f2_add(B.f2_mul(B.f2_sqr(x), x), B.B_G2))
        if y is not None:
            return (x, y if rng.random() < 0.5 else B.f2_neg(y))


GROUPS = {
    "g1": (H1, B.g1_mul, B.g1_add, B.g1_neg, B.g1_compress, random_g1, B.G1_GEN),
    "g2": (H2, B.g2_mul, B.g2_add, B.g2_neg, B.g2_compress, random_g2, B.G2_GEN),
}


def q_part_point(mul, pt, h, q, e):
    """([r h / q^e] pt, its order q^k) -- None if it vanished"""
    t = mul(pt, B.R * (h // q ** e))
    if t is None:
        return None, 1
    k, u = 0, t
    while u is not None:
        u, k = mul(u, q), k + 1
    assert k <= e
    return t, q ** k


def main(seed=20261019, tries=6):
    rng = random.Random(seed)
    doc = {"seed": seed}
    for name, (h, mul, add, neg, compress, rand, gen) in GROUPS.items():
        fac = factor(h, rng)
        prod = 1
        for q, e in fac:
            prod *= q ** e
        assert prod == h
        for _ in range(2):  # h r annihilates the curve group
            assert mul(rand(rng), h * B.R) is None
        g = mul(gen, rng.randrange(1, B.R))
        entries, q2_found = [], []

        def put(kind, q, order, pt):
            entries.append({"kind": kind, "q": str(q), "order": str(order), "point": compress(pt).hex()})

        for q, e in fac:
            best, best_ord = None, 1
            for _ in range(tries if e > 1 else 1):
                t, o = None, 1
                while t is None:
                    t, o = q_part_point(mul, rand(rng), h, q, e)
                if o > best_ord:
                    best, best_ord = t, o
                if best_ord >= q * q or e == 1:
                    break
            t2 = None
            while best_ord > q * q:
                best, best_ord = mul(best, q), best_ord // q
            if best_ord == q * q:
                t2, best, best_ord = best, mul(best, q), q
            assert best is not None and mul(best, q) is None
            put("T", q, q, best)
            put("-T", q, q, neg(best))
            put("G+T", q, q * B.R, add(g, best))
            if t2 is not None:
                put("T2", q, q * q, t2)
                q2_found.append(str(q))
        doc[name] = {"cofactor": str(h), "factors": [[str(q), e] for q, e in fac], "q2_found": q2_found,
                     "q2_draws": tries, "points": entries}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "torsion_points.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
