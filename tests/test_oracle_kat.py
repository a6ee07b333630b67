"""The oracle (oracle/bls12381.py) against the reference's own known-answer vectors.

KAT sources (extracted by tests/golden/make_kats.py):
  eth2util/signing/signing_test.go:24-74 (teku registration signature: Sign byte-exact),
  eth2util/deposit/testdata/TestMarshalDepositData.golden (4 Sign/Verify vectors),
  cluster/examples/cluster-lock-00{0..3}.json (VerifyAggregate over all pubshares, builder
  registration Verify under the DV key, Lagrange interpolation of pubshares to the DV key).
"""
import pytest

from oracle import bls12381 as B


def test_generators_valid():
    assert B.g1_in_subgroup(B.G1_GEN)
    assert B.g2_in_subgroup(B.G2_GEN)


def test_iso3_choice_pinned(kats):
    reg = kats["registration"]
    sk = bytes.fromhex(reg["sk"])
    msg = bytes.fromhex(reg["msg"])
    ok = [i for i in range(len(B.iso3_candidates()))
          if B.g2_compress(B.g2_mul(B.hash_to_g2(msg, iso_choice=i), B.sk_from_bytes(sk))).hex() == reg["sig"]]
    assert ok == [B.ISO3_CHOICE]


def test_registration_sign_kat(kats):
    reg = kats["registration"]
    sk = bytes.fromhex(reg["sk"])
    msg = bytes.fromhex(reg["msg"])
    assert B.sign(sk, msg).hex() == reg["sig"]
    assert B.verify(B.secret_to_public_key(sk), msg, bytes.fromhex(reg["sig"])) == B.ST_OK


@pytest.mark.parametrize("i", range(4))
def test_deposit_kats(kats, i):
    d = kats["deposit"][i]
    sk, msg = bytes.fromhex(d["sk"]), bytes.fromhex(d["msg"])
    assert B.secret_to_public_key(sk).hex() == d["pk"]
    assert B.sign(sk, msg).hex() == d["sig"]


@pytest.mark.slow
@pytest.mark.parametrize("i", range(4))
def test_lock_kats(kats, i):
    L = kats["locks"][i]
    pks = [bytes.fromhex(s) for v in L["validators"] for s in v["shares"]]
    assert B.verify_aggregate(pks, bytes.fromhex(L["signature_aggregate"]), bytes.fromhex(L["lock_hash"])) == B.ST_OK
    t = L["threshold"]
    for v in L["validators"]:
        ids = list(range(1, t + 1))
        acc = None
        for lam, idx in zip(B.lagrange_coeffs_at_zero(ids), ids):
            acc = B.g1_add(acc, B.g1_mul(B.g1_decompress(bytes.fromhex(v["shares"][idx - 1])), lam))
        assert B.g1_compress(acc).hex() == v["dpk"]
        if "registration" in v:
            r = v["registration"]
            assert B.verify(bytes.fromhex(v["dpk"]), bytes.fromhex(r["msg"]), bytes.fromhex(r["sig"])) == B.ST_OK


def test_fixtures_consistent_with_oracle_fast_paths(fixtures):
    # spot-check: decode-level verdicts of every verify case re-derived by the oracle
    for c in fixtures["verify"]:
        pk, sig = bytes.fromhex(c["pk"]), bytes.fromhex(c["sig"])
        try:
            B.g1_decompress(pk)
        except B.DecodeError:
            assert c["status"] == B.ST_BAD_PUBKEY, c["name"]
            continue
        try:
            B.g2_decompress(sig)
        except B.DecodeError:
            assert c["status"] == B.ST_BAD_SIGNATURE, c["name"]


def test_off_subgroup_fixture():
    """tests/golden/off_subgroup_g2.json (bench.py's C5 class 1): every point decompresses onto the
    curve but lies outside G2, so Verify reports an undecodable signature (oracle)."""
    import json
    import os
    from oracle import bls12381 as B
    path = os.path.join(os.path.dirname(__file__), "golden", "off_subgroup_g2.json")
    pts = json.load(open(path))["points"]
    assert len(pts) == 16
    for h in pts[:4]:
        b = bytes.fromhex(h)
        x = (int.from_bytes(b[48:], "big"), int.from_bytes(bytes([b[0] & 0x1F]) + b[1:48], "big"))
        y = B.f2_sqrt(B.f2_add(B.f2_mul(B.f2_sqr(x), x), B.B_G2))
        assert y is not None and not B.g2_in_subgroup((x, y))


def _torsion_entries():
    import json
    import os
    doc = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "torsion_points.json")))
    return [(g, e) for g in ("g1", "g2") for e in doc[g]["points"]]


def test_torsion_fixture_covers_every_cofactor_prime():
    """tests/golden/torsion_points.json: the recorded factorisations multiply to the cofactors (h1
    the oracle's, h2 from the curve parameter), and every prime of each has T, -T and G+T."""
    import json
    import os
    doc = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "torsion_points.json")))
    x = B.X_PARAM
    h2 = (x ** 8 - 4 * x ** 7 + 5 * x ** 6 - 4 * x ** 4 + 6 * x ** 3 - 4 * x ** 2 - 4 * x + 13) // 9
    for g, h in (("g1", B.H1), ("g2", h2)):
        prod = 1
        for q, e in doc[g]["factors"]:
            prod *= int(q) ** e
        assert prod == h == int(doc[g]["cofactor"])
        for q, _ in doc[g]["factors"]:
            kinds = sorted(e["kind"] for e in doc[g]["points"] if e["q"] == q and e["kind"] != "T2")
            assert kinds == ["-T", "G+T", "T"], (g, q)
        assert sorted(e["q"] for e in doc[g]["points"] if e["kind"] == "T2") == sorted(doc[g]["q2_found"])


@pytest.mark.parametrize("g,e", _torsion_entries(), ids=lambda v: v if isinstance(v, str) else v["kind"] + "/" + v["q"][:9])
def test_torsion_fixture(g, e):
    """every entry: on the curve, of exactly the recorded order ([order] pt = O, [order / q] pt != O),
    outside the subgroup, and refused by the decompressor"""
    dec, mul, insub = (B.g1_decompress, B.g1_mul, B.g1_in_subgroup) if g == "g1" else \
        (B.g2_decompress, B.g2_mul, B.g2_in_subgroup)
    raw = bytes.fromhex(e["point"])
    pt = dec(raw, subgroup_check=False)  # raises unless x is on the curve
    assert pt is not None
    q, order = int(e["q"]), int(e["order"])
    assert order % q == 0
    assert mul(pt, order) is None
    assert mul(pt, order // q) is not None
    assert not insub(pt)
    with pytest.raises(B.DecodeError):
        dec(raw)
