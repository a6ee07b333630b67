"""hbls_slot_select_batch: one duty from host buffers to aggregates (what the Go shim calls), -m gpu.

Inputs are the tests/gpu_helpers/slot_select.py clusters: 256 validators (four waves), 5 of 7 and 3
of 4, four messages.  The references are the device entry point on the same bytes (ss.run), the
construction (root_sigs: the shares of a validator come from one polynomial, so every correct
aggregate equals the root key's signature byte for byte), the matching rule restated in Python
(matching() below: parsigdb/memory.go:149-160, 197-225 as include/hipbls.h states it) and, for one
validator, the bigint oracle.  Every comparison is exact.

A case is a dict of host arrays: pks (N x 48), sigs (N x 96), msgs (N x 32), the candidates (src,
idx, goff), dv (G x 48) and t.
"""
import ctypes
import hashlib
import os
import sys
import threading

import numpy as np
import pytest

from charon_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPERS = os.path.join(ROOT, "tests", "gpu_helpers")
for p in (ROOT, HELPERS):
    if p not in sys.path:
        sys.path.insert(0, p)

OK, BAD_PUBKEY, BAD_SIGNATURE, NOT_VERIFIED, COMBINE_FAILED, BAD_INPUT, UNCHECKED = 0, 1, 2, 3, 4, 6, 7
NONE = 0xFFFFFFFF
KEYS = ("vst", "chosen", "count", "out", "tst", "ast")
PAD = 64  # sentinel entries behind every output array


@pytest.fixture(scope="module")
def L(hipbls):
    return _lib.load_library()


@pytest.fixture(scope="module")
def ss():
    import slot_select
    return slot_select


@pytest.fixture(scope="module")
def clusters(L, ss):
    return {(7, 5): ss.inputs(L, 7, 5), (4, 3): ss.inputs(L, 4, 3)}


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def host(L, c, raw=False):
    """hbls_slot_select_batch on a case -> dict of KEYS.  Every output array has PAD sentinel entries
    behind it, which must come back untouched."""
    N, G, t = len(c["pks"]), len(c["goff"]) - 1, c["t"]
    pks, sigs, msgs = (np.ascontiguousarray(c[k]).reshape(-1) for k in ("pks", "sigs", "msgs"))
    off = np.arange(max(N, 1), dtype=np.uint64) * 32
    ln = np.full(max(N, 1), 32, dtype=np.uint32)
    src = np.ascontiguousarray(c["src"], dtype=np.uint32) if len(c["src"]) else np.zeros(1, np.uint32)
    idx = np.ascontiguousarray(c["idx"], dtype=np.int64) if len(c["idx"]) else np.zeros(1, np.int64)
    goff = np.ascontiguousarray(c["goff"], dtype=np.uint32)
    dv = np.ascontiguousarray(c["dv"]).reshape(-1)[:48 * G] if G else np.zeros(48, np.uint8)
    o = dict(vst=np.full(N + PAD, 0xA5, np.uint8), chosen=np.full(G * t + PAD, 0xA5A5A5A5, np.uint32),
             count=np.full(G + PAD, 0xA5A5A5A5, np.uint32), out=np.full(96 * G + PAD, 0xA5, np.uint8),
             tst=np.full(G + PAD, 0xA5, np.uint8), ast=np.full(G + PAD, 0xA5, np.uint8))
    rc = L.hbls_slot_select_batch(_p(pks if N else np.zeros(48, np.uint8)), _p(sigs if N else np.zeros(96, np.uint8)),
                                  _p(msgs if N else np.zeros(32, np.uint8)), _p(off), _p(ln), N, _p(src), _p(idx),
                                  _p(goff), G, _p(dv), t, *(_p(o[k]) for k in KEYS))
    if raw:
        return rc, o
    assert rc == 0, L.hbls_last_error().decode()
    size = dict(vst=N, chosen=G * t, count=G, out=96 * G, tst=G, ast=G)
    for k in KEYS:
        assert (o[k][size[k]:] == (0xA5 if o[k].dtype == np.uint8 else 0xA5A5A5A5)).all(), "sentinel behind " + k
        o[k] = o[k][:size[k]]
    o["chosen"], o["out"] = o["chosen"].reshape(G, t), o["out"].reshape(G, 96)
    return o


def same(a, b, what=""):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (what, k)


def case(ss, d, sigs=None, cand=None, pks=None):
    NP = d["NP"]
    src, idx, goff = cand if cand is not None else ss.all_candidates(d)
    return dict(pks=(d["pks"] if pks is None else pks).reshape(NP, 48), sigs=(d["sigs"] if sigs is None else sigs).reshape(NP, 96),
                msgs=d["msgs"].reshape(-1, 32)[d["midx"]], src=np.asarray(src, np.uint32), idx=np.asarray(idx, np.int64),
                goff=np.asarray(goff, np.uint32), dv=d["dv_pks"].reshape(-1, 48), t=d["t"])


def edge_case(L, ss, d):
    """tests/test_gpu_slot_select.py's threshold-edge input without its mixed-message validator.
    -> (sigs, pks, candidates, expected vstatus)"""
    n, V, NP = d["n"], d["V"], d["NP"]
    sigs, pks = d["sigs"].reshape(NP, 96).copy(), d["pks"].copy()
    items = [(1 * n + 0, 2), (1 * n + 1, 0)]                               # v1: exactly t good, the last t
    items += [(2 * n + 0, 1), (2 * n + 2, 3), (2 * n + 4, 4)]              # v2: t - 1 good
    items += [(3 * n + k, k % 5) for k in range(n)]                        # v3: none good
    exp_v = ss.corrupt_at(L, d, sigs, items)
    pks[48 * (5 * n + 1):48 * (5 * n + 1) + 48] = 0xFF                     # v5: an undecodable key
    exp_v[5 * n + 1] = BAD_PUBKEY
    src, idx, goff = [], [], [0]
    for v in range(V):
        c, x = list(range(v * n, v * n + n)), list(range(1, n + 1))
        if v == 4:                                                         # v4: no candidates
            c, x = [], []
        if v == 6:                                                         # v6: a candidate listed twice
            c, x = [c[0], c[0]] + c[1:], [x[0], x[0]] + x[1:]
        if v == 8:                                                         # v8: share index 0 among the good
            x[1] = 0
        src += c
        idx += x
        goff.append(len(src))
    return sigs, pks, (np.asarray(src, np.uint32), np.asarray(idx, np.int64), np.asarray(goff, np.uint32)), exp_v


@pytest.fixture(scope="module")
def base(L, ss, clusters):
    """The single-root cases with the device entry's result on the same bytes: name -> (case, device result)."""
    out = {}
    for key, d in clusters.items():
        out["clean", key] = (case(ss, d), ss.run(L, d))
        sigs, _ = ss.skip_case(L, d)
        out["skip", key] = (case(ss, d, sigs=sigs), ss.run(L, d, sigs=sigs))
    d = clusters[(7, 5)]
    sigs, pks, cand, exp_v = edge_case(L, ss, d)
    out["edge", (7, 5)] = (case(ss, d, sigs=sigs, cand=cand, pks=pks), ss.run(L, d, sigs=sigs, cand=cand, pks=pks))
    assert np.array_equal(out["edge", (7, 5)][1]["vst"], exp_v)
    return out


@pytest.fixture(scope="module")
def base_host(L, base):
    return {k: host(L, c) for k, (c, _) in base.items()}


def to_peer(c, V, n, extra=0):
    """The same bytes in peer-major order: item v n + share -> share V + v (the `extra` partials behind
    them stay).  -> (case, back: new index -> old index)"""
    N = len(c["pks"])
    assert N == V * n + extra
    old = np.arange(N)
    new_of_old = np.where(old < V * n, (old % n) * V + old // n, old)
    back = np.empty(N, dtype=np.int64)
    back[new_of_old] = old
    p = dict(c)
    for k in ("pks", "sigs", "msgs"):
        p[k] = np.ascontiguousarray(c[k][back])
    src = np.asarray(c["src"], dtype=np.int64)
    p["src"] = np.where(src < N, new_of_old[np.minimum(src, N - 1)], src).astype(np.uint32)
    return p, back


def from_peer(r, back):
    """A peer-major result in the validator-major case's terms."""
    o = dict(r)
    o["vst"] = np.empty_like(r["vst"])
    o["vst"][back] = r["vst"]
    ch = r["chosen"].astype(np.int64)
    o["chosen"] = np.where(ch == NONE, NONE, back[np.minimum(ch, len(back) - 1)]).astype(np.uint32)
    return o


# ---------------------------------------------------------------------------------------------
# 1, 2: the host call against the device entry, validator-major and peer-major
# ---------------------------------------------------------------------------------------------
def test_host_call_equals_device_entry(clusters, base, base_host):
    for name, (c, dev) in base.items():
        r = base_host[name]
        same(r, dev, name)
        d = clusters[name[1]]
        have = r["tst"] == OK
        assert np.array_equal(r["out"][have], d["root_sigs"].reshape(-1, 96)[have]), name
        assert have.sum() >= d["V"] - 5 and not r["out"][~have].any()
    r = base_host["edge", (7, 5)]
    assert [int(x) for x in r["tst"][:7]] == [OK, OK, UNCHECKED, UNCHECKED, UNCHECKED, OK, OK] and r["tst"][8] not in (OK, UNCHECKED)
    assert r["count"][2] == 4 and r["count"][3] == 0 and r["count"][4] == 0


def test_peer_major_layout(L, clusters, base, base_host):
    for name, (c, _) in base.items():
        d = clusters[name[1]]
        p, back = to_peer(c, d["V"], d["n"])
        same(from_peer(host(L, p), back), base_host[name], name)


# ---------------------------------------------------------------------------------------------
# 3: the matching rule
# ---------------------------------------------------------------------------------------------
def matching(vst, root_of, cand, t):
    """[(partial, share index)] -> (member partials, winning root or None): candidate j is stored iff
    it is verified and no earlier verified candidate has its share index; the first root to hold t
    stored candidates wins.  Without a winner, candidates over one root report their stored ones and
    candidates over several roots none."""
    seen, by_root = set(), {}
    for p, x in cand:
        if p >= len(vst) or vst[p] != OK or x in seen:
            continue
        seen.add(x)
        mem = by_root.setdefault(root_of[p], [])
        mem.append(p)
        if len(mem) == t:
            return mem, root_of[p]
    roots = {root_of[p] for p, _ in cand if p < len(vst)}
    return (next(iter(by_root.values()), []) if len(roots) <= 1 else []), None


def sign(L, sks, msgs):
    """hbls_sign_batch: sks (k x 32), msgs (k x 32) -> k x 96"""
    k = len(sks)
    sks, msgs = np.ascontiguousarray(sks).reshape(-1), np.ascontiguousarray(msgs).reshape(-1)
    out, st = np.zeros(96 * k, np.uint8), np.zeros(k, np.uint8)
    off, ln = np.arange(k, dtype=np.uint64) * 32, np.full(k, 32, np.uint32)
    assert L.hbls_sign_batch(_p(sks), _p(msgs), _p(off), _p(ln), k, _p(out), _p(st)) == 0 and not st.any()
    return out.reshape(k, 96)


@pytest.fixture(scope="module")
def two_roots(L, ss, clusters):
    """The 5-of-7 cluster with some partials re-signed over a second root B (validator v follows
    pattern v % 6), the re-signed copies that arrive beside a validator's own partials appended behind
    the V n partials.  -> (case, expected result, number of appended partials)
      0  untouched: root A with the first t
      1  shares 1, 2 over B: A wins with shares 3 .. 7
      2  copies of shares 1 .. 5 over B arrive first, then the seven over A: the minority root B wins
         (the seven over A are dropped or too late)
      3  shares 1 .. 3 over B, 4 .. 7 over A: seven verify, no root reaches t
      4  a copy of share 1 over B arrives first: share 1 over A is dropped, A wins with shares 2 .. 6
      5  copies of shares 1 .. 3 over B arrive first: A keeps 4 .. 7 only, nobody reaches t"""
    from charon_amd import synth
    from charon_amd.shard import owned_validators
    d = clusters[(7, 5)]
    V, n, t, NP = d["V"], d["n"], d["t"], d["NP"]
    B = np.frombuffer(ss.OTHER_ROOT, dtype=np.uint8)
    sks = d["sks"].reshape(NP, 32)
    c = case(ss, d)
    sigs, msgs, pks = c["sigs"].copy(), c["msgs"].copy(), c["pks"]
    resign = [v * n + s for v in range(V) for s in range({1: 2, 3: 3}.get(v % 6, 0))]
    sigs[resign] = sign(L, sks[resign], np.tile(B, (len(resign), 1)))
    msgs[resign] = B
    copies = [v * n + s for v in range(V) for s in range({2: 5, 4: 1, 5: 3}.get(v % 6, 0))]
    sigs = np.concatenate([sigs, sign(L, sks[copies], np.tile(B, (len(copies), 1)))])
    msgs = np.concatenate([msgs, np.tile(B, (len(copies), 1))])
    pks = np.concatenate([pks, pks[copies]])
    src, idx, goff, at = [], [], [0], NP
    for v in range(V):
        k = {2: 5, 4: 1, 5: 3}.get(v % 6, 0)
        src += list(range(at, at + k)) + list(range(v * n, v * n + n))
        idx += list(range(1, k + 1)) + list(range(1, n + 1))
        at += k
        goff.append(len(src))
    assert at == len(pks)
    c.update(pks=pks, sigs=sigs, msgs=msgs, src=np.asarray(src, np.uint32), idx=np.asarray(idx, np.int64),
             goff=np.asarray(goff, np.uint32))
    # expected, from the restated rule and the root keys
    cl = synth.make_cluster(V, n, t, first_validator=owned_validators(0, V).start, n_msgs=4, distinct_messages=False)
    root_of = [bytes(m) for m in msgs]
    exp = dict(vst=np.zeros(len(pks), np.uint8), chosen=np.full((V, t), NONE, np.uint32), count=np.zeros(V, np.uint32),
               out=np.zeros((V, 96), np.uint8), tst=np.full(V, UNCHECKED, np.uint8), ast=np.full(V, UNCHECKED, np.uint8))
    win_b = []
    for v in range(V):
        mem, root = matching(exp["vst"], root_of, list(zip(src[goff[v]:goff[v + 1]], idx[goff[v]:goff[v + 1]])), t)
        exp["chosen"][v, :len(mem)] = mem
        exp["count"][v] = len(mem)
        assert (root is None) == (v % 6 in (3, 5)) and (root == ss.OTHER_ROOT) == (v % 6 == 2)
        if root is not None:
            exp["tst"][v] = exp["ast"][v] = OK
            if root == ss.OTHER_ROOT:
                win_b.append(v)
            else:
                exp["out"][v] = d["root_sigs"].reshape(V, 96)[v]
    root_sks = np.frombuffer(b"".join(cl.root_sks), dtype=np.uint8).reshape(V, 32)
    # the cluster is the one the inputs were signed with: its root keys give root_sigs
    assert np.array_equal(sign(L, root_sks[:2], d["msgs"].reshape(-1, 32)[d["midx"][[0, n]]]), d["root_sigs"].reshape(V, 96)[:2])
    exp["out"][win_b] = sign(L, root_sks[win_b], np.tile(B, (len(win_b), 1)))
    return c, exp, len(copies)


@pytest.fixture(scope="module")
def two_roots_host(L, two_roots):
    return host(L, two_roots[0])


def test_matching_rule(ss, clusters, two_roots, two_roots_host):
    from oracle import bls12381 as Bo
    c, exp, _ = two_roots
    r = two_roots_host
    same(r, exp)
    d = clusters[(7, 5)]
    n, t, NP = d["n"], d["t"], d["NP"]
    assert list(r["chosen"][1]) == [n + 2, n + 3, n + 4, n + 5, n + 6]
    assert list(r["chosen"][2]) == [NP + k for k in range(5)]                   # the copies over B: appended first
    assert list(r["chosen"][3]) == [NONE] * t and r["tst"][3] == UNCHECKED and r["count"][3] == 0
    assert list(r["chosen"][4]) == [4 * n + 1 + k for k in range(5)]
    assert r["tst"][5] == UNCHECKED and not r["out"][5].any()
    # the oracle on the validator whose minority root won
    members = {int(c["idx"][c["goff"][2] + k]): bytes(c["sigs"][int(m)]) for k, m in enumerate(r["chosen"][2])}
    assert sorted(members) == [1, 2, 3, 4, 5]
    st, agg = Bo.threshold_aggregate(members)
    assert st == OK and agg == bytes(r["out"][2])
    assert Bo.verify(bytes(c["dv"][2]), ss.OTHER_ROOT, agg) == OK


# ---------------------------------------------------------------------------------------------
# 4: several devices
# ---------------------------------------------------------------------------------------------
def test_device_split(L, ss, clusters, two_roots):
    """Two and three contexts on the peer-major two-root input, with partials no validator lists (two
    of them corrupted) and one partial listed by validators 0 and V - 1, against the unsplit run."""
    c, _, ncopies = two_roots
    d = clusters[(7, 5)]
    V, n = d["V"], d["n"]
    c = dict(c)
    orphans = [3, 10 * n + 2, 77 * n + 6, 200 * n, 255 * n + 1]
    for k in ("pks", "sigs", "msgs"):
        c[k] = np.concatenate([c[k], c[k][orphans]])
    c["sigs"][-1] = c["sigs"][0]                     # verifies under another key only
    c["sigs"][-2, 5] ^= 1                            # not a signature any more (or not this one)
    src, idx, goff = list(c["src"]), list(c["idx"]), c["goff"]
    c["src"] = np.asarray(src + [src[0]], np.uint32)  # V - 1 also lists validator 0's first candidate
    c["idx"] = np.asarray(idx + [9], np.int64)
    c["goff"] = np.concatenate([goff[:-1], [goff[-1] + 1]]).astype(np.uint32)
    p, back = to_peer(c, V, n, extra=ncopies + len(orphans))
    one = host(L, p)
    assert one["vst"][-1] == NOT_VERIFIED and one["vst"][-2] in (BAD_SIGNATURE, NOT_VERIFIED) and not one["vst"][-5:-2].any()
    devices = L.hbls_device_count()
    try:
        for copies in (2, 3):
            assert L.hbls_debug_split(copies) == 0
            assert L.hbls_device_count() == copies * devices
            same(host(L, p), one, copies)
    finally:
        assert L.hbls_debug_split(1) == 0
    same(host(L, p), one, "restored")


# ---------------------------------------------------------------------------------------------
# 5: edges and call errors
# ---------------------------------------------------------------------------------------------
def sub(c, V, n):
    """The first V validators of a validator-major case with n candidates each."""
    s = dict(c)
    for k in ("pks", "sigs", "msgs"):
        s[k] = c[k][:V * n]
    s.update(src=c["src"][:V * n], idx=c["idx"][:V * n], goff=c["goff"][:V + 1], dv=c["dv"][:V])
    return s


def test_edges(L, clusters, base, base_host):
    d = clusters[(4, 3)]
    V, n, t = 6, d["n"], d["t"]
    c = sub(base["clean", (4, 3)][0], V, n)
    full = base_host["clean", (4, 3)]
    r = host(L, c)
    for k in KEYS:
        assert np.array_equal(r[k], full[k][:len(r[k])]), k
    # n == 0: every group unchecked, whatever its candidates name
    e = dict(c, pks=c["pks"][:0], sigs=c["sigs"][:0], msgs=c["msgs"][:0])
    r0 = host(L, e)
    assert len(r0["vst"]) == 0 and (r0["tst"] == UNCHECKED).all() and (r0["ast"] == UNCHECKED).all()
    assert not r0["out"].any() and not r0["count"].any() and (r0["chosen"] == NONE).all()
    # n_groups == 0: the partials are verified, nothing else is written
    g0 = dict(c, src=c["src"][:0], idx=c["idx"][:0], goff=np.zeros(1, np.uint32))
    r1 = host(L, g0)
    assert np.array_equal(r1["vst"], r["vst"]) and len(r1["tst"]) == 0
    bad = dict(g0, sigs=c["sigs"].copy())
    bad["sigs"][5] = c["sigs"][6]
    assert [int(x) for x in host(L, bad)["vst"]] == [OK] * 5 + [NOT_VERIFIED] + [OK] * (V * n - 6)
    # n == 0 and n_groups == 0
    assert host(L, dict(e, src=c["src"][:0], idx=c["idx"][:0], goff=np.zeros(1, np.uint32)))["vst"].size == 0
    # an empty group, candidates naming no partial, an undecodable DV key
    goff = c["goff"].copy()
    goff[2:] -= n                                     # validator 1 lists nothing (its partials: orphans)
    src = np.concatenate([c["src"][:n], c["src"][2 * n:]]).astype(np.uint32)
    idx = np.concatenate([c["idx"][:n], c["idx"][2 * n:]])
    src[1] = V * n                                    # validator 0: two candidates name no partial
    src[2] = NONE
    dv = c["dv"].copy()
    dv[3] = 0xFF
    r2 = host(L, dict(c, src=src, idx=idx, goff=goff, dv=dv))
    assert np.array_equal(r2["vst"], r["vst"])
    assert [int(x) for x in r2["tst"]] == [UNCHECKED, UNCHECKED, OK, OK, OK, OK]
    assert [int(x) for x in r2["ast"]] == [UNCHECKED, UNCHECKED, OK, BAD_PUBKEY, OK, OK]
    assert list(r2["chosen"][0]) == [0, 3, NONE] and r2["count"][0] == 2 and list(r2["chosen"][1]) == [NONE] * t
    assert not r2["out"][:2].any() and np.array_equal(r2["out"][2:], r["out"][2:])


def test_call_errors(L, base):
    c = sub(base["clean", (4, 3)][0], 4, 4)

    def err(c, **kw):
        a = dict(pks=c["pks"], sigs=c["sigs"], msgs=c["msgs"], off=np.arange(16, dtype=np.uint64) * 32,
                 ln=np.full(16, 32, np.uint32), n=16, src=c["src"], idx=c["idx"], goff=c["goff"], G=4, dv=c["dv"], t=c["t"],
                 vst=np.zeros(16, np.uint8), chosen=np.zeros(64, np.uint32), count=np.zeros(4, np.uint32),
                 out=np.zeros(4 * 96, np.uint8), tst=np.zeros(4, np.uint8), ast=np.zeros(4, np.uint8))
        a.update(kw)
        keep = [np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v for v in
                (a[k] for k in ("pks", "sigs", "msgs", "off", "ln", "n", "src", "idx", "goff", "G", "dv", "t", "vst", "chosen",
                                "count", "out", "tst", "ast"))]
        rc = L.hbls_slot_select_batch(*(_p(v) if isinstance(v, np.ndarray) or v is None else v for v in keep))
        return rc, L.hbls_last_error().decode()

    assert err(c)[0] == 0
    for t in (0, 17):
        assert err(c, t=t) == (-1, "hbls_slot_select_batch: threshold must be in 1..16")
    assert err(c, goff=np.asarray([0, 4, 3, 12, 16], np.uint32)) == (-1, "hbls_slot_select_batch: grp_off must be non-decreasing")
    for n, G, t in ((0xFFFFFFFF, 4, 3), (1 << 40, 4, 3), (16, 0xFFFFFFFF, 1), (16, 0x10000000, 16)):
        assert err(c, n=n, G=G, t=t) == (-1, "hbls_slot_select_batch: too many items")
    want = (-1, "hbls_slot_select_batch: pks, sigs, msg_off, msg_len and vstatus are required")
    for k in ("pks", "sigs", "off", "ln", "vst"):
        assert err(c, **{k: None}) == want, k
    assert err(c, msgs=None) == (-1, "hbls_slot_select_batch: msgs is required")
    want = (-1, "hbls_slot_select_batch: grp_off, dv_pks, chosen, ta_count, ta_out, ta_status and agg_vstatus are required")
    for k in ("goff", "dv", "chosen", "count", "out", "tst", "ast"):
        assert err(c, **{k: None}) == want, k
    for k in ("src", "idx"):
        assert err(c, **{k: None}) == (-1, "hbls_slot_select_batch: cand and cand_idx are required"), k
    # NULL where the count is zero is no error
    assert err(c, n=0, pks=None, sigs=None, msgs=None, off=None, ln=None, vst=None)[0] == 0
    assert err(c, G=0, src=None, idx=None, goff=None, dv=None, chosen=None, count=None, out=None, tst=None, ast=None)[0] == 0
    assert err(c, src=None, idx=None, goff=np.zeros(5, np.uint32))[0] == 0


# ---------------------------------------------------------------------------------------------
# 6 - 8: concurrent callers, the learned key cache, the caller mirror
# ---------------------------------------------------------------------------------------------
def test_concurrent_callers(L, base, base_host, two_roots, two_roots_host):
    """Four host threads with different inputs against the three host-call contexts."""
    jobs = [(base["clean", (7, 5)][0], base_host["clean", (7, 5)]), (base["skip", (7, 5)][0], base_host["skip", (7, 5)]),
            (base["edge", (7, 5)][0], base_host["edge", (7, 5)]), (two_roots[0], two_roots_host)]
    got, errs = [None] * len(jobs), []

    def work(k):
        try:
            for _ in range(2):
                got[k] = host(L, jobs[k][0])
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errs.append((k, repr(e)))

    th = [threading.Thread(target=work, args=(k,)) for k in range(len(jobs))]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs, errs
    for k, (_, want) in enumerate(jobs):
        same(got[k], want, k)


def test_learned_key_cache_serves_the_second_call(L, base, base_host):
    """The host path is the warm path: the second of two identical calls finds every pubshare and every
    DV key in the learned key cache."""
    c, want = base["clean", (7, 5)][0], base_host["clean", (7, 5)]
    n, G = len(c["pks"]), len(c["goff"]) - 1
    assert L.hbls_pubkey_cache_clear() == 0
    a = _lib.key_learn_stats(L)[0]
    same(host(L, c), want)
    b = _lib.key_learn_stats(L)[0]
    same(host(L, c), want)
    e = _lib.key_learn_stats(L)[0]
    assert b["misses"] - a["misses"] >= n + G and b["hits"] == a["hits"]
    assert e["hits"] - b["hits"] == n + G and e["misses"] == b["misses"]


def test_callers_sigagg_slot_host(L, ss, clusters, base, hipbls):
    from charon_amd import callers
    d = clusters[(7, 5)]
    V, n, t = 24, d["n"], d["t"]
    c = base["skip", (7, 5)][0]
    sigs, msgs = c["sigs"], c["msgs"]
    dv = [bytes(d["dv_pks"][48 * v:48 * v + 48]) for v in range(V + 1)]
    shares = {dv[v]: {k + 1: bytes(c["pks"][v * n + k]) for k in range(n)} for v in range(V + 1)}
    sets = {dv[v]: [callers.ParSig(k + 1, bytes(msgs[v * n + k]), bytes(sigs[v * n + k])) for k in range(n)]
            for v in range(V)}
    want = callers.sigagg_slot(hipbls, t, dict(zip(dv, dv)), shares, sets)
    got = callers.sigagg_slot_host(hipbls, t, dict(zip(dv, dv)), shares, sets)
    assert got == want
    assert all(got[1][dv[v]] == bytes(d["root_sigs"][96 * v:96 * v + 96]) for v in range(V))
    assert any(u != list(range(t)) for u in got[2].values())
    # a validator whose partials span two roots with neither reaching t: the duty fails as below threshold
    other = hashlib.sha256(b"another signing root").digest()
    sets[dv[V]] = [callers.ParSig(k + 1, other if k < 3 else bytes(msgs[V * n + k]), bytes(sigs[V * n + k])) for k in range(n)]
    with pytest.raises(callers.CallerError, match="^threshold aggregate: require threshold signatures$"):
        callers.sigagg_slot_host(L, t, dict(zip(dv, dv)), shares, sets)
