"""Host-side mirrors of charon's BLS call sites, switched to the batch entry points (SURVEY.md
§8(f)1 and §8(f)4).  Each function keeps the reference's error strings and reports the error the
reference's per-item loop would return first; only the per-item tbls calls are replaced by batch
calls.  INTEGRATION.md §3 gives the same changes as Go patches.

  parsigex_verify_set             core/parsigex/parsigex.go:93-98 + NewEth2Verifier :145-170
                                  (+ eth2util/signing/signing.go:96-115 zero-signature check)
  sigagg_aggregate                core/sigagg/sigagg.go:48-81 + aggregate :83-122 (TA :105, verify :117,
                                  NewVerifier :124-144)
  sigagg_slot                     parsigex.go:93-98 -> parsigdb/memory.go:198-225 -> sigagg.go:84-117 for one duty
                                  in ONE device call (hbls_slot_select_device): verify, pick verified members,
                                  aggregate, verify the aggregates
  sigagg_slot_host                the same duty through the host-buffer call the Go shim binds (hbls_slot_select_batch),
                                  under parsigdb's matching rule (memory.go:149-160, 197-225); numpy only
  ParSigDuty                      the same chain as the sets arrive: one duty session (hbls_duty_*), one call per
                                  peer's set, aggregates for the validators that reach the threshold through it
  validatorapi_submit             core/validatorapi/validatorapi.go:284-306 + verifyPartialSig :1213-1229
  lock_verify_signatures          cluster/lock.go:151-197 (VerifyAggregate over every pubshare, :185)
  dkg_agg_deposit_data            dkg/dkg.go:820-899 (n x Verify + ThresholdAggregate + Verify per DV)
  dkg_agg_validator_registrations dkg/dkg.go:901-984 (the same shape over registration roots)
  dkg_agg_lock_hash_sig           dkg/dkg.go:659-703 (Verify of every partial + plain Aggregate)
  dkg_verify_lock_multisig        dkg/dkg.go:595-598 (VerifyAggregate of that aggregate)
  exit_aggregate                  app/obolapi/exit.go:165-194 (ThresholdAggregate of the exit partials)
  exit_aggregate_batch            cmd/exit_fetch.go:120-137 --all: every validator's exit partials in one batch

First-error semantics.  The reference loops check item by item and return at the first failure.
A batch call verifies everything at once, so each mirror (i) runs the cheap per-item pre-checks
(lookups, lengths, zero signature) in loop order up to the first failing one, (ii) batches the
cryptographic checks of every item before it, and (iii) walks the loop order again, returning the
first error of either kind -- exactly the error the reference returns (for the Go map iterations,
exactly the error of that iteration order).

`impl` is any object with the batch methods of charon_amd.tbls.HIPBLS (verify_batch,
threshold_aggregate_batch, aggregate_batch, verify_aggregate_batch).  Messages are the 32-byte
signing roots the callers compute (eth2util/signing.GetDataRoot), or roots computed on the GPU by
charon_amd.signing_roots.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

from .tbls import TblsError, status_error

OK = 0
ZERO_SIG = bytes(96)
_LEN_ERR = "data is not of the correct length"  # tbls/tblsconv/tblsconv.go:46,66


class CallerError(TblsError):
    """The error a reference call site returns (wrapped message, as errors.Wrap prints it)."""


def _wrap(outer: str, inner: str) -> CallerError:
    return CallerError(f"{outer}: {inner}")


def _verr(st: int) -> str:
    return status_error("verify", st)


@dataclass
class ParSig:
    """core.ParSignedData reduced to what verification needs."""
    share_idx: int
    signing_root: bytes
    signature: bytes


def parsigex_verify_set(impl, pubshares_by_key: Mapping[bytes, Mapping[int, bytes]],
                        data_set: Sequence[Tuple[bytes, ParSig]]) -> None:
    """ParSigEx.handle's verification loop (parsigex.go:93-98) over a peer's whole set in one
    batch.  The first failing entry (in set order) aborts with the reference's error chain:
    "invalid partial signature: <NewEth2Verifier error>" (parsigex.go:96, :148-165)."""
    pks, msgs, sigs = [], [], []
    pre: Optional[str] = None
    for pubkey, ps in data_set:
        shares = pubshares_by_key.get(pubkey)
        if shares is None:
            pre = "unknown pubkey, not part of cluster lock"
            break
        pubshare = shares.get(ps.share_idx)
        if pubshare is None:
            pre = "invalid shareIdx"
            break
        if ps.signature == ZERO_SIG:  # signing.go:107-110, before tbls.Verify
            pre = "invalid signature: no signature found"
            break
        pks.append(pubshare)
        msgs.append(ps.signing_root)
        sigs.append(ps.signature)
    if pks and hasattr(impl, "verify_batch_first_error"):
        # the set up to its first failure (hbls_verify_batch_first_error): under attack the library
        # resolves only the first failing item instead of every item's verdict
        first, st = impl.verify_batch_first_error(pks, msgs, sigs)
        if first >= 0:
            raise _wrap("invalid partial signature", "invalid signature: " + _verr(st))
    else:
        for s in impl.verify_batch(pks, msgs, sigs) if pks else []:
            if s != OK:
                raise _wrap("invalid partial signature", "invalid signature: " + _verr(s))
    if pre is not None:
        raise _wrap("invalid partial signature", pre)


def sigagg_aggregate(impl, threshold: int, dv_pubkeys: Mapping[bytes, bytes],
                     sets: Mapping[bytes, Sequence[ParSig]]) -> Dict[bytes, bytes]:
    """Aggregator.Aggregate (sigagg.go:48-81): the validators' partials threshold-aggregated in one
    batch, then every aggregate verified under its DV key in one batch (sigagg.go:117,
    NewVerifier :124-144).  The first validator whose step fails aborts the duty set with
    "threshold aggregate: <error>" (sigagg.go:58)."""
    if not sets:
        raise CallerError("empty partial signed data set")
    keys = list(sets)
    groups: List[Dict[int, bytes]] = []
    pre: Optional[str] = None
    for pk in keys:  # aggregate()'s checks before the TA (sigagg.go:84-101)
        par = sets[pk]
        if len(par) < threshold:
            pre = "require threshold signatures"
            break
        by_idx: Dict[int, bytes] = {}
        for ps in par:
            if len(ps.signature) != 96:
                pre = "signature from core: " + _LEN_ERR
                break
            by_idx[ps.share_idx] = ps.signature
        if pre is not None:
            break
        if len(by_idx) < threshold:
            pre = "number of partial signatures less than threshold"
            break
        groups.append(by_idx)
    done = keys[:len(groups)]
    outs, sts = impl.threshold_aggregate_batch(groups) if groups else ([], [])
    ok = [k for k, s in enumerate(sts) if s == OK]
    vst = dict(zip(ok, impl.verify_batch([dv_pubkeys[done[k]] for k in ok],
                                         [sets[done[k]][0].signing_root for k in ok],
                                         [outs[k] for k in ok]))) if ok else {}
    for k in range(len(done)):
        if sts[k] != OK:
            raise _wrap("threshold aggregate", status_error("threshold_aggregate", sts[k]))
        if vst[k] != OK:
            raise _wrap("threshold aggregate", "aggregate signature verification failed: " + _verr(vst[k]))
    if pre is not None:
        raise _wrap("threshold aggregate", pre)
    return dict(zip(done, outs))


def sigagg_slot(impl_or_L, threshold: int, dv_pubkeys: Mapping[bytes, bytes],
                pubshares_by_key: Mapping[bytes, Mapping[int, bytes]], sets: Mapping[bytes, Sequence[ParSig]],
                device: int = 0):
    """One duty from the exchanged partials to the aggregates, as the node does it in three places:
    ParSigEx verifies every partial before it is stored (parsigex.go:93-98), the ParSigDB fires with
    the first `threshold` stored partials of a validator (parsigdb/memory.go:198-225), and the
    Aggregator aggregates exactly those and verifies the result under the DV key (sigagg.go:84-117).
    Here the whole duty is one hbls_slot_select_device call: sets[pubkey] lists the validator's
    partials in arrival order, every one is verified, and the first `threshold` that verify (one per
    share index) are aggregated -- a corrupted partial costs its operator's vote, not the
    validator's signature.

    Returns (statuses, aggregates, used): per validator the status of each of its partials (in set
    order), the 96-byte aggregate, and the positions in its set of the partials that were aggregated.
    The first validator (in set order) without an aggregate aborts the duty as Aggregator.Aggregate
    does: "threshold aggregate: require threshold signatures" (sigagg.go:86) when fewer than
    `threshold` of its partials verified, else the aggregation's or the aggregate verification's error.
    impl_or_L: a charon_amd.tbls.HIPBLS or the loaded library."""
    import ctypes

    import numpy as np
    import torch

    from . import _lib
    L = getattr(impl_or_L, "_L", impl_or_L)
    if not sets:
        raise CallerError("empty partial signed data set")
    keys = list(sets)
    roots, root_of = [], {}
    pks, sigs, midx, idx, goff = [], [], [], [], [0]
    for pk in keys:
        for ps in sets[pk]:
            if len(ps.signature) != 96:
                raise _wrap("threshold aggregate", "signature from core: " + _LEN_ERR)
            shares = pubshares_by_key.get(pk)
            if shares is None or ps.share_idx not in shares:
                raise _wrap("invalid partial signature",
                            "unknown pubkey, not part of cluster lock" if shares is None else "invalid shareIdx")
            if ps.signing_root not in root_of:
                root_of[ps.signing_root] = len(roots)
                roots.append(ps.signing_root)
            pks.append(shares[ps.share_idx])
            sigs.append(ps.signature)
            midx.append(root_of[ps.signing_root])
            idx.append(ps.share_idx)
        goff.append(len(pks))
    n, V, M = len(pks), len(keys), len(roots)
    dev = torch.device("cuda", device)

    def up(a):
        return torch.from_numpy(a).to(dev)

    def u8(chunks, width):
        return np.frombuffer(b"".join(chunks), dtype=np.uint8).copy() if chunks else np.zeros(width, dtype=np.uint8)

    g_msgs = up(u8(roots, 32))
    g_moff = up((np.arange(max(M, 1), dtype=np.int64) * 32))
    g_mlen = up(np.asarray([len(r) for r in roots] or [0], dtype=np.int32))
    g_pks, g_sigs = up(u8(pks, 48)), up(u8(sigs, 96))
    g_midx = up(np.asarray(midx or [0], dtype=np.int32))
    g_src = up(np.arange(max(n, 1), dtype=np.int32))
    g_idx = up(np.asarray(idx or [0], dtype=np.int64))
    g_goff = up(np.asarray(goff, dtype=np.int32))
    g_dv = up(u8([dv_pubkeys[pk] for pk in keys], 48))
    hm = torch.zeros(max(M, 1) * L.hbls_hm_entry_bytes(), dtype=torch.uint8, device=dev)
    vst = torch.full((max(n, 1),), 255, dtype=torch.uint8, device=dev)
    tout = torch.zeros(V * 96, dtype=torch.uint8, device=dev)
    tst = torch.full((V,), 255, dtype=torch.uint8, device=dev)
    ast = torch.full((V,), 255, dtype=torch.uint8, device=dev)
    chosen = torch.zeros(V * threshold, dtype=torch.int32, device=dev)
    count = torch.zeros(V, dtype=torch.int32, device=dev)
    # a validator's partials are consecutive, so when each validator signs one root (and has a
    # partial) the candidate offsets also serve as the verification groups; else every partial alone
    grouped = all(goff[k + 1] > goff[k] and len({ps.signing_root for ps in sets[pk]}) == 1
                  for k, pk in enumerate(keys))
    ptr = lambda x: x.data_ptr()  # noqa: E731
    slot = _lib.HblsSlot(msgs=ptr(g_msgs), msg_off=ptr(g_moff), msg_len=ptr(g_mlen), n_msgs=M, hm=ptr(hm),
                         pks=ptr(g_pks), sigs=ptr(g_sigs), msg_idx=ptr(g_midx), n=n,
                         vgrp_off=ptr(g_goff) if grouped else None, n_vgroups=V if grouped else n, vstatus=ptr(vst), ta_sigs=None, ta_src=ptr(g_src), ta_idx=ptr(g_idx),
                         grp_off=ptr(g_goff), n_groups=V, n_ta_partials=n, ta_out=ptr(tout), ta_status=ptr(tst),
                         dv_pks=ptr(g_dv), agg_vstatus=ptr(ast))
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    _lib.check(L.hbls_slot_select_device(ctypes.byref(slot), threshold, ctypes.c_void_p(ptr(chosen)),
                                         ctypes.c_void_p(ptr(count)), ctypes.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    vst_h, tst_h, ast_h = vst.cpu().numpy(), tst.cpu().numpy(), ast.cpu().numpy()
    out_h = tout.cpu().numpy().reshape(V, 96)
    chosen_h = chosen.cpu().numpy().view(np.uint32).reshape(V, threshold)
    count_h = count.cpu().numpy()
    statuses = {pk: [int(x) for x in vst_h[goff[k]:goff[k + 1]]] for k, pk in enumerate(keys)}
    used = {pk: [int(c) - goff[k] for c in chosen_h[k, :count_h[k]]] for k, pk in enumerate(keys)}
    for k in range(V):
        if tst_h[k] == _lib.UNCHECKED:
            raise _wrap("threshold aggregate", "require threshold signatures")
        if tst_h[k] == _lib.BAD_INPUT:
            raise _wrap("threshold aggregate", "partial signatures over different signing roots")
        if tst_h[k] != OK:
            raise _wrap("threshold aggregate", status_error("threshold_aggregate", int(tst_h[k])))
        if ast_h[k] != OK:
            raise _wrap("threshold aggregate", "aggregate signature verification failed: " + _verr(int(ast_h[k])))
    return statuses, {pk: bytes(out_h[k]) for k, pk in enumerate(keys)}, used


def sigagg_slot_host(impl_or_L, threshold: int, dv_pubkeys: Mapping[bytes, bytes],
                     pubshares_by_key: Mapping[bytes, Mapping[int, bytes]], sets: Mapping[bytes, Sequence[ParSig]]):
    """sigagg_slot through the host-buffer entry point the Go shim calls (hbls_slot_select_batch):
    the same contract -- arguments, the (statuses, aggregates, used) it returns, the errors and their
    order -- over numpy arrays only, with no torch and no device memory of the caller's.

    One difference follows from the entry point: its members follow the ParSigDB's matching rule
    (parsigdb/memory.go:197-225), which groups a validator's stored partials by signing root and
    fires for the first root to hold `threshold` of them.  A validator whose partials span several
    roots is therefore aggregated over the winning root, or fails with "require threshold
    signatures" when no root gets there; the "partial signatures over different signing roots" error
    of sigagg_slot cannot arise here.
    impl_or_L: a charon_amd.tbls.HIPBLS or the loaded library."""
    import ctypes

    import numpy as np

    from . import _lib
    L = getattr(impl_or_L, "_L", impl_or_L)
    if not sets:
        raise CallerError("empty partial signed data set")
    keys = list(sets)
    pks, sigs, msgs, idx, goff = [], [], [], [], [0]
    for pk in keys:
        for ps in sets[pk]:
            if len(ps.signature) != 96:
                raise _wrap("threshold aggregate", "signature from core: " + _LEN_ERR)
            shares = pubshares_by_key.get(pk)
            if shares is None or ps.share_idx not in shares:
                raise _wrap("invalid partial signature",
                            "unknown pubkey, not part of cluster lock" if shares is None else "invalid shareIdx")
            pks.append(shares[ps.share_idx])
            sigs.append(ps.signature)
            msgs.append(ps.signing_root)
            idx.append(ps.share_idx)
        goff.append(len(pks))
    n, V = len(pks), len(keys)

    def u8(chunks):
        return np.frombuffer(b"".join(chunks) or bytes(1), dtype=np.uint8).copy()

    a_pks, a_sigs, a_msgs, a_dv = u8(pks), u8(sigs), u8(msgs), u8([dv_pubkeys[pk] for pk in keys])
    a_len = np.asarray([len(m) for m in msgs] or [0], dtype=np.uint32)
    a_off = (np.cumsum(a_len, dtype=np.uint64) - a_len).astype(np.uint64)
    a_cand = np.arange(max(n, 1), dtype=np.uint32)
    a_idx = np.asarray(idx or [0], dtype=np.int64)
    a_goff = np.asarray(goff, dtype=np.uint32)
    vst = np.full(max(n, 1), 255, dtype=np.uint8)
    chosen = np.zeros(V * threshold, dtype=np.uint32)
    count = np.zeros(V, dtype=np.uint32)
    out = np.zeros(V * 96, dtype=np.uint8)
    tst, ast = np.full(V, 255, dtype=np.uint8), np.full(V, 255, dtype=np.uint8)
    p = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    if L.hbls_slot_select_batch(p(a_pks), p(a_sigs), p(a_msgs), p(a_off), p(a_len), n, p(a_cand), p(a_idx), p(a_goff), V,
                                p(a_dv), threshold, p(vst), p(chosen), p(count), p(out), p(tst), p(ast)) != 0:
        raise _lib.HipBlsRuntimeError("hipbls: " + L.hbls_last_error().decode(errors="replace"))
    chosen, out = chosen.reshape(V, threshold), out.reshape(V, 96)
    statuses = {pk: [int(x) for x in vst[goff[k]:goff[k + 1]]] for k, pk in enumerate(keys)}
    used = {pk: [int(c) - goff[k] for c in chosen[k, :count[k]]] for k, pk in enumerate(keys)}
    for k in range(V):
        if tst[k] == _lib.UNCHECKED:
            raise _wrap("threshold aggregate", "require threshold signatures")
        if tst[k] != OK:
            raise _wrap("threshold aggregate", status_error("threshold_aggregate", int(tst[k])))
        if ast[k] != OK:
            raise _wrap("threshold aggregate", "aggregate signature verification failed: " + _verr(int(ast[k])))
    return statuses, {pk: bytes(out[k]) for k, pk in enumerate(keys)}, used


class Cluster:
    """The cluster lock as an object of the library (hbls_cluster_open): every validator's DV key and
    its pubshares of share indices 1 .. n, decompressed, subgroup-checked and (ladder_tables) given
    ladder tables once, resident on the device for as long as the handle -- or a duty opened on it --
    lives.  dv_pubkeys: {validator pubkey: DV key bytes} in cluster order; pubshares_by_key: {validator
    pubkey: {share index: pubshare}} with the same indices 1 .. n for every validator.  A context
    manager; ParSigDuty(..., cluster=this) opens duties that pass no keys.  `key_status`: per validator
    the statuses of its 1 + n keys (DV key first) -- a bad key does not fail the open, every partial
    that names it gets BAD_PUBKEY."""

    def __init__(self, impl, dv_pubkeys: Mapping[bytes, bytes], pubshares_by_key: Mapping[bytes, Mapping[int, bytes]],
                 ladder_tables: bool = True):
        import ctypes

        self.keys = list(dv_pubkeys)
        self.dv_pubkeys, self.pubshares_by_key = dv_pubkeys, pubshares_by_key
        self.n_validators = len(self.keys)
        self.n_shares = max((max(pubshares_by_key[pk]) for pk in self.keys), default=1)
        for pk in self.keys:
            if sorted(pubshares_by_key[pk]) != list(range(1, self.n_shares + 1)):
                raise TblsError("cluster: every validator needs the pubshares of share indices 1 .. n")
        dv = b"".join(bytes(dv_pubkeys[pk]) for pk in self.keys)
        sh = b"".join(bytes(pubshares_by_key[pk][j]) for pk in self.keys for j in range(1, self.n_shares + 1))
        if len(dv) != 48 * self.n_validators or len(sh) != 48 * self.n_validators * self.n_shares:
            raise TblsError("cluster: " + _LEN_ERR)
        self._L = impl._L
        row = 1 + self.n_shares
        st = ctypes.create_string_buffer(max(self.n_validators * row, 1))
        h = ctypes.c_uint64(0)
        if self._L.hbls_cluster_open(ctypes.create_string_buffer(dv, max(len(dv), 1)),
                                     ctypes.create_string_buffer(sh, max(len(sh), 1)), self.n_validators, self.n_shares,
                                     1 if ladder_tables else 0, st, ctypes.byref(h)) != 0:
            raise TblsError("hipbls: " + self._L.hbls_last_error().decode(errors="replace"))
        self._h: Optional[int] = h.value
        self.key_status = [list(st.raw[g * row:(g + 1) * row]) for g in range(self.n_validators)]

    def __enter__(self) -> "Cluster":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def handle(self) -> int:
        if self._h is None:
            raise TblsError("the cluster is closed")
        return self._h

    def stats(self) -> Dict[str, int]:
        import ctypes

        out = (ctypes.c_uint64 * 6)()
        if self._L.hbls_cluster_stats(self.handle(), out, 6) != 0:
            raise TblsError("hipbls: " + self._L.hbls_last_error().decode(errors="replace"))
        return dict(zip(("keys", "bad_keys", "ladder_tables", "partials_resolved", "partials_no_key", "dv_keys_resolved"),
                        (int(x) for x in out)))

    def check(self, threshold: int) -> Tuple[List[int], List[int]]:
        """hbls_cluster_check: do every validator's pubshares interpolate to its DV key under
        `threshold` -> (row_status, row_windows), one entry per validator in cluster order.  Status OK:
        consistent; BAD_PUBKEY: one of the row's keys has a non-zero key_status (nothing computed,
        windows 0); NOT_VERIFIED: bit k of the row's windows is set iff the threshold-th forward
        difference over its keys k .. k + threshold (0: the DV key, j: the pubshare of share index j)
        does not vanish.  Only reads the cluster."""
        import ctypes

        st = ctypes.create_string_buffer(max(self.n_validators, 1))
        win = (ctypes.c_uint64 * max(self.n_validators, 1))()
        if self._L.hbls_cluster_check(self.handle(), threshold, st, win, None) != 0:
            raise TblsError("hipbls: " + self._L.hbls_last_error().decode(errors="replace"))
        return list(st.raw[:self.n_validators]), [int(w) for w in win[:self.n_validators]]

    def inconsistent(self, threshold: int) -> Dict[bytes, Tuple[int, List[int], List[int]]]:
        """The validators check(threshold) does not report OK: {validator pubkey: (status, failing
        windows, candidate positions)}; empty for a consistent lock.  The candidates
        (lock_check_candidates) are a single wrong key's position where the windows determine it:
        0 the DV key, j the pubshare of share index j."""
        status, windows = self.check(threshold)
        W = self.n_shares - threshold + 1
        return {pk: (st, [k for k in range(W) if (w >> k) & 1], lock_check_candidates(self.n_shares, threshold, w))
                for pk, st, w in zip(self.keys, status, windows) if st != OK}

    def check_stats(self) -> Dict[str, int]:
        import ctypes

        out = (ctypes.c_uint64 * 2)()
        if self._L.hbls_cluster_check_stats(self.handle(), out, 2) != 0:
            raise TblsError("hipbls: " + self._L.hbls_last_error().decode(errors="replace"))
        return dict(zip(("checks", "rows_not_verified"), (int(x) for x in out)))

    def verify(self, items: Sequence[Tuple[bytes, int, bytes, bytes]]) -> List[int]:
        """hbls_cluster_verify_batch: items of (validator pubkey, key index, message, signature), each
        verified under the lock key it names -- key index 0 the validator's DV key, j in 1 .. n its
        pubshare of share index j -> the statuses.  A validator pubkey that is not in the cluster is sent
        with a group at or above n_validators, so the library itself answers BAD_PUBKEY (as it does for a
        key index that names no key).  Only reads the cluster."""
        import ctypes

        n = len(items)
        if not n:
            return []
        row = {pk: g for g, pk in enumerate(self.keys)}
        msgs = b"".join(bytes(m) for _, _, m, _ in items)
        sigs = b"".join(bytes(s) for _, _, _, s in items)
        if len(sigs) != 96 * n:
            raise TblsError("cluster verify: " + _LEN_ERR)
        group = (ctypes.c_uint32 * n)(*[row.get(pk, self.n_validators) for pk, _, _, _ in items])
        idx = (ctypes.c_int64 * n)(*[int(j) for _, j, _, _ in items])
        length = (ctypes.c_uint32 * n)(*[len(m) for _, _, m, _ in items])
        off = (ctypes.c_uint64 * n)()
        for i in range(1, n):
            off[i] = off[i - 1] + length[i - 1]
        st = ctypes.create_string_buffer(n)
        if self._L.hbls_cluster_verify_batch(self.handle(), group, idx, ctypes.create_string_buffer(sigs, len(sigs)),
                                             ctypes.create_string_buffer(msgs, max(len(msgs), 1)), off, length, n, st) != 0:
            raise TblsError("hipbls: " + self._L.hbls_last_error().decode(errors="replace"))
        return list(st.raw[:n])

    def verify_aggregate(self, signature: bytes, message: bytes, shares: Optional[Sequence[int]] = None,
                         with_dv: bool = False) -> int:
        """hbls_cluster_verify_aggregate: FastAggregateVerify of one signature over one message under the
        sum of every validator's selected keys -> the status.  shares: the share indices whose pubshares
        are selected (None: all of them); with_dv: the DV keys as well.  Only reads the cluster."""
        import ctypes

        if len(signature) != 96:
            raise TblsError("cluster verify aggregate: " + _LEN_ERR)
        mask = 0
        for j in range(1, self.n_shares + 1) if shares is None else shares:
            if j < 1 or j > 64:
                raise TblsError("cluster verify aggregate: a share index is 1 .. 64")
            mask |= 1 << (j - 1)
        st = ctypes.create_string_buffer(1)
        if self._L.hbls_cluster_verify_aggregate(self.handle(), mask, 1 if with_dv else 0,
                                                 ctypes.create_string_buffer(bytes(signature), 96),
                                                 ctypes.create_string_buffer(bytes(message), max(len(message), 1)),
                                                 len(message), st) != 0:
            raise TblsError("hipbls: " + self._L.hbls_last_error().decode(errors="replace"))
        return st.raw[0]

    def verify_lock_signatures(self, signature_aggregate: bytes, lock_hash: bytes,
                               registrations: Optional[Mapping[bytes, Tuple[bytes, bytes]]] = None) -> None:
        """The BLS part of Lock.VerifySignatures (lock.go:151-196) on the open cluster.  First the
        aggregate over every validator's every pubshare against the lock hash (lock.go:185), its error
        wrapped as lock_verify_signatures wraps it; then `registrations`, {validator pubkey: (signing
        root, signature)}, in cluster order under the DV keys (verifyBuilderRegistrations, lock.go:235-281):
        the first failing one is raised as lock.go:190 and :274-276 wrap the tbls.Verify error."""
        st = self.verify_aggregate(signature_aggregate, lock_hash)
        if st != OK:
            raise _wrap("verify lock signature aggregate", status_error("verify_aggregate", st))
        if not registrations:
            return
        regs = [(pk,) + tuple(registrations[pk]) for pk in self.keys if pk in registrations]
        for s in self.verify([(pk, 0, root, sig) for pk, root, sig in regs]):
            if s != OK:
                raise _wrap("verify pre-generated builder registrations", "verify builder registration signature: " + _verr(s))

    def verify_stats(self) -> Dict[str, int]:
        import ctypes

        out = (ctypes.c_uint64 * 5)()
        if self._L.hbls_cluster_verify_stats(self.handle(), out, 5) != 0:
            raise TblsError("hipbls: " + self._L.hbls_last_error().decode(errors="replace"))
        return dict(zip(("verify_calls", "items_resolved", "items_no_key", "aggregate_calls", "aggregate_keys"),
                        (int(x) for x in out)))

    def close(self) -> None:
        """Invalidates the handle; the device memory goes with the last duty opened on the cluster."""
        if self._h is not None:
            h, self._h = self._h, None
            if self._L.hbls_cluster_close(h) != 0:
                raise TblsError("hipbls: " + self._L.hbls_last_error().decode(errors="replace"))


def lock_check_candidates(n_shares: int, threshold: int, windows: int) -> List[int]:
    """The positions 0 .. n_shares of a row (0: the DV key, j: the pubshare of share index j) that lie in
    every failing window of hbls_cluster_check's mask `windows` and in no passing one; window k holds the
    positions k .. k + threshold.  One wrong key at p fails exactly the windows with k <= p <= k +
    threshold, so p is always among its own mask's candidates, and alone wherever the windows
    determine it; no failing window, or failures no single position explains, give []."""
    W = n_shares - threshold + 1
    if not 1 <= threshold <= n_shares or windows >> W:
        raise TblsError("lock check: threshold must be in 1 .. n_shares and the mask within its windows")
    if not windows:
        return []
    return [p for p in range(n_shares + 1)
            if all(((windows >> k) & 1) == (1 if k <= p <= k + threshold else 0) for k in range(W))]


class ParSigDuty:
    """ParSigEx.handle -> MemDB.StoreExternal -> Aggregator.Aggregate for ONE duty under the
    reference's arrival pattern (parsigex.go:93-98, parsigdb/memory.go:80-123 and 197-225,
    sigagg.go:84-117): every peer's set is one call of a duty session (hbls_duty_add), which verifies
    it, stores what the ParSigDB would store, and aggregates the validators that reach the threshold
    through this very set from the partials resident on the device.

    store_external(set) takes a peer's {pubkey: ParSig} and returns {pubkey: aggregate} for the
    validators that fired; it raises the reference's error chain as sigagg_slot_host does: the first
    entry of the set (in set order) that fails its pre-checks or its verification aborts with
    "invalid partial signature: ..." (parsigex.go:96), a fired validator whose aggregation or
    aggregate verification fails with "threshold aggregate: ..." (sigagg.go:105-119).  A context
    manager: close() frees the device state, where MemDB.Trim deletes the duty.

    reject_sets: False admits a set's partials one by one (hbls_duty_add; see store_external on what
    a set with a failing entry then leaves behind).  True gives the reference's rule exactly
    (hbls_duty_add_sets): a set with an entry that fails verification stores nothing, fires nothing
    and leaves the duty as it was.  store_external_many(sets) takes several peers' sets in one call,
    each with that all-or-nothing boundary of its own, whatever reject_sets is.
    first_error: the calls that go through sets (reject_sets=True, store_external_many) stop a rejected
    set's verification at its first failing entry, as parsigex.go:93-98 does (hbls_duty_add_sets_first):
    the same results and errors -- the error of a rejected set is that of its first failing entry,
    whose status is exact -- at a cost that does not grow with the number of bad entries.
    cluster: an open Cluster -- the duty is opened on it (hbls_duty_open_cluster) and passes no keys: the
    device resolves each partial's key from (validator, share index) and verifies the aggregates under
    the cluster's DV keys.  dv_pubkeys and pubshares_by_key may then be None (the cluster's are used for
    the pre-checks, which stay the shim's own and keep their two error strings).
    The ONE place where a cluster duty still passes keys: a set with a failing pre-check.  The reference's
    loop verifies the entries in front of that entry before it returns the pre-check's error, so a
    failing signature among them wins.  A plain duty sends them as partials of no group ("verify only");
    a cluster duty has no such partial (a group of no validator names no key), so they go through one
    impl.verify_batch under the pubshares the pre-checks found (_verify_only), beside the duty, and
    store_external_many sends that set in empty.  Nothing of it is stored either way."""

    def __init__(self, impl, threshold: int, dv_pubkeys: Optional[Mapping[bytes, bytes]] = None,
                 pubshares_by_key: Optional[Mapping[bytes, Mapping[int, bytes]]] = None, max_stored: int = 16,
                 reject_sets: bool = False, first_error: bool = False, cluster: Optional["Cluster"] = None):
        self._reject_sets = reject_sets
        self._first_error = first_error
        self._cluster = cluster
        self._impl = impl
        if cluster is not None:
            dv_pubkeys, pubshares_by_key = cluster.dv_pubkeys, cluster.pubshares_by_key
        self._keys = list(dv_pubkeys)
        self._group = {pk: g for g, pk in enumerate(self._keys)}
        self._shares = pubshares_by_key
        if cluster is not None:
            self._duty = impl.duty_open((), threshold, max_stored, cluster=cluster)
        else:
            self._duty = impl.duty_open([dv_pubkeys[pk] for pk in self._keys], threshold, max_stored)

    def __enter__(self) -> "ParSigDuty":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def close(self) -> None:
        self._duty.close()

    def state(self):
        cnt, fired = self._duty.state()
        return {pk: (cnt[g], fired[g]) for g, pk in enumerate(self._keys)}

    def store_external_many(self, sets: Sequence[Mapping[bytes, ParSig]]) -> List[object]:
        """Several peers' sets, in arrival order, as ONE hbls_duty_add_sets call (first_error:
        hbls_duty_add_sets_first).  Per set, what
        ParSigEx.handle + StoreExternal would have given for it: {pubkey: aggregate} of the validators
        that fired through it (a fired validator belongs to the set that holds its last member), or the
        CallerError the reference would have returned -- not raised: a rejected set does not stop the
        sets behind it, which are stored and fire.  An error of the aggregation stage carries the set's
        other aggregates as `fired`; a rejected set's error carries an empty one."""
        pks, msgs, sigs, groups, idx, set_off, pres = [], [], [], [], [], [0], []
        only: Dict[int, Optional[int]] = {}  # a cluster duty: sets verified beside the call -> first failing status
        for j, signed_set in enumerate(sets):
            p, m, s, g, x, pre = self._checked(signed_set)
            if pre is not None and self._cluster is not None:
                # a cluster duty has no "verify only" group (a group of no validator names no key): the
                # entries before the failing one are verified beside the call, and the set goes in empty
                bad = [st for st in self._verify_only(p, m, s, x).vstatus if st != OK] if p else []
                only[j] = bad[0] if bad else None
                p, m, s, g, x = [], [], [], [], []
            elif pre is not None:  # the entries before the failing one are verified only
                g = [0xFFFFFFFF] * len(p)
            pks += p
            msgs += m
            sigs += s
            groups += g
            idx += x
            set_off.append(len(pks))
            pres.append(pre)
        add = self._duty.add_sets_first if self._first_error else self._duty.add_sets
        r = add(None if self._cluster is not None else pks, msgs, sigs, groups, idx, set_off)
        res: List[object] = []
        for j, pre in enumerate(pres):
            b, e = set_off[j], set_off[j + 1]
            if r.set_first[j] is not None or only.get(j) is not None:
                # the verification loop runs first in the reference: its error wins
                st = only[j] if only.get(j) is not None else r.vstatus[r.set_first[j]]
                err = _wrap("invalid partial signature", "invalid signature: " + _verr(st))
                err.fired = {}
                res.append(err)
                continue
            if pre is not None:
                err = _wrap("invalid partial signature", pre)
                err.fired = {}
                res.append(err)
                continue
            out: Dict[bytes, bytes] = {}
            err = None
            for k, g in enumerate(r.fired):
                if not b <= r.chosen[k][-1] - r.first_serial < e:
                    continue
                if r.ta_status[k] != OK:
                    err = err or _wrap("threshold aggregate", status_error("threshold_aggregate", int(r.ta_status[k])))
                elif r.agg_vstatus[k] != OK:
                    err = err or _wrap("threshold aggregate",
                                       "aggregate signature verification failed: " + _verr(int(r.agg_vstatus[k])))
                else:
                    out[self._keys[g]] = r.aggregates[k]
            if err is not None:
                err.fired = out
                res.append(err)
            else:
                res.append(out)
        return res

    def _verify_only(self, pks, msgs, sigs, idx):
        """The entries in front of a set's failing pre-check, verified and not stored: partials of no
        group on a plain duty; on a cluster duty, where a group of no validator names no key, one
        Verify batch under the pubshares the pre-checks found.  `.vstatus` either way."""
        if self._cluster is None:
            return self._duty.add(pks, msgs, sigs, [0xFFFFFFFF] * len(pks), idx)
        from types import SimpleNamespace
        return SimpleNamespace(vstatus=list(self._impl.verify_batch(pks, msgs, sigs)))

    def _checked(self, signed_set: Mapping[bytes, ParSig]):
        """The pre-checks of a set in set order, up to the first failing one: the entries that passed
        (public shares, roots, signatures, groups, share indices) and that failure's text, or None."""
        pks, msgs, sigs, groups, idx = [], [], [], [], []
        pre: Optional[str] = None
        for pk, ps in signed_set.items():
            shares = self._shares.get(pk)
            if shares is None or pk not in self._group:
                pre = "unknown pubkey, not part of cluster lock"
            elif ps.share_idx not in shares:
                pre = "invalid shareIdx"
            elif len(ps.signature) != 96:
                pre = "signature from core: " + _LEN_ERR
            elif ps.signature == ZERO_SIG:
                pre = "invalid signature: no signature found"  # signing.go:107-110
            if pre is not None:
                break
            pks.append(shares[ps.share_idx])
            msgs.append(ps.signing_root)
            sigs.append(ps.signature)
            groups.append(self._group[pk])
            idx.append(ps.share_idx)
        return pks, msgs, sigs, groups, idx, pre

    def store_external(self, signed_set: Mapping[bytes, ParSig]) -> Dict[bytes, bytes]:
        if self._reject_sets:
            res = self.store_external_many([signed_set])[0]
            if isinstance(res, CallerError):
                raise res
            return res
        pks, msgs, sigs, groups, idx = [], [], [], [], []
        pre: Optional[str] = None
        for pk, ps in signed_set.items():  # the pre-checks in set order, up to the first failing one
            shares = self._shares.get(pk)
            if shares is None or pk not in self._group:
                pre = "unknown pubkey, not part of cluster lock"
            elif ps.share_idx not in shares:
                pre = "invalid shareIdx"
            elif len(ps.signature) != 96:
                pre = "signature from core: " + _LEN_ERR
            elif ps.signature == ZERO_SIG:
                pre = "invalid signature: no signature found"  # signing.go:107-110
            if pre is not None:
                break
            pks.append(shares[ps.share_idx])
            msgs.append(ps.signing_root)
            sigs.append(ps.signature)
            groups.append(self._group[pk])
            idx.append(ps.share_idx)
        if pre is not None or not pks:
            # nothing of a set with a failing entry is stored (parsigex.go:93-98 returns before StoreExternal):
            # the entries before it are verified only, for the error the reference's loop returns first
            if pks:
                r = self._verify_only(pks, msgs, sigs, idx)
                for st in r.vstatus:
                    if st != OK:
                        raise _wrap("invalid partial signature", "invalid signature: " + _verr(st))
            if pre is not None:
                raise _wrap("invalid partial signature", pre)
            return {}
        # One call verifies and stores.  Where an entry fails verification the reference drops the whole
        # set (handle returns before StoreExternal); the session has by then stored the set's verified
        # entries, each of which is a partial the ParSigDB would accept from that peer on its own.
        # The error then carries, as `fired`, the aggregates of the validators those entries brought to the
        # threshold: they fire once, so the caller must not lose them.  (reject_sets=True closes this
        # divergence: there the set is one set of hbls_duty_add_sets and is stored whole or not at all.)
        r = self._duty.add(None if self._cluster is not None else pks, msgs, sigs, groups, idx)
        out: Dict[bytes, bytes] = {}
        err: Optional[CallerError] = None
        for k, g in enumerate(r.fired):
            if r.ta_status[k] != OK:
                err = err or _wrap("threshold aggregate", status_error("threshold_aggregate", int(r.ta_status[k])))
            elif r.agg_vstatus[k] != OK:
                err = err or _wrap("threshold aggregate",
                                   "aggregate signature verification failed: " + _verr(int(r.agg_vstatus[k])))
            else:
                out[self._keys[g]] = r.aggregates[k]
        for st in r.vstatus:  # the verification loop runs first in the reference: its error wins
            if st != OK:
                err = _wrap("invalid partial signature", "invalid signature: " + _verr(st))
                break
        if err is not None:
            err.fired = out
            raise err
        return out


def validatorapi_submit(impl, pubshare_of: Mapping[bytes, bytes],
                        submissions: Sequence[Tuple[bytes, bytes, bytes]]) -> None:
    """Component.SubmitAttestations (validatorapi.go:284-306): the local VC's partials
    (pubkey, signing root, signature) verified in one batch before any set reaches the
    subscribers; the first failing attestation's error is returned as verifyPartialSig returns it
    (validatorapi.go:1213-1229: "unknown public key" from getVerifyShareFunc :121-125, "no signature
    found" from signing.Verify, else the tbls.Verify error)."""
    pks, msgs, sigs = [], [], []
    pre: Optional[str] = None
    for pubkey, root, sig in submissions:
        pubshare = pubshare_of.get(pubkey)
        if pubshare is None:
            pre = "unknown public key"
            break
        if sig == ZERO_SIG:
            pre = "no signature found"
            break
        pks.append(pubshare)
        msgs.append(root)
        sigs.append(sig)
    for s in impl.verify_batch(pks, msgs, sigs) if pks else []:
        if s != OK:
            raise CallerError(_verr(s))
    if pre is not None:
        raise CallerError(pre)


def lock_verify_signatures(impl, public_shares: Sequence[bytes], signature_aggregate: bytes,
                           lock_hash: bytes) -> None:
    """Lock.VerifySignatures' aggregate check (lock.go:165-189): VerifyAggregate over every
    validator's every public share against the lock hash."""
    st = impl.verify_aggregate_batch([list(public_shares)], [signature_aggregate], [lock_hash])[0]
    if st != OK:
        raise _wrap("verify lock signature aggregate", status_error("verify_aggregate", st))


def _dkg_partials(pubshares_by_dv, partials, roots, what: str, missing_msg: Optional[str],
                  sig_ctx: str = "signature from core"):
    """The DKG loops' per-partial pre-checks in loop order (dkg.go:838-869 / :919-950 / :665-682),
    up to the first failure.  Returns (checked items [(dv index, pubshare, root, sig)], complete DVs,
    the first pre-check error or None)."""
    items, complete = [], 0
    for d, dv in enumerate(partials):
        if missing_msg is not None and dv not in roots:
            return items, complete, missing_msg
        for ps in partials[dv]:
            if len(ps.signature) != 96:
                return items, complete, f"{sig_ctx}: {_LEN_ERR}"
            shares = pubshares_by_dv.get(dv)
            if shares is None:
                return items, complete, f"invalid pubkey in {what} partial signature from peer"
            if ps.share_idx not in shares:
                return items, complete, "invalid pubshare"
            items.append((d, shares[ps.share_idx], roots[dv] if roots is not None else ps.signing_root,
                          ps.signature))
        complete = d + 1
    return items, complete, None


def _dkg_threshold_aggregate(impl, pubshares_by_dv, partials, roots, what, missing_msg, agg_err, verify_what=None):
    """aggDepositData / aggValidatorRegistrations (dkg.go:820-899, :901-984) batched: every checked
    partial verified (one batch), every complete DV threshold-aggregated (one batch), every aggregate
    verified under the DV key (one batch); then the first error in the reference's loop order."""
    keys = list(partials)
    items, complete, pre = _dkg_partials(pubshares_by_dv, partials, roots, what, missing_msg)
    vst = impl.verify_batch([p for _, p, _, _ in items], [m for _, _, m, _ in items],
                            [s for _, _, _, s in items]) if items else []
    groups = [{ps.share_idx: ps.signature for ps in partials[keys[d]]} for d in range(complete)]
    outs, tst = impl.threshold_aggregate_batch(groups) if groups else ([], [])
    ok = [d for d in range(complete) if tst[d] == OK]
    ast = dict(zip(ok, impl.verify_batch([keys[d] for d in ok], [roots[keys[d]] for d in ok],
                                         [outs[d] for d in ok]))) if ok else {}
    k = 0
    for d in range(len(keys)):
        while k < len(items) and items[k][0] == d:
            if vst[k] != OK:  # errors.New: the herumi error is not wrapped (dkg.go:866-868)
                raise CallerError(f"invalid {verify_what or what} partial signature from peer")
            k += 1
        if d >= complete:
            break
        if tst[d] != OK:
            raise CallerError(status_error("threshold_aggregate", tst[d]))
        if ast[d] != OK:
            raise _wrap(agg_err, _verr(ast[d]))
    if pre is not None:
        raise CallerError(pre)
    return dict(zip(keys, outs))


def dkg_agg_deposit_data(impl, pubshares_by_dv: Mapping[bytes, Mapping[int, bytes]],
                         partials: Mapping[bytes, Sequence[ParSig]],
                         signing_roots: Mapping[bytes, bytes]) -> Dict[bytes, bytes]:
    """aggDepositData (dkg.go:820-899); signing_roots[dv] = deposit.GetMessageSigningRoot of the
    DV's deposit message (dkg.go:836).  Returns the aggregate signature per DV."""
    return _dkg_threshold_aggregate(impl, pubshares_by_dv, partials, signing_roots, "deposit data",
                                    "deposit message not found", "invalid deposit data aggregated signature")


def dkg_agg_validator_registrations(impl, pubshares_by_dv: Mapping[bytes, Mapping[int, bytes]],
                                    partials: Mapping[bytes, Sequence[ParSig]],
                                    signing_roots: Mapping[bytes, bytes]) -> Dict[bytes, bytes]:
    """aggValidatorRegistrations (dkg.go:901-984); signing_roots[dv] =
    registration.GetMessageSigningRoot of the DV's registration (dkg.go:917).  Returns the
    aggregate signature per DV (setRegistrationSignature's input, dkg.go:974)."""
    # the key lookup says "registrations", the partial check "registration" (dkg.go:938, :956)
    return _dkg_threshold_aggregate(impl, pubshares_by_dv, partials, signing_roots, "validator registrations",
                                    "validator registration not found",
                                    "invalid validator registration aggregated signature", "validator registration")


def dkg_agg_lock_hash_sig(impl, pubshares_by_dv: Mapping[bytes, Mapping[int, bytes]],
                          partials: Mapping[bytes, Sequence[ParSig]], lock_hash: bytes) -> Tuple[bytes, List[bytes]]:
    """aggLockHashSig (dkg.go:659-703): every node's lock-hash partial of every DV verified (one
    batch; the error wraps the tbls error, "invalid lock hash partial signature from peer: ..."),
    then ONE plain BLS aggregate of all of them.  Returns (aggregate, the pubshares in order)."""
    items, _, pre = _dkg_partials(pubshares_by_dv, partials, None, "lock hash", None, "signature from bytes")
    vst = impl.verify_batch([p for _, p, _, _ in items], [lock_hash] * len(items),
                            [s for _, _, _, s in items]) if items else []
    for s in vst:
        if s != OK:
            raise _wrap("invalid lock hash partial signature from peer", _verr(s))
    if pre is not None:
        raise CallerError(pre)
    outs, sts = impl.aggregate_batch([[s for _, _, _, s in items]])
    if sts[0] != OK:
        raise _wrap("bls aggregate Signatures", status_error("aggregate", sts[0]))
    return outs[0], [p for _, p, _, _ in items]


def dkg_verify_lock_multisig(impl, pubkeys: Sequence[bytes], agg_sig: bytes, lock_hash: bytes) -> None:
    """signAndAggLockHash's check of that aggregate (dkg.go:595-598)."""
    st = impl.verify_aggregate_batch([list(pubkeys)], [agg_sig], [lock_hash])[0]
    if st != OK:
        raise _wrap("verify multisignature", status_error("verify_aggregate", st))


def exit_aggregate(impl, partial_sigs: Sequence[Optional[bytes]]) -> bytes:
    """The exit blob's aggregation (app/obolapi/exit.go:165-194): entry i is share i+1's partial
    signature or None (not pushed yet, ignored)."""
    group = {}
    for i, s in enumerate(partial_sigs):
        if not s:
            continue
        if len(s) != 96:
            raise _wrap("invalid partial signature", _LEN_ERR)
        group[i + 1] = s
    outs, sts = impl.threshold_aggregate_batch([group])
    if sts[0] != OK:
        raise _wrap("partial signatures threshold aggregate", status_error("threshold_aggregate", sts[0]))
    return outs[0]


def exit_aggregate_batch(impl, validators: Sequence[Tuple[str, Sequence[Optional[bytes]]]]) -> List[bytes]:
    """`charon exit fetch --all` (cmd/exit_fetch.go:120-137) with INTEGRATION.md's
    AggregateFullExits: every validator's fetched exit partials (entry i = share i+1's signature or
    None) threshold-aggregated in ONE batch; the first validator (in lock order) whose aggregation
    fails aborts with "load full exit data from Obol API: partial signatures threshold aggregate:
    <error>"."""
    groups = []
    pre: Optional[str] = None
    for _, partial_sigs in validators:  # the length pre-check in lock order, up to the first failure
        group = {}
        for i, s in enumerate(partial_sigs):
            if not s:
                continue
            if len(s) != 96:
                pre = _wrap("invalid partial signature", _LEN_ERR).args[0]
                break
            group[i + 1] = s
        if pre is not None:
            break
        groups.append(group)
    outs, sts = impl.threshold_aggregate_batch(groups) if groups else ([], [])
    for st in sts:  # an earlier validator's aggregation error comes first (exit_fetch.go:122-132)
        if st != OK:
            raise _wrap("load full exit data from Obol API",
                        "partial signatures threshold aggregate: " + status_error("threshold_aggregate", st))
    if pre is not None:
        raise _wrap("load full exit data from Obol API", pre)
    return outs
