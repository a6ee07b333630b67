/*
 * hipbls.h -- C ABI of libhipbls.so, the MI355X (gfx950) BLS12-381 backend for charon's tbls
 * package.  Plain pointers and sizes only; every hot-path entry point runs as HIP kernels.
 *
 * Each entry point replaces one method of charon's tbls.Implementation
 * (/root/reference/tbls/tbls.go:27-69) as implemented by tbls.Herumi
 * (/root/reference/tbls/herumi.go), in batched form; see INTEGRATION.md for the cgo binding.
 *
 * Byte formats (identical to herumi ETH mode):
 *   public key  48 B  compressed G1 (ZCash flags 0x80/0x40/0x20, big-endian x)   tbls.go:18
 *   signature   96 B  compressed G2 (x.c1 || x.c0, flags in byte 0)             tbls.go:24
 *   secret key  32 B  big-endian scalar < r                                     tbls.go:21
 *
 * Per-item status codes (the Go shim maps them to herumi's error strings):
 */
#ifndef HIPBLS_H
#define HIPBLS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum hbls_status {
  HBLS_OK = 0,
  HBLS_BAD_PUBKEY = 1,     /* "cannot set compressed public key in Herumi format"   herumi.go:291 */
  HBLS_BAD_SIGNATURE = 2,  /* "cannot unmarshal signature into Herumi signature"    herumi.go:296 */
  HBLS_NOT_VERIFIED = 3,   /* "signature not verified" (Verify, herumi.go:300) /
                              "signature verification failed" (VerifyAggregate, herumi.go:338) */
  HBLS_COMBINE_FAILED = 4, /* "cannot combine signatures"                           herumi.go:282 */
  HBLS_BAD_SECRET = 5,     /* "cannot unmarshal secret into Herumi secret key"      herumi.go:310 */
  HBLS_BAD_INPUT = 6,      /* malformed batch description (offsets/lengths)  -- new, batch-only */
  HBLS_UNCHECKED = 7       /* not resolved: first-error calls, after the first failing item;
                              hbls_slot_select_device, a group with fewer than `threshold` verified
                              members ("require threshold signatures", sigagg.go:86) */
};

/* Return codes of the entry points themselves: 0 on success, <0 on a HIP/runtime error or a
 * malformed batch description (text via hbls_last_error()).  Per-item verdicts are in the status
 * arrays. */

/* Select and initialise the devices the library drives (herumi.go:18-36 init(), idempotent and
 * thread-safe).  device_mask: bit k = HIP device k; 0 = HBLS_DEVICE_MASK from the environment
 * (default: device 0); 0xffffffff = every visible device.  Host-buffer calls shard their items
 * over the devices of the mask (one process, several GPUs: charon runs as one Go process,
 * app/app.go:131).  Calling again with a different mask fails. */
int hbls_init(uint32_t device_mask);
const char* hbls_last_error(void);
/* Nonzero if a gfx950 device is present and the kernels are loadable. */
int hbls_available(void);
/* Devices driven by the library (after hbls_init). */
int hbls_device_count(void);
/* Build provenance (new, no herumi counterpart): "hbls-build:<sha256 prefix of the charon_amd/csrc files
 * and this header>[+<compile defines>]", embedded at compile time by charon_amd/build.py.  The
 * loader (charon_amd/_lib.py) recomputes the source hash from the tree and refuses a library built
 * from other sources. */
const char* hbls_build_id(void);

/* ---------------------------------------------------------------------------------------
 * Host-buffer entry points (the drop-in boundary for the Go shim).  Blocking; the library
 * copies inputs to device memory, runs the kernels and copies results back.
 * --------------------------------------------------------------------------------------- */

/* Verify: n independent (pk, msg, sig) triples.  tbls.Verify / Herumi.Verify
 * (tbls.go:121, herumi.go:288-304).  Message i is msgs[msg_off[i] .. msg_off[i]+msg_len[i]).
 * Identical messages are hashed to G2 once; items over one message are checked together by a
 * random linear combination (one pairing per group, each item re-checked alone if its group
 * fails), so every status equals the per-item verdict.  status[i] in {OK, BAD_PUBKEY,
 * BAD_SIGNATURE, NOT_VERIFIED}.  Thread-safe: concurrent calls (one goroutine per libp2p stream,
 * p2p/receive.go:52) are coalesced into one launch after at most HBLS_COALESCE_US microseconds
 * (default 200; 0 disables). */
int hbls_verify_batch(const uint8_t* pks, const uint8_t* sigs, const uint8_t* msgs,
                      const uint64_t* msg_off, const uint32_t* msg_len, size_t n, uint8_t* status);

/* Verify an ORDERED set up to its first failure (new; the callers' loops that stop at the first
 * failing item: core/parsigex/parsigex.go:93-98 drops a peer's set, core/sigagg/sigagg.go:56-63
 * and core/validatorapi/validatorapi.go:302-306 return the first error).  Same inputs as
 * hbls_verify_batch.  *first = the smallest i whose tbls.Verify fails (-1: every item verifies)
 * and *first_status (nullable) its status, exactly as hbls_verify_batch would report it.
 * status (nullable, n bytes): every item before *first is OK; after it an item is either its
 * exact status or HBLS_UNCHECKED.  Runs of consecutive items over one message are checked
 * together and, behind a failing check, only the first failing batch of runs and the first failing
 * run are resolved -- under attack the cost stays near a clean call's instead of one pairing per
 * item of every failing run.  One device; not coalesced. */
int hbls_verify_batch_first_error(const uint8_t* pks, const uint8_t* sigs, const uint8_t* msgs,
                                  const uint64_t* msg_off, const uint32_t* msg_len, size_t n, int64_t* first,
                                  uint8_t* first_status, uint8_t* status);

/* ThresholdAggregate over groups: group g holds partials grp_off[g] .. grp_off[g+1]-1 with
 * 96-byte signatures sigs[j] and share indices idx[j].  out[g] = sum_j lambda_j(0) sig_j,
 * tbls.ThresholdAggregate / Herumi.ThresholdAggregate (tbls.go:115, herumi.go:249-286).
 * status[g] in {OK, BAD_SIGNATURE, COMBINE_FAILED}. */
int hbls_threshold_aggregate_batch(const uint8_t* sigs, const int64_t* idx, const uint32_t* grp_off,
                                   size_t n_groups, uint8_t* out, uint8_t* status);

/* Aggregate: plain sum of each group's signatures (tbls.Aggregate, herumi.go:225-247).
 * An empty group yields the infinity encoding 0xc0||0^95. status in {OK, BAD_SIGNATURE}. */
int hbls_aggregate_batch(const uint8_t* sigs, const uint32_t* grp_off, size_t n_groups, uint8_t* out,
                         uint8_t* status);

/* VerifyAggregate (FastAggregateVerify): group g verifies sigs[g] on message g against the sum of
 * pks[grp_off[g] .. grp_off[g+1]).  tbls.VerifyAggregate / Herumi.VerifyAggregate
 * (tbls.go:133, herumi.go:318-342).  status in {OK, BAD_SIGNATURE, BAD_PUBKEY, NOT_VERIFIED}.
 * The keys of a group are summed by a parallel segmented reduction, so one group may hold all
 * public shares of a cluster lock (cluster/lock.go:185). */
int hbls_verify_aggregate_batch(const uint8_t* pks, const uint32_t* grp_off, const uint8_t* sigs,
                                const uint8_t* msgs, const uint64_t* msg_off, const uint32_t* msg_len,
                                size_t n_groups, uint8_t* status);

/* Signing roots (eth2util/signing/signing.go:63-77 GetDataRoot = SSZ SigningData{object_root,
 * domain}.HashTreeRoot), the 32-byte messages every verification hashes to G2.
 *   attestation: data[i] is the 128-byte SSZ encoding of a phase0.AttestationData (object root =
 *                its hash-tree-root, core/signeddata.go Attestation.MessageRoot);
 *   generic:     object_roots[i] is a 32-byte object root computed by the caller.
 * domains: n_domains 32-byte domains (signing.GetDomain); item i uses domains[dom_idx[i]]
 * (dom_idx NULL: domain 0).  roots: n x 32 bytes. */
int hbls_attestation_signing_roots(const uint8_t* data, size_t n, const uint8_t* domains, size_t n_domains,
                                   const uint32_t* dom_idx, uint8_t* roots);
int hbls_signing_roots(const uint8_t* object_roots, size_t n, const uint8_t* domains, size_t n_domains,
                       const uint32_t* dom_idx, uint8_t* roots);
/* The signing roots of the other duty types charon verifies per slot, from their SSZ encodings
 * (core/signeddata.go MessageRoot; no host SSZ pass): object i is data[off[i] .. off[i]+len[i]).
 *   kind 1  phase0.AggregateAndProof          (SignedAggregateAndProof.MessageRoot, :979)
 *   kind 2  altair.ContributionAndProof, 264 B (SignedSyncContributionAndProof.MessageRoot, :1227)
 *   kind 3  altair.SyncAggregatorSelectionData{slot, subcommittee_index}, 16 B
 *           (SyncContributionAndProof / SyncCommitteeSelection.MessageRoot, :1135 / :915)
 *   kind 4  uint64 slot, 8 B little-endian (BeaconCommitteeSelection, eth2util.SlotHashRoot, :852)
 *   kind 5  beacon block root, 32 B (SignedSyncMessage.MessageRoot, :1056)
 *   kind 6  v1.ValidatorRegistration{fee_recipient, gas_limit, timestamp, pubkey}, 84 B
 *           (VersionedSignedValidatorRegistration.MessageRoot, :661; one per validator per epoch)
 *   kind 7  phase0.VoluntaryExit{epoch, validator_index}, 16 B (SignedVoluntaryExit.MessageRoot, :580)
 *   kind 8  uint64 epoch, 8 B little-endian (SignedRandao.MessageRoot = eth2util.SignedEpoch, :791)
 *   kind 9  phase0.BeaconBlockHeader{slot, proposer_index, parent_root, state_root, body_root}, 112 B
 *           (VersionedSignedProposal.MessageRoot, :301: a block's root is its header's; the
 *           caller supplies the body root, which the beacon node's block already carries)
 * roots: n x 32 bytes; status: 0, or HBLS_BAD_INPUT for a malformed object (its root all zero). */
int hbls_duty_signing_roots(int kind, const uint8_t* data, const uint64_t* off, const uint32_t* len, size_t n,
                            const uint8_t* domains, size_t n_domains, const uint32_t* dom_idx, uint8_t* roots,
                            uint8_t* status);

/* Public-key cache for the host-buffer verification (hbls_verify_batch): keys added here are
 * decompressed and subgroup-checked once, on every device of the mask; later calls take cached
 * keys from the cache and decompress only the others.  charon adds every pubshare of its cluster
 * lock at startup (cluster/lock.go; the keys never change while it runs).  Statuses and verdicts
 * are unchanged: an undecodable cached key still yields HBLS_BAD_PUBKEY. */
int hbls_pubkey_cache_add(const uint8_t* pks, size_t n);
int hbls_pubkey_cache_clear(void); /* also empties the learned key cache below */
size_t hbls_pubkey_cache_size(void);
/* Learned key cache of the device entry points (hbls_slot_device, hbls_verify_device,
 * hbls_verify_device_first_error without key tables): each device remembers the public keys those
 * calls decompressed -- compressed bytes -> decompressed entry and status, found again by a keyed
 * hash and a compare of all 48 bytes -- and later calls copy the entries instead of repeating the
 * square root and the subgroup ladder; only keys not seen before are decompressed, then learned.
 * Nothing for the caller to manage: a node's pubshares and DV keys are fixed by its cluster lock
 * (cluster/lock.go), so from its second slot on every key is found.  Statuses and outputs are
 * byte-identical with or without it (a status is a function of the key's bytes alone).  The table
 * holds HBLS_KEY_LEARN entries (environment at init, or hbls_tune; default 2^21, about 3.3 GB per
 * device with the ladder tables below, 0.33 GB without them, allocated by the first call that uses
 * it; 0 = off), is append-only and never evicts: a
 * full table keeps what it has and further new keys are decompressed in every call.  Consecutive
 * calls are ordered on the device (a call's lookup runs after the previous call's inserts), so
 * slots enqueued back to back from a cold start decompress each key once.  Not used by calls that
 * pass pk_table / dv_pk_table, by the host-buffer calls (hbls_pubkey_cache_add serves those), by
 * hbls_decompress_pubkeys_device or by VerifyAggregate.
 * hbls_key_learn_stats: for each device of the mask (at most max_devices; *n_devices receives the
 * number written) four values: out[4k] entries held, out[4k+1] capacity, out[4k+2] keys found and
 * out[4k+3] keys decompressed, both cumulative since init.  Waits for the library's enqueued work
 * on each device.
 * Ladder tables: the first HBLS_KEY_WIDE entries (environment at init, or hbls_tune; default: all of
 * them; 0 = none) also keep 15 affine multiples of the key (1440 bytes), built once when a good,
 * finite key is learned.  The random linear combination of a later call then takes 16 ladder steps
 * per key instead of 32 and builds no per-slot tables; the coefficients, and so every status and
 * output, are what they are without the tables.
 * hbls_key_wide_stats: per device five cumulative values: out[5k] tables built, out[5k+1] /
 * out[5k+2] chunks of the chunked combination's key side combined through tables / without,
 * out[5k+3] / out[5k+4] per-item key-side ladders through tables / without.  Waits likewise. */
int hbls_key_learn_stats(uint64_t* out, size_t max_devices, size_t* n_devices);
int hbls_key_wide_stats(uint64_t* out, size_t max_devices, size_t* n_devices);
/* Decompressed-signature cache (new, no herumi counterpart): hbls_verify_batch keeps the
 * decompressed, subgroup-checked points of the partials it verified (a ring of `entries` per
 * device, keyed by all 96 bytes), and hbls_threshold_aggregate_batch takes its members from it
 * instead of decompressing them again -- charon aggregates exactly the partials parsigex verified
 * (core/parsigdb/memory.go:197-225 -> core/sigagg/sigagg.go:105).  Results are identical with or
 * without it.  Sets the capacity (rounded down to a power of two; 0 = off; default 2^21, or
 * HBLS_SIG_CACHE), drops the contents and returns the previous capacity.  Call while no host-buffer
 * call is in flight. */
size_t hbls_sig_cache(size_t entries);

/* Test switch of the in-process multi-device split (charon is one process over every GPU of the
 * node, app/app.go:131): every device of the mask is driven through `copies` contexts (own streams,
 * workspaces and host thread), so the host-buffer entry points shard their items over them exactly
 * as over several GPUs, on a one-GPU machine.  1 restores one context per device.  Call while no
 * other call is in flight.  Results never depend on it. */
int hbls_debug_split(uint32_t copies);

/* Sign (herumi.go:306-316) and SecretToPublicKey (herumi.go:66-79), batched.
 * Sign status in {OK, BAD_SECRET}; SecretToPublicKey additionally rejects the zero key. */
int hbls_sign_batch(const uint8_t* sks, const uint8_t* msgs, const uint64_t* msg_off,
                    const uint32_t* msg_len, size_t n, uint8_t* sigs, uint8_t* status);
int hbls_secret_to_public_key_batch(const uint8_t* sks, size_t n, uint8_t* pks, uint8_t* status);

/* ThresholdSplit core (herumi.go:137-185): shares[i-1] = f(i) for i = 1..total where
 * f(z) = secret + sum_k coeffs[k-1] z^k (threshold-1 coefficients, 32 B big-endian each; the
 * caller draws them from a CSPRNG or, for ThresholdSplitInsecure, from its reader).
 * RecoverSecret (herumi.go:187-223): Lagrange interpolation at 0 over k shares. */
int hbls_threshold_split(const uint8_t* secret, const uint8_t* coeffs, uint32_t total, uint32_t threshold,
                         uint8_t* shares, uint8_t* status);
int hbls_recover_secret(const uint8_t* shares, const int64_t* idx, size_t k, uint8_t* out, uint8_t* status);

/* ---------------------------------------------------------------------------------------
 * Device-buffer entry points (inputs already resident in HBM; asynchronous on `stream`, a
 * hipStream_t passed as void*; 0 = the first device's null stream).  The device is the one the
 * stream belongs to.  All pointers are device pointers.  Work is ordered after prior work on
 * `stream` and complete when later work on `stream` starts; library workspaces are ordered by
 * events, so calls on different streams never race on them.
 *
 * verify: msg_idx[i] indexes the table of distinct messages hashed by hbls_hash_to_g2_device
 * into `hm` (hbls_hm_entry_bytes() per message, library layout).  vgrp_off (nullable): groups
 * of consecutive partials over one message (group g = [vgrp_off[g], vgrp_off[g+1])), checked
 * together; NULL = every partial on its own.
 * --------------------------------------------------------------------------------------- */
int hbls_hash_to_g2_device(const uint8_t* msgs, const uint64_t* msg_off, const uint32_t* msg_len,
                           size_t n_msgs, void* hm, void* stream);
/* hbls_verify_batch_first_error on device buffers: the items in set order with vgrp_off's groups
 * (consecutive items over one message); status as there; *first (a device uint32) = the first
 * failing item, 0xffffffff when every item verifies. */
int hbls_verify_device_first_error(const uint8_t* pks, const uint8_t* sigs, const uint32_t* msg_idx, const void* hm,
                                   size_t n, const uint32_t* vgrp_off, size_t n_vgroups, uint8_t* status,
                                   uint32_t* first, void* stream);
int hbls_verify_device(const uint8_t* pks, const uint8_t* sigs, const uint32_t* msg_idx, const void* hm,
                       size_t n, const uint32_t* vgrp_off, size_t n_vgroups, uint8_t* status, void* stream);
int hbls_threshold_aggregate_device(const uint8_t* sigs, const int64_t* idx, const uint32_t* grp_off,
                                    size_t n_groups, size_t n_partials, uint8_t* out, uint8_t* status,
                                    void* stream);

/* Attestation signing roots on device buffers (see hbls_attestation_signing_roots); dom_idx
 * entries must be < n_domains: the device path cannot return a per-call error without a host
 * synchronisation, so an out-of-range entry yields the all-zero root (never a root under another
 * domain; no signature over a real signing root verifies against it -- the item fails closed).
 * Writes the messages a slot then hashes (hbls_hash_to_g2_device / hbls_slot_device msgs). */
int hbls_attestation_signing_roots_device(const uint8_t* data, size_t n, const uint8_t* domains, size_t n_domains,
                                          const uint32_t* dom_idx, uint8_t* roots, void* stream);

/* Decompressed-key tables for hbls_slot pk_table / dv_pk_table: n compressed public keys ->
 * n entries of hbls_pk_entry_bytes() (library layout) + a status byte each (0 = valid, else the
 * key is undecodable or outside G1 and every partial under it gets HBLS_BAD_PUBKEY). */
size_t hbls_pk_entry_bytes(void);
int hbls_decompress_pubkeys_device(const uint8_t* pks, size_t n, void* table, uint8_t* status, void* stream);

/* VerifyAggregate on device buffers: pks (48 B each), sigs (96 B per group), hm (one hashed message
 * per group, hbls_hash_to_g2_device), status (n_groups) are device pointers; grp_off is a HOST
 * array of n_groups + 1 non-decreasing offsets into pks (the reduction is planned from it). */
int hbls_verify_aggregate_device(const uint8_t* pks, const uint32_t* grp_off, size_t n_groups,
                                 const uint8_t* sigs, const void* hm, uint8_t* status, void* stream);

/* One attestation slot in one call: the batch entry point of SURVEY.md section 8b for
 * sigagg/parsigex (core/parsigex/parsigex.go:93-98, core/sigagg/sigagg.go:56-63,105,117).
 *   - hash the n_msgs distinct messages (+ their Miller lines) into hm;
 *   - verify the n partials (msg_idx[i] indexes the messages, vgrp_off groups as in
 *     hbls_verify_device) into vstatus;
 *   - threshold-aggregate n_groups groups (grp_off over n_ta_partials members with share indices
 *     ta_idx) into ta_out / ta_status.  Members are either verified partials (ta_src[j] = index
 *     of member j among the n partials: their decompression is shared) or their own 96-byte
 *     signatures ta_sigs (ta_src == NULL);
 *   - optionally (dv_pks != NULL, requires n_vgroups == n_groups with group g = validator g):
 *     verify each aggregate under the validator's DV public key (sigagg.go:117) into
 *     agg_vstatus, folded into group g's combined check.  agg_vstatus[g] is the aggregation
 *     status when no aggregate was produced.
 * Semantics per item as hbls_verify_batch / hbls_threshold_aggregate_batch.
 * Ordering: the call's work runs behind what `stream` holds and, because it starts writing hm on
 * its own side streams at once, also behind what the device's default stream holds when the call
 * is made (buffers filled there need no extra synchronisation, as with a blocking stream). */
typedef struct hbls_slot {
  const uint8_t* msgs;
  const uint64_t* msg_off;
  const uint32_t* msg_len;
  size_t n_msgs;
  void* hm;
  const uint8_t* pks;
  const uint8_t* sigs;
  const uint32_t* msg_idx;
  size_t n;
  const uint32_t* vgrp_off;
  size_t n_vgroups;
  uint8_t* vstatus;
  const uint8_t* ta_sigs;
  const uint32_t* ta_src;
  const int64_t* ta_idx;
  const uint32_t* grp_off;
  size_t n_groups;
  size_t n_ta_partials;
  uint8_t* ta_out;
  uint8_t* ta_status;
  const uint8_t* dv_pks;
  uint8_t* agg_vstatus;
  /* Optional decompressed-key tables (hbls_decompress_pubkeys_device): when non-NULL the slot
   * reads entry i of pk_table (status pk_table_st[i]) instead of decompressing pks[i], and
   * entry g of dv_pk_table instead of dv_pks[g].  Pubshares are static per cluster lock, so a
   * node decompresses and subgroup-checks them once (SURVEY.md 8e pubshare cache).  Without
   * tables the learned key cache (hbls_key_learn_stats above) does the same by itself. */
  const void* pk_table;
  const uint8_t* pk_table_st;
  const void* dv_pk_table;
  const uint8_t* dv_pk_table_st;
} hbls_slot;
int hbls_slot_device(const hbls_slot* args, void* stream);
/* hbls_slot_device with verified-member selection (parsigex.go:93-98 -> parsigdb/memory.go:198-225
 * -> sigagg.go:84-117).  args as for hbls_slot_device, except:
 *   - ta_src / ta_idx / grp_off list each group's CANDIDATES in the caller's order of preference
 *     (arrival order); groups may have different candidate counts, 0 included; ta_sigs must be NULL;
 *   - dv_pks is required; vgrp_off's groups are independent of the aggregation groups (the
 *     n_vgroups == n_groups rule of the folded form does not apply).
 * Group g's members are its first `threshold` candidates j, in order, with vstatus[ta_src[j]] == OK
 * whose share index differs from every member already chosen (sigagg.go:90-97 keys by ShareIdx).
 * chosen (device, n_groups * threshold uint32): the members as indices among the n partials,
 * 0xffffffff past the last one.  ta_count (device, n_groups uint32): members found (<= threshold).
 * A group with fewer than `threshold` members gets ta_status = agg_vstatus = HBLS_UNCHECKED and 96
 * zero bytes in ta_out (sigagg.go:85-86, 99-101); a group whose candidates do not all carry one
 * msg_idx gets HBLS_BAD_INPUT in both (and zero bytes).  Otherwise ta_status is as in
 * hbls_threshold_aggregate_batch over the chosen members and agg_vstatus[g] the verdict of the
 * aggregate under dv_pks[g] over the members' message (the aggregation status when no aggregate was
 * produced).  vstatus is what hbls_slot_device writes for the same partials.  The aggregation runs
 * behind the verdicts and the aggregates' verification behind the aggregation, all stream-ordered
 * as hbls_slot_device: no host synchronisation, every output valid when later work on `stream`
 * starts.  threshold: 1 .. 16, anything else is a call error.
 * hbls_slot_select_stats: cumulative per-process counters over the devices of the mask, reset by
 * reading (n <= 4): out[0] groups seen, out[1] groups with fewer than `threshold` members, out[2]
 * groups whose members are not their first `threshold` candidates, out[3] groups aggregated by the
 * small-scalar path (whole waves of validators with one index set: the call orders the groups by
 * their chosen positions to keep it that way; a falling share means the slower per-member ladders
 * ran).  Waits for the devices' work. */
int hbls_slot_select_device(const hbls_slot* args, uint32_t threshold, uint32_t* chosen,
                            uint32_t* ta_count, void* stream);
int hbls_slot_select_stats(uint64_t* out, size_t n);
/* One duty from host buffers to aggregates: hbls_verify_batch over the n partials, the choice of
 * each validator's members among its verified candidates, hbls_threshold_aggregate_batch over the
 * members and hbls_verify_batch of the aggregates under the DV keys, in one blocking, thread-safe
 * call with flat arguments (what the Go shim can pass; hbls_slot's pointers to Go memory it cannot).
 *   pks, sigs, msgs, msg_off, msg_len, n: the partials, exactly as hbls_verify_batch takes them;
 *   cand, cand_idx, grp_off (n_groups + 1 entries): group g's candidates in arrival order are
 *     cand[j], an index among the n partials, under share index cand_idx[j], for j in
 *     [grp_off[g], grp_off[g + 1]); a candidate with cand[j] >= n counts as not verified;
 *   dv_pks: 48 bytes per group; threshold: 1 .. 16.
 * Outputs, all host memory: vstatus (n), one per partial as hbls_verify_batch writes it, whether
 * or not a group lists the partial; chosen (n_groups * threshold), the members as indices among the
 * n partials, 0xffffffff past the last one; ta_count (n_groups); ta_out (96 bytes per group);
 * ta_status and agg_vstatus (n_groups each).
 * The members follow the reference's matching rule (parsigdb/memory.go:149-160, 197-225).  Walking
 * a group's candidates in order, candidate j is stored iff its vstatus is OK and no earlier
 * candidate with OK status has its share index (whatever that one's message).  The first message
 * to hold `threshold` stored candidates wins; those, in candidate order, are the members.  A group
 * whose candidates are all over one message gets what hbls_slot_select_device gives it: also below
 * `threshold`, where chosen and ta_count report the stored candidates found.  A group whose
 * candidates span several messages of which none reaches `threshold` has no members: ta_count 0.
 * HBLS_BAD_INPUT for candidates over two messages does not arise here.
 * ta_status is as hbls_threshold_aggregate_batch over the members, agg_vstatus[g] the aggregate's
 * verdict under dv_pks[g] over the members' message (the aggregation status when there is no
 * aggregate).  A group without `threshold` members gets HBLS_UNCHECKED in both and 96 zero bytes.
 * n_groups == 0 verifies the partials and returns; n == 0 gives every group HBLS_UNCHECKED.
 * Call errors (-1): threshold outside 1..16, grp_off not non-decreasing, n or n_groups * threshold
 * of 2^32 - 1 or more, a required pointer that is NULL while its count is not zero.
 * The aggregation groups are sharded over the devices of the mask; a shard verifies the partials
 * its groups list (one listed by groups of two shards is verified in both) and its share of the
 * partials no group lists.  The call runs the device entry's pipeline: learned key cache, ladder
 * tables, batched subgroup test, the aggregation reading the partials the verification
 * decompressed.  It does not write into the decompressed-signature cache (hbls_sig_cache): a later
 * hbls_threshold_aggregate_batch over the same partials decompresses them again.  One shard is not
 * chunked: a call beyond the workspace's reach fails, as hbls_slot_select_device does. */
int hbls_slot_select_batch(const uint8_t* pks, const uint8_t* sigs, const uint8_t* msgs,
                           const uint64_t* msg_off, const uint32_t* msg_len, size_t n,
                           const uint32_t* cand, const int64_t* cand_idx, const uint32_t* grp_off,
                           size_t n_groups, const uint8_t* dv_pks, uint32_t threshold,
                           uint8_t* vstatus, uint32_t* chosen, uint32_t* ta_count, uint8_t* ta_out,
                           uint8_t* ta_status, uint8_t* agg_vstatus);
/* Duty sessions: hbls_slot_select_batch's pipeline under the reference node's arrival pattern.  A
 * duty keeps its state in device memory between calls: the hashed messages, and per group
 * (validator) the decompressed points, share indices and message ids of the partials stored so
 * far.  Each arriving set is one hbls_duty_add: it verifies the set, stores what the ParSigDB would
 * store, aggregates the groups that reach `threshold` through this set from the resident points,
 * verifies their aggregates under the DV keys, and returns those groups only.  For any way of
 * cutting one candidate stream into adds, the union of what the adds return equals what
 * hbls_slot_select_batch returns for the concatenation (given max_stored no smaller than a group's
 * candidates).  A handle is never 0.
 * hbls_duty_open: group g is validator g and dv_pks[48 g] its DV key; threshold: 1 .. 16;
 *   max_stored: 1 .. 64, the stored partials a group can hold.  Everything but the message table
 *   is allocated here, on every device that owns groups (208 + 16 bytes per slot of n_groups *
 *   max_stored); a failed allocation is a call error that leaves nothing behind.
 * hbls_duty_add: the n partials in arrival order, bytes and messages exactly as hbls_verify_batch
 *   takes them; partial i belongs to group group[i] under share index share_idx[i]; group[i] >=
 *   n_groups (0xffffffff, say) means "verify only".  Partial i is serial *first_serial + i, where
 *   *first_serial is the number of partials of all earlier adds.
 *   vstatus[i]: what hbls_verify_batch writes for the partial, whatever its group.
 *   Walking the partials in order, partial i is stored (stored[i] = 1) iff its vstatus is OK, its
 *   group has not fired, no stored partial of the group has its share index (whatever that one's
 *   message) and the group holds fewer than max_stored.  A store that gives some message `threshold`
 *   stored partials in the group fires it: its members are those partials in stored order, and the
 *   group is closed from then on (later partials, also of the same call, are verified, not stored).
 *   fired[0 .. *n_fired): the groups that fired in this call, ascending; for row k, chosen[k t ..
 *   k t + t) are the members' serials, ta_out[96 k] and ta_status[k] as
 *   hbls_threshold_aggregate_batch over the members, agg_vstatus[k] the aggregate's verdict under the
 *   group's DV key over the members' message (the aggregation status when there is no aggregate).
 *   The caller sizes the fired-row arrays for min(n, n_groups) rows; rows past *n_fired are not
 *   written.  n == 0 is valid and fires nothing.
 * hbls_duty_state: per group, the number of stored partials and whether it has fired (n_groups each).
 * hbls_duty_stats (cumulative for the duty, n <= 6): out[0] partials seen, out[1] partials stored,
 *   out[2] messages hashed to G2, out[3] message lookups answered from the duty's resident table
 *   (every partial is one lookup: out[2] + out[3] == out[0] on one device), out[4] groups fired,
 *   out[5] partials not stored because their group was full.
 * hbls_duty_close frees the duty.  Any call with a closed handle, or one never issued, is a call
 *   error (-1 with hbls_last_error).  Other call errors: threshold or max_stored out of range, a
 *   required pointer that is NULL while its count is not zero, a duty that would reach 2^32 - 1
 *   partials.  A device error inside an add fails the duty: later adds are call errors.
 * Threading: calls on one duty are serialised by the library; calls on different duties, and every
 * other entry point, may run concurrently.  Every call is blocking.
 * Devices: the groups are sharded over the devices of the mask in contiguous ranges, as
 * hbls_slot_select_batch shards them; each shard owns its groups' state and its own message table.
 * A partial goes to the shard of its group, a verify-only partial i of n to shard i nd / n.  One
 * shard's add is not chunked: an add beyond the workspace's reach fails.
 * Caches: the device entry's pipeline (learned key cache, ladder tables, batched subgroup test);
 * the decompressed-signature cache is not written. */
int hbls_duty_open(const uint8_t* dv_pks, size_t n_groups, uint32_t threshold, uint32_t max_stored,
                   uint64_t* duty);
int hbls_duty_add(uint64_t duty, const uint8_t* pks, const uint8_t* sigs, const uint8_t* msgs,
                  const uint64_t* msg_off, const uint32_t* msg_len, const uint32_t* group,
                  const int64_t* share_idx, size_t n, uint8_t* vstatus, uint8_t* stored,
                  uint32_t* first_serial, uint32_t* fired, size_t* n_fired, uint32_t* chosen,
                  uint8_t* ta_out, uint8_t* ta_status, uint8_t* agg_vstatus);
int hbls_duty_state(uint64_t duty, uint32_t* stored_count, uint8_t* fired_flag);
int hbls_duty_stats(uint64_t duty, uint64_t* out, size_t n);
int hbls_duty_close(uint64_t duty);
/* Set-atomic adds: a peer's set is stored whole or not at all, as the reference node does it
 * (ParSigEx.handle verifies every partial of a set and returns at the first failure, before
 * ParSigDB.StoreExternal sees the set).  Everything not named here means what it means for
 * hbls_duty_add; the two calls may be mixed on one duty.
 * hbls_duty_add_sets: set k of the call is partials [set_off[k], set_off[k + 1]) in arrival order.
 *   set_off has n_sets + 1 entries, set_off[0] == 0, set_off[n_sets] == n, non-decreasing; empty
 *   sets are allowed anywhere.  Anything else, a NULL set_off or set_first with n_sets > 0, and
 *   n_sets == 0 with n != 0 are call errors, on which nothing is verified, stored or numbered.
 *   vstatus[i]: exactly what hbls_verify_batch writes, for every partial -- those of rejected sets
 *   and verify-only ones (which belong to their set like any other) included.
 *   set_first[k]: the smallest i of set k with vstatus[i] != HBLS_OK, as an index among the call's n
 *   partials; 0xffffffff when there is none (an empty set has none).  Set k is rejected iff
 *   set_first[k] != 0xffffffff.
 *   No partial of a rejected set is stored: stored[i] = 0, no record slot is taken, nothing counts
 *   towards max_stored or "group full" (hbls_duty_stats out[5]); it still has serial *first_serial + i.
 *   To the partials of the admitted sets, in arrival order across the call, hbls_duty_add's rule
 *   applies unchanged: a later set of the call sees what an earlier admitted set of it stored and fired.
 *   So the call equals hbls_duty_add given the same partials with group[i] = 0xffffffff for every i of
 *   a rejected set, in vstatus, stored, first_serial, the fired rows and the duty's state; with every
 *   set a singleton it equals hbls_duty_add on the call as it is.
 * hbls_duty_set_stats (cumulative, n <= 3): out[0] sets seen, empty ones included; out[1] sets
 *   rejected; out[2] partials with vstatus OK that were not stored because their set was rejected.
 * Devices: a set spans shards (its partials go to their groups' shards, verify-only ones by position);
 *   rejection is decided over the whole call, whichever shard saw the failure, at the cost of one
 *   more host round trip when the duty has more than one shard. */
int hbls_duty_add_sets(uint64_t duty, const uint8_t* pks, const uint8_t* sigs, const uint8_t* msgs,
                       const uint64_t* msg_off, const uint32_t* msg_len, const uint32_t* group,
                       const int64_t* share_idx, size_t n, const uint32_t* set_off, size_t n_sets,
                       uint8_t* vstatus, uint8_t* stored, uint32_t* first_serial, uint32_t* set_first,
                       uint32_t* fired, size_t* n_fired, uint32_t* chosen, uint8_t* ta_out,
                       uint8_t* ta_status, uint8_t* agg_vstatus);
int hbls_duty_set_stats(uint64_t duty, uint64_t* out, size_t n);
/* hbls_duty_add_sets that stops a rejected set at its first failure (parsigex.go:93-98 returns at the
 * first failing partial of a set): the same arguments and outputs, freely mixed with hbls_duty_add and
 * hbls_duty_add_sets on one duty, and everything not named here means what it means there.  A set
 * that is thrown away no longer costs the exact status of each of its partials, however many are bad.
 *   set_first[k]: exact -- the smallest i of set k, in arrival order, whose status from
 *   hbls_verify_batch would not be HBLS_OK; 0xffffffff when there is none.
 *   vstatus of an admitted set: every partial HBLS_OK (exact: nothing failed).
 *   vstatus of a rejected set k, f = set_first[k]: vstatus[f] is the exact status (not OK); every i < f
 *   of the set is HBLS_OK; every other partial of the set carries its exact status or HBLS_UNCHECKED,
 *   nothing else.  Decoding failures are exact everywhere; verify-only partials belong to their set.
 *   Below the batched final exponentiation's size (hbls_fe_batch) every status is exact.
 *   On a twin duty given the same calls through hbls_duty_add_sets, set_first, stored, first_serial,
 *   the fired rows (fired, n_fired, chosen, ta_out, ta_status, agg_vstatus), hbls_duty_state,
 *   hbls_duty_stats and hbls_duty_set_stats out[0] and out[1] are equal; out[2] counts the partials of
 *   rejected sets reported HBLS_OK and is at most the twin's.
 *   The partials are verified in arrival order (set by set), in runs of consecutive partials over one
 *   message: a call of many sets over the same messages forms smaller groups than hbls_duty_add_sets,
 *   which sorts the call by message.  Take this call for a peer's set as it arrives, or whenever sets
 *   may be bad; take hbls_duty_add_sets for a large window of sets known to be clean.
 * hbls_duty_first_stats (cumulative, n <= 2): out[0] partials that went through this call, out[1]
 *   those reported HBLS_UNCHECKED. */
int hbls_duty_add_sets_first(uint64_t duty, const uint8_t* pks, const uint8_t* sigs, const uint8_t* msgs,
                             const uint64_t* msg_off, const uint32_t* msg_len, const uint32_t* group,
                             const int64_t* share_idx, size_t n, const uint32_t* set_off, size_t n_sets,
                             uint8_t* vstatus, uint8_t* stored, uint32_t* first_serial, uint32_t* set_first,
                             uint32_t* fired, size_t* n_fired, uint32_t* chosen, uint8_t* ta_out,
                             uint8_t* ta_status, uint8_t* agg_vstatus);
int hbls_duty_first_stats(uint64_t duty, uint64_t* out, size_t n);
/* Cluster handles: the cluster lock as an object of the library, and duties that take their keys from
 * it.  The reference ties a partial's key to its share index inside the verifier
 * (core/parsigex/parsigex.go:146-170 NewEth2Verifier looks the pubshare up by (DV pubkey, ShareIdx) in
 * the lock and fails with "unknown pubkey, not part of cluster lock" or "invalid shareIdx" before any
 * pairing runs).  A duty opened on a cluster does the same on the device: its adds take no pks, each
 * partial's key is resolved from (group[i], share_idx[i]), and the fired groups' aggregates are verified
 * under the cluster's DV keys.
 * hbls_cluster_open: row g of the cluster: entry 0 is validator g's DV key, entry j (1..n_shares) its
 *   pubshare of share index j.  dv_pks: 48 n_validators bytes; pubshares: 48 n_validators n_shares
 *   bytes, validator-major (share j of validator g at 48 (g n_shares + j - 1)).  key_status (nullable):
 *   n_validators (1 + n_shares) bytes, row-major as above, each what hbls_decompress_pubkeys_device
 *   reports for that key.  ladder_tables: 0 / 1 (1: every good, finite key also gets its ladder table,
 *   15 points, as the learned key cache's HBLS_KEY_WIDE entries have).  1 <= n_shares <= 64;
 *   n_validators (1 + n_shares) < 2^32 - 1.  The keys are decompressed and subgroup-checked once, sharded
 *   over the devices as a duty's groups are (contiguous ranges, the devices as they are at open), and
 *   live as long as the handle or any duty opened on it; after open the cluster never changes, and any
 *   number of duties and calls read it concurrently.  A bad key does not fail the open: its status is
 *   reported and kept, and every partial that names it gets HBLS_BAD_PUBKEY.  Nothing of the learned key
 *   cache is used: hbls_pubkey_cache_clear, hbls_tune and HBLS_KEY_LEARN do not touch a cluster.
 *   Device memory: 112 + 1 bytes per key, 1440 more with ladder tables -- about 1.7 GB at 100 000
 *   validators x 11 keys with tables, 0.15 GB without.  That is what the cluster itself allocates and
 *   what goes when it does.  Measured, device memory in use grew by 2.6 GB, not 1.7, across an open
 *   with tables at that size (0.13 GB without tables): the other 0.9 GB is not the cluster's and does
 *   not come back at close.  It is put down -- not verified -- to the scratch the HIP runtime reserves
 *   on the queue of the device's library stream for the table builder's 3 096 bytes per lane.  Size
 *   memory by the larger figure, once per process and device.  A failing device call leaves nothing
 *   allocated.
 * hbls_cluster_close invalidates the handle; the device memory goes when the last duty opened on the
 *   cluster is closed.
 * hbls_cluster_stats (n <= 6; counted on the host): out[0] keys held, out[1] keys with a non-zero
 *   status, out[2] ladder tables built, out[3] partials of adds resolved to a key, out[4] partials of
 *   adds that named no key, out[5] DV keys resolved for aggregates.  out[3..5] count the adds that
 *   returned 0: an add that fails on a device call counts nothing.
 * hbls_duty_open_cluster: a duty over the cluster's validators (n_groups = n_validators), threshold and
 *   max_stored as hbls_duty_open takes them.  Its shards are the cluster's (same devices, same ranges),
 *   whatever the device split is by now.  Every duty call serves it with unchanged signatures, except:
 *   pks must be NULL in hbls_duty_add, hbls_duty_add_sets and hbls_duty_add_sets_first (a non-NULL pks
 *   is a call error that writes nothing; on a plain duty a NULL pks stays the call error it is).
 * Which key: partial i has a key iff group[i] < n_validators and 1 <= share_idx[i] <= n_shares, compared
 *   on the full 64-bit share_idx (2^32 + 1, a negative value or INT64_MIN names no key; nothing is
 *   truncated).  A partial that names no key gets HBLS_BAD_PUBKEY, is not stored, and is a set's first
 *   failure like any other.  So a group[i] >= n_validators, which is "verify only" on a plain duty, has
 *   no key on a cluster duty and fails the same way.  The shim tells the reference's two pre-errors apart
 *   from its own group and share index when it sees HBLS_BAD_PUBKEY.
 * DEFINING PROPERTY (the twin).  For any cluster and any sequence of calls, a cluster duty equals a plain
 *   duty opened with the same dv_pks, threshold and max_stored under the same shard layout and fed the
 *   same calls with pks[i] = the lock's 48 bytes for (group[i], share_idx[i]) where that names a key and
 *   48 zero bytes (no compression flag: HBLS_BAD_PUBKEY) elsewhere: every output of every call (vstatus,
 *   stored, first_serial, set_first, fired, n_fired, chosen, ta_out, ta_status, agg_vstatus),
 *   hbls_duty_state, hbls_duty_stats, hbls_duty_set_stats and hbls_duty_first_stats are equal.  The one
 *   exception is vstatus of hbls_duty_add_sets_first, held to that call's contract above against the
 *   twin's exact statuses (as that call is against hbls_duty_add_sets).
 * hbls_cluster_check: is the lock consistent -- do the pubshares of every validator interpolate to its DV
 *   key under `threshold`.  A lock with a wrong, swapped or stale pubshare opens clean (every key decodes
 *   and is in the subgroup) and every partial verifies under its pubshare; only the aggregates fail
 *   (agg_vstatus HBLS_NOT_VERIFIED), with no hint which key is at fault.  This call finds it beforehand.
 *   Row g is P_0 (the DV key, node 0), P_1 .. P_n (the pubshares, nodes 1 .. n = n_shares): points of a
 *   cyclic group of prime order on consecutive nodes, which lie on a polynomial of degree < threshold in
 *   the exponent iff every threshold-th forward difference vanishes,
 *       D_k = sum_{i=0..t} (-1)^(t-i) C(t,i) P_{k+i} = O     for k = 0 .. n - t   (W = n - t + 1 windows).
 *   The criterion is exact both ways (the sequences with every D_k = O form a space of dimension t, the
 *   polynomials of degree < t), and a row of lower degree passes too: the call answers "degree < t",
 *   which is what interpolation from any t shares needs.  1 <= threshold <= n_shares; anything else, or
 *   an unknown handle, is a call error (-1, hbls_last_error) that writes nothing.
 *   row_status (n_validators bytes): HBLS_OK when all W differences of the row are O; HBLS_BAD_PUBKEY
 *   when any of the row's 1 + n_shares keys has a non-zero key_status -- nothing is computed for such a
 *   row and its row_windows is 0: it is not inconsistent, it is unusable; HBLS_NOT_VERIFIED when some
 *   D_k != O.  row_windows (nullable, n_validators words): bit k set iff D_k != O (W <= 64).  If exactly
 *   one key P_p of a row is wrong, exactly the windows with k <= p <= k + t fail, which locates it.
 *   *n_bad (nullable): the rows with a non-zero status.  A key at infinity with status 0 is the identity
 *   in the sums: the group law decides, nothing is special-cased into a status.
 *   Blocking and thread-safe; it only reads the cluster, so it may run beside any number of duties and
 *   adds on it and changes nothing they return.  It runs per shard, on the shard's device, over the
 *   shard's own rows (the ranges as they were at open); a failing device call leaves nothing allocated
 *   and writes nothing.
 * hbls_cluster_check_stats (n <= 2; counted on the host): out[0] checks that returned 0, out[1] rows
 *   those checks reported HBLS_NOT_VERIFIED.
 * Cluster verifies: anything signed by a key of the lock is verified by naming the key, not by sending it
 *   (cluster/lock.go:185 and :235-281 at every start, dkg/dkg.go:595, :684, :864, :948, the validator
 *   API's own partials, exits under DV keys and pubshares).  Neither call reads or writes the learned key
 *   cache, the host public-key cache or the decompressed-signature cache; both only read the cluster, are
 *   blocking and thread-safe, and may run beside any duty or call on it, changing nothing those return.
 * hbls_cluster_verify_batch: hbls_verify_batch whose keys come from the lock.  Item i is verified under
 *   the key (group[i], key_idx[i]) names: key_idx 0 the validator's DV key, key_idx j in 1..n_shares its
 *   pubshare of share index j.  An item that names no key -- group[i] >= n_validators, or a key_idx that
 *   is negative, above n_shares, 2^32 + 1 or INT64_MIN: every comparison is on the full 64 bits -- gets
 *   HBLS_BAD_PUBKEY.  The keys' ladder tables are used where the cluster has them.
 *   DEFINING PROPERTY (the twin).  For any cluster and any call, status equals what hbls_verify_batch
 *   writes for the same sigs and messages with pks[i] = the lock's 48 bytes for the named key, or 48 zero
 *   bytes where the pair names no key.
 *   Items go to the shard that owns their group (items that name no validator need no device).  One
 *   shard's part of a call is one verification: it is not chunked, as a duty add is not.  n == 0 is valid
 *   and writes nothing; an unknown handle or a NULL group, key_idx, sigs, msg_off, msg_len or status with
 *   n > 0 (or NULL msgs with a message of non-zero length) is a call error that writes nothing.
 * hbls_cluster_verify_aggregate: FastAggregateVerify of one signature over one message under the sum of
 *   the selected keys of every row.  Bit j - 1 of share_mask selects the pubshare of share index j,
 *   with_dv (0 or 1) the DV key; lock.go:185 and dkg.go:595 are every share and no DV key.
 *   DEFINING PROPERTY (the twin).  *status equals what hbls_verify_aggregate_batch writes for one group
 *   holding the selected keys' 48-byte forms in row-major order, the same signature and the same
 *   message -- herumi's order of checks included: the signature's decoding first (HBLS_BAD_SIGNATURE),
 *   then a selected key with a non-zero key_status (HBLS_BAD_PUBKEY), then "an empty group or an identity
 *   signature never verifies" (HBLS_NOT_VERIFIED), then the pairing.  A selected key at infinity with
 *   status 0 is the identity in the sum; an unselected bad key does not matter.
 *   Call errors (-1, nothing written): a mask bit at or above n_shares, with_dv > 1, a NULL sig or status,
 *   a NULL msg with msg_len > 0, an unknown handle.
 *   Per shard, on its device, the selected entries of every row are summed straight from the resident
 *   table (nothing is decompressed or copied out) and reduced to one point and one flag; these go through
 *   the host to the first non-empty shard's device, where one more reduction pass and the tail of
 *   hbls_verify_aggregate_batch run.
 * hbls_cluster_verify_stats (n <= 5; counted on the host, for calls that returned 0): out[0] verify-batch
 *   calls, out[1] items resolved to a key, out[2] items that named no key, out[3] aggregate calls, out[4]
 *   keys summed by aggregate calls.  hbls_cluster_stats and hbls_cluster_check_stats are not touched.
 * Not covered: hbls_slot_select_batch and the device entry points take no cluster. */
int hbls_cluster_open(const uint8_t* dv_pks, const uint8_t* pubshares, size_t n_validators, uint32_t n_shares,
                      uint32_t ladder_tables, uint8_t* key_status, uint64_t* cluster);
int hbls_cluster_close(uint64_t cluster);
int hbls_cluster_stats(uint64_t cluster, uint64_t* out, size_t n);
int hbls_duty_open_cluster(uint64_t cluster, uint32_t threshold, uint32_t max_stored, uint64_t* duty);
int hbls_cluster_check(uint64_t cluster, uint32_t threshold, uint8_t* row_status, uint64_t* row_windows,
                       size_t* n_bad);
int hbls_cluster_check_stats(uint64_t cluster, uint64_t* out, size_t n);
int hbls_cluster_verify_batch(uint64_t cluster, const uint32_t* group, const int64_t* key_idx, const uint8_t* sigs,
                              const uint8_t* msgs, const uint64_t* msg_off, const uint32_t* msg_len, size_t n,
                              uint8_t* status);
int hbls_cluster_verify_aggregate(uint64_t cluster, uint64_t share_mask, uint32_t with_dv, const uint8_t* sig,
                                  const uint8_t* msg, uint32_t msg_len, uint8_t* status);
int hbls_cluster_verify_stats(uint64_t cluster, uint64_t* out, size_t n);
/* Bytes of the `hm` table entry per message. */
size_t hbls_hm_entry_bytes(void);
/* Measurement: with timing enabled (which also resets the record), every kernel launch of the
 * verification, aggregation and hashing paths is bracketed by HIP events on the stream it runs
 * on; hbls_timing_read returns kernel names (static strings) and durations in milliseconds, in
 * launch order.  enable: 0 off, 1 on, 2 on and serialised (each timed launch completes before
 * the call enqueues the next one, so every duration is the kernel alone on the device: the
 * per-kernel roofline; calls then block). */
int hbls_timing(int enable);
int hbls_timing_read(const char** names, float* ms, size_t max_n, size_t* n_out);
/* Verification statistics, collected only with HBLS_STATS=1 in the environment (each call then
 * synchronises): out[0] items verified, out[1] verification groups, out[2] items re-checked
 * alone because their group's combined check failed, out[3] groups checked alone because their
 * batch's shared final exponentiation failed, out[4] slot-wide checks run, out[5] slot-wide
 * checks that failed (the call then took the per-batch check), out[6] ThresholdAggregate /
 * Aggregate members looked up in the decompressed-signature cache, out[7] those found.  n <= 8. */
int hbls_stats(uint64_t* out, size_t n);
/* Tuning: verifications of at least min_groups groups share one final exponentiation among 64
 * groups (0 = one per group; default 128, HBLS_FE_BATCH).  Returns the previous value.  Verdicts
 * do not depend on it. */
size_t hbls_fe_batch(size_t min_groups);
/* Tuning: batched verifications of at least min_items items (partials + folded aggregates) first
 * check every group at once -- the signature side as one multi-scalar multiplication, one final
 * exponentiation for the call -- and take the per-batch check only if that fails (0 = never;
 * default 32768, HBLS_SLOT_MSM).  Returns the previous value and clears the adaptive history
 * below.  Verdicts do not depend on it. */
size_t hbls_slot_msm(size_t min_items);
/* Tuning: adaptive slot-wide check (1 = on, the default; HBLS_ADAPTIVE): after a call whose
 * slot-wide check failed, the next calls take the per-batch check directly until one passes every
 * batch.  Returns the previous setting.  Verdicts do not depend on it. */
int hbls_adaptive(int on);
/* Tuning: device-buffer verifications of at least min_items items that decompress all their
 * signatures test them for G2 membership at once -- five bucket entries per signature and 20
 * tested sums, each a combination with random coefficients below 13 -- and run the per-item
 * ladders only if a sum fails (0 = never; default 524288, HBLS_SUBGROUP_BATCH).  With
 * hbls_adaptive on, after a call whose batched test failed the next calls take the ladders
 * directly until one of them finds every signature in G2.  Returns the previous value and clears
 * that history.  Verdicts, statuses and outputs do not depend on it.
 * hbls_subgroup_batch_stats: per device (at most max_devices; *n_devices = the number written)
 * four cumulative values: out[4k] batched tests run, out[4k+1] batched tests that failed,
 * out[4k+2] signatures of such calls that went through the per-item ladders, out[4k+3] calls that
 * skipped the test by the history.  Waits for the library's enqueued work on each device. */
size_t hbls_subgroup_batch(size_t min_items);
int hbls_subgroup_batch_stats(uint64_t* out, size_t max_devices, size_t* n_devices);
/* Host Verify batches of fewer than `items` check every item alone (no random-combination ladder
 * on the latency path); SIZE_MAX = the default (the batched final exponentiation's threshold).
 * Returns the previous setting (HBLS_SINGLE_MAX at init).  Verdicts never depend on it. */
size_t hbls_single_max(size_t items);
/* Tuning: decompressions of at most `items` keys or signatures run their subgroup checks with each
 * item's ladder split over a lane pair (latency for calls that do not fill the chip; 0 = never, the
 * default, HBLS_DEC_PAIR_MAX).  Returns the previous value.  Verdicts do not depend on it. */
size_t hbls_dec_pair_max(size_t items);
/* Tuning by name (read from the environment at init; verdicts and outputs never depend on them):
 * the layouts of the latency-bound small calls "HBLS_HASH_PAIR_MAX", "HBLS_HASH_ONE_LANE",
 * "HBLS_HASH_SPLIT" (0: the unstaged hashing kernels), "HBLS_FE18_MAX", "HBLS_TA_PAIR_MAX",
 * "HBLS_DEC_PAIR_MAX"; the chunking of large verifications "HBLS_GROUP_CHUNK" (groups per pairing
 * chunk), "HBLS_FALLBACK_CHUNK" (items per fallback pass), "HBLS_GROUP_MAX" (items per group of a
 * host call); "HBLS_KEY_LEARN" (entries of the learned key cache, 0 = off: a new value empties the
 * table after waiting for the library's enqueued work); "HBLS_KEY_WIDE" (how many of those entries
 * get a ladder table, 0 = none: a new value empties the cache likewise).  *previous (if not NULL) receives the old
 * value.  Returns 0, or -1 for an unknown name. */
int hbls_tune(const char* name, size_t value, size_t* previous);
/* Tuning: the random linear combination's public-key side groups a verification group's items
 * into shared-doubling chunks sized to keep about `lanes` lanes busy (at most 16 items per chunk;
 * calls of fewer than 2 lanes' worth keep one ladder per item).  0 restores the default 65536
 * (HBLS_RLC_LANES).  Returns the previous value.  Verdicts do not depend on it. */
size_t hbls_rlc_lanes(size_t lanes);
/* Tuning: ThresholdAggregate calls whose groups all have t members run joint ladders over chunks
 * of `members` (<= 8) members of a validator, sharing the doublings; 0 = auto (HBLS_TA_JOINT), 1 =
 * one ladder per member.  Returns the previous value.  Outputs do not depend on it. */
size_t hbls_ta_joint(size_t members);
/* Wait for all work the library queued on `stream`. */
int hbls_sync(void* stream);
/* Device: the verify bitmap of n statuses (bit i of bits[i / 8], least significant bit first, set
 * when status[i] == HBLS_OK; bits holds ceil(n / 8) bytes), on `stream` -- the compact form of a
 * slot's verdicts that the ranks all-gather (north_star: "all-gather verify bitmaps"); the
 * failure classes stay in the owning rank's status bytes. */
int hbls_status_bitmap(const uint8_t* status, size_t n, uint8_t* bits, void* stream);

/* ---------------------------------------------------------------------------------------
 * Exchange of slot results between processes that drive one GPU each:
 * RCCL over xGMI.  Rank 0 creates the id, every rank passes it to hbls_comm_init, then
 * hbls_allgather_device gathers `bytes` from every rank into recv (rank order) on `stream`.
 * --------------------------------------------------------------------------------------- */
size_t hbls_comm_id_bytes(void);
int hbls_comm_unique_id(uint8_t* id);
int hbls_comm_init(int nranks, int rank, const uint8_t* id);
int hbls_allgather_device(const void* send, void* recv, size_t bytes, void* stream);
/* The number of ranks of the communicator as RCCL reports it (ncclCommCount), 0 without one:
 * bench.py puts it in its line beside n_gpus. */
int hbls_comm_size(void);
int hbls_comm_destroy(void);

#ifdef __cplusplus
}
#endif
#endif /* HIPBLS_H */
