// The plan of one verification (hipbls.hip verify_pipeline): which of its paths a call takes and
// the sizes that follow, decided once from the call's shape, the device and a snapshot of the
// knobs.  Host code only (no HIP) and plain values in, so that tests/native/hostcheck.cpp fills
// plans on the CPU (tests/test_vplan.py: a table of shapes, and the implications between the
// fields over random inputs).  The phases of verify_pipeline read the plan; none derives a mode
// of its own.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace hb {

// layout.h's values (that header needs HIP; hipbls.hip asserts that these agree with it)
constexpr size_t VP_GROUPS_PER_WAVE = 21;  // GROUPS_PER_WAVE
constexpr size_t VP_PROD_FAN = 8;          // PROD_FAN
constexpr size_t VP_RLC_CHUNK = 16;        // RLC_CHUNK

// the knobs a plan depends on, read once per call
struct VerifyKnobs {
  size_t gcap, fbcap;   // HBLS_GROUP_CHUNK, HBLS_FALLBACK_CHUNK
  size_t fe_batch_min;  // HBLS_FE_BATCH
  size_t slot_msm_min;  // HBLS_SLOT_MSM
  size_t rlc_lanes;     // HBLS_RLC_LANES
  bool adaptive;        // HBLS_ADAPTIVE
  size_t subg_batch_min = 0;  // HBLS_SUBGROUP_BATCH (0 = never)
};

struct VerifyShape {
  size_t n, n_groups;  // items; verification groups (ignored unless grouped)
  size_t n_agg;        // folded aggregates (post-aggregate verification)
  bool grouped;        // group offsets given (else every item is its own group)
  bool first_error;    // first-error mode asked for
  size_t defer_msgs;   // messages whose Miller lines the caller left uncomputed
  int n_cu;            // the device's compute units
  bool attack;         // the device's adaptive history: the last known call had items a pairing caught
  // the call decompresses its own signatures, all of them, from a device-buffer entry point (no
  // signatures handed over decompressed, no signature-cache hits to skip)
  bool own_sigs = false;
  bool subg_failed = false;  // the adaptive history: the last known call had signatures off G2
};

struct VerifyPlan {
  size_t n, n_groups, n_agg;  // n_groups: n when the call gave no group offsets
  size_t gcap, fbcap;         // groups per chunk of the group checks, items per fallback pass
  bool bfe;                   // batched final exponentiation
  int item_always;            // every item takes a random coefficient
  bool first_only;            // first-error mode descends only into the first failure
  size_t mmlk, nb1, nb2, nbcap;
  bool smsm;      // the slot-wide check applies (one chunk of groups, large enough)
  bool adaptive;  // the call's outcome is recorded for the next calls' choice
  bool skip_msm;  // ... but the adaptive history says it would fail: straight to the per-batch check
  bool try_msm;   // smsm && !skip_msm: the MSM takes the signature side
  int sides1;     // sides of the first combination: 1 = keys only, 3 = both
  uint32_t rlc_cmax;
  bool rlc_chunked;  // the chunked combination (k_plan, k_rlc_msm) instead of the per-item one
  bool keys_only, sparse, lines_at_p;
  // the signatures' subgroup checks as one batched test (msm.hip k_subg_*), the per-item ladders
  // behind its flag; subg_skip: ... but the adaptive history says it would fail, so the ladders
  // run unguarded and count what they find
  bool subg_batch, subg_skip;
};

inline size_t vp_groups(const VerifyShape& in) { return in.grouped ? in.n_groups : in.n; }
inline size_t vp_gcap(const VerifyShape& in, const VerifyKnobs& k) {
  return std::min(std::max<size_t>(1, k.gcap), std::max<size_t>(vp_groups(in), 1));
}
inline bool vp_bfe(const VerifyShape& in, const VerifyKnobs& k) {
  return k.fe_batch_min && vp_groups(in) >= k.fe_batch_min;
}
// Slot-wide check (msm.hip): every group of the call at once, the signature side as one
// multi-scalar multiplication; the per-batch path runs only if it fails (its kernels wait on the
// device flag sfail).  Needs all groups in one chunk.  (Apart from the plan: the adaptive history
// is read only by calls this holds for, before they plan.)
inline bool vp_slot_wide(const VerifyShape& in, const VerifyKnobs& k) {
  return vp_bfe(in, k) && k.slot_msm_min && vp_groups(in) <= vp_gcap(in, k) && in.n + in.n_agg >= k.slot_msm_min;
}

// Batched subgroup test: large calls that decompress all their signatures themselves.  (Apart from
// the plan: its adaptive history is read only by calls this holds for, before they plan.)
inline bool vp_subg_wide(const VerifyShape& in, const VerifyKnobs& k) {
  return in.own_sigs && k.subg_batch_min && in.n >= k.subg_batch_min;
}

// Fills p; returns null, or the reason the call is refused.
inline const char* verify_plan(const VerifyShape& in, const VerifyKnobs& k, VerifyPlan& p) {
  p.n = in.n;
  p.n_groups = vp_groups(in);
  p.n_agg = in.n_agg;
  p.gcap = vp_gcap(in, k);
  p.fbcap = std::min(std::max<size_t>(1, k.fbcap), std::max<size_t>(p.n + p.n_agg, 1));
  // Coefficients: at most ONE fixed (r = 1) coefficient per combined check.  Items of a singleton
  // group keep r = 1 only when nothing else joins their group's check; with a folded aggregate
  // (which keeps r = 1 without the batched final exponentiation) every item takes a random one --
  // otherwise an error +D on a group's single partial and -D on its aggregate would cancel.
  // Batched final exponentiation: a batch of groups (FE_BATCH; behind a failed slot-wide check the
  // multi-Miller loops' chunks of mmlk groups) shares one final exponentiation and one Miller
  // loop of the signature side, checking prod_g e(P_g, H(m_g)) * e(-g1, sum_g S_g) == 1.  Every
  // item (singletons and folded aggregates included) then takes a random coefficient: with two
  // fixed coefficients in one combination, errors of two items could cancel.
  p.bfe = vp_bfe(in, k);
  p.item_always = (p.bfe || p.n_agg) ? 1 : 0;  // see the coefficient rule above
  // First-error mode (the callers' contract: parsigex.go:93-98, sigagg.go:56-63 stop at the first
  // failing item): behind a failed combined check only the FIRST failing batch descends to its
  // groups and only the first failing group to its items -- groups and batches are in item order,
  // so every item before the first failure has passed a check and every item left unresolved
  // (ST_UNCHECKED) comes after it.  Without the batched final exponentiation every group is
  // checked anyway (exact statuses).
  if (in.first_error && p.n_agg) return "verify: the first-error mode takes no folded aggregates";
  p.first_only = in.first_error && p.bfe;
  // pairs per multi-Miller loop of the slot-wide check: enough that the loops fill at most one
  // round of waves (21 groups per wave, one wave per SIMD) -- a second, partial round would double
  // the kernel's span
  const size_t round = VP_GROUPS_PER_WAVE * 4 * (size_t)in.n_cu;
  p.mmlk = std::min<size_t>(16, std::max<size_t>(1, (std::min(p.gcap, p.n_groups) + round - 1) / round));
  p.nb1 = (p.gcap + p.mmlk - 1) / p.mmlk;
  p.nb2 = (p.nb1 + VP_PROD_FAN - 1) / VP_PROD_FAN;
  // batches of >= 2 groups (FE_BATCH), or behind a failed slot-wide check its multi-Miller loops' chunks
  p.nbcap = std::max((p.gcap + 1) / 2, p.nb1);
  p.smsm = vp_slot_wide(in, k);
  // adaptive: the outcome of the last completed checked call decides whether this one tries the
  // slot-wide check at all (skip: the fallback's kernels run unguarded, sfail set to 1)
  p.adaptive = k.adaptive;
  p.skip_msm = p.smsm && k.adaptive && in.attack;
  p.try_msm = p.smsm && !p.skip_msm;
  // first pass: the public-key side only when the MSM takes the other
  p.sides1 = p.try_msm ? 1 : 3;
  // chunks of a group's items share their ladders' doublings (k_rlc_msm); the chunk size keeps
  // about rlc_lanes lanes busy (at most RLC_CHUNK items, one item per lane for small calls)
  p.rlc_cmax = (uint32_t)std::min<size_t>(VP_RLC_CHUNK, std::max<size_t>(1, p.n / k.rlc_lanes));
  p.rlc_chunked = in.grouped && p.rlc_cmax > 1;
  // the partials' key side from the keys alone when the slot-wide MSM takes the signature side
  // (sides1 1, the per-lane combination): it runs beside the signatures' subgroup checks, whose
  // statuses group_scan and msm_take apply; otherwise the signatures' statuses first
  p.keys_only = p.sides1 == 1 && !p.rlc_chunked;
  // the sparse coefficient format (22 additions per item instead of 32) unless the slot-wide
  // bucket MSM reads the coefficients: under attack (skip_msm), or a chunked call without the
  // slot-wide check (HBLS_SLOT_MSM above its size)
  p.sparse = !p.try_msm;
  if (in.defer_msgs && !p.bfe) return "verify: deferred Miller lines need the batched final exponentiation";
  // deferred lines: the slot-wide check evaluates each group's chain at P directly (k_lines_at_p);
  // any other path computes the messages' lines first
  p.lines_at_p = in.defer_msgs && p.try_msm;
  // a failed batched test costs its pass and then the ladders as well: after one, the next calls
  // ladder every item until one of them finds every signature in G2
  p.subg_skip = vp_subg_wide(in, k) && k.adaptive && in.subg_failed;
  p.subg_batch = vp_subg_wide(in, k) && !p.subg_skip;
  return nullptr;
}

}  // namespace hb
