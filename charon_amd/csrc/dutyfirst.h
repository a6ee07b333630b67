// The descent rule of a segmented first-error verification (hbls_duty_add_sets_first): which groups of
// a failing batch are checked one by one when the call's groups are cut into ordered segments (a
// duty call's sets) and each segment wants its own first failure.
//
// The groups of a call are in segment-major order and, within a segment, in arrival order (hduty.h
// duty_plan_shard with set ids: a group belongs to exactly one segment).  Batches are fb consecutive
// groups of a chunk (g0: the chunk's first group) and do not stop at segment boundaries; a batch is
// named by its key, the index of its first group (g0 + (lg / fb) fb).  A batch fails when one of
// its READY groups does.
//
// With one segment the first failing batch certainly holds a failing group of it (vplan.h first_only).
// With several it need not: a batch that straddles segments k - 1 and k can fail through k - 1 alone,
// and segment k's real first failure then sits in a later batch.  Hence the rule:
//   * the HEAD batch of segment k is the batch of its first group when that batch begins with a group
//     of an earlier segment -- for a group g of k in batch B: gseg[B] != k;
//   * first[k] is the smallest failing batch with a READY group of k that is NOT k's head batch (one
//     atomicMin per segment, sfirst[2k]);
//   * a READY group of k in a failing batch B descends (is checked alone) iff B is k's head batch or
//     B == first[k]; every other group of a failing batch stays GV_UNCHECKED.  At most two batches
//     per segment descend;
//   * the segment's first failing group is the smallest descended group whose own check failed (a second
//     atomicMin per segment, sfirst[2k + 1]); only its items are re-checked alone, the items of the
//     other failing or unchecked groups get ST_UNCHECKED.
// Exactness.  Let G* be the first READY group of k, in arrival order, whose own check would fail, in
// batch B* (which then fails).  If B* is k's head batch it descends.  Otherwise first[k] <= B*.  Every
// non-head batch of k before first[k] passed, so its groups of k pass; batch first[k] descends, so its
// groups of k are checked alone.  If none of them fails, first[k] failed through another segment's
// groups -- later ones, since first[k] begins with a group of k -- so k ends inside first[k] and has no
// group behind it: G* does not exist outside the head batch.  If one fails, G* is at or before it.
// Either way G* (when it exists) was checked alone, every group of k before it passed a batch check
// or its own, and every group left GV_UNCHECKED comes after it.  Groups that are not READY take the
// exact per-item fallback as ever, and decoding failures are exact everywhere, so the smallest item of
// k whose status is decided and not OK (ST_UNCHECKED skipped) is k's first failing item, and every
// item before it is OK.
//
// No HIP in here: dutyfirst.hip's kernels call these per lane, and the CPU harness
// tests/native/dutyfirstcheck.cpp compiles the same functions for tests/test_duty_first_host.py.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DUTYFIRST_HD __host__ __device__ inline
#else
#define DUTYFIRST_HD inline
#endif

namespace hb {

constexpr uint32_t SEG_NONE = 0xffffffffu;
// what seg_group_verdict answers (the first three are layout.h's GV_PASS / GV_UNCHECKED / GV_NOT_READY)
constexpr uint8_t SEG_PASS = 0, SEG_UNCHECKED = 0x80, SEG_NOT_READY = 0x81, SEG_DESCEND = 0xff;

// the key of group lg's batch in the chunk that starts at group g0
DUTYFIRST_HD uint32_t seg_batch_key(uint32_t g0, uint32_t lg, uint32_t fb) { return g0 + (lg / fb) * fb; }

// Group g (of segment gseg[g]) sits in a failing batch `key` and is READY: does it vote for first[k]?
// Not in its head batch, and never with a segment id outside the call's (which indexes nothing).
DUTYFIRST_HD bool seg_votes(const uint32_t* gseg, uint32_t n_seg, uint32_t key, uint32_t g) {
  const uint32_t k = gseg[g];
  return k < n_seg && gseg[key] == k;
}

// The verdict of group g in batch `key`: not READY, in a passing batch, left unchecked, or descends.
// sfirst[2k]: first[k] as the votes left it.
DUTYFIRST_HD uint8_t seg_group_verdict(bool ready, bool batch_failed, const uint32_t* gseg, uint32_t n_seg,
                                       const uint32_t* sfirst, uint32_t key, uint32_t g) {
  if (!ready) return SEG_NOT_READY;
  if (!batch_failed) return SEG_PASS;
  const uint32_t k = gseg[g];
  if (k >= n_seg) return SEG_UNCHECKED;
  return (gseg[key] != k || sfirst[2 * k] == key) ? SEG_DESCEND : SEG_UNCHECKED;
}

// An item of group g whose verdict gv is not a pass: left ST_UNCHECKED (true), or resolved alone?
// sfirst[2k + 1]: segment k's first failing group.
DUTYFIRST_HD bool seg_item_unchecked(uint8_t gv, const uint32_t* gseg, uint32_t n_seg, const uint32_t* sfirst,
                                     uint32_t g) {
  if (gv == SEG_UNCHECKED) return true;
  if (gv == SEG_PASS || gv >= SEG_UNCHECKED) return false;  // passed, or not READY: the exact fallback
  const uint32_t k = gseg[g];
  return k >= n_seg || sfirst[2 * k + 1] != g;
}

}  // namespace hb
