// Segmented first-error verification (hbls_duty_add_sets_first; hipbls.hip verify_pipeline with
// VerifyCall::gseg): the first-error kernels of vgroup.hip / vbatch.hip with one first failure per
// segment of the call's groups instead of one per call.  The rule and its exactness argument are
// dutyfirst.h's; each kernel below is one lane per group or item calling it.
//   k_seg_first_batch   before the verdicts: sfirst[2k] = the smallest failing batch with a READY group
//                       of segment k that is not k's head batch
//   k_seg_batch_verdict k_batch_verdict with the rule: a group of a failing batch joins the list iff
//                       its batch is its segment's head batch or first[k]; else GV_UNCHECKED
//   k_seg_first_group   sfirst[2k + 1] = the smallest group of k whose own check failed
//   k_seg_scatter       k_scatter's item branch (no folded aggregates): only the items of a segment's
//                       first failing group are re-checked alone, those of its other failing or
//                       unchecked groups get ST_UNCHECKED
//   k_seg_first_item    set_first[k] = the smallest arrival index of k whose status is decided and not OK
// The mins are atomicMin on words preset to 0xff bytes.  As in duty.hip's k_duty_set_first the voting
// lanes of a wave that share a segment combine first: one atomic per distinct voting segment of the
// wave, none when nothing fails.  A segment id is checked against n_seg before it indexes anything.
#include <hip/hip_runtime.h>

#include "dutyfirst.h"
#include "layout.h"

namespace hb {

static_assert(SEG_PASS == GV_PASS && SEG_UNCHECKED == GV_UNCHECKED && SEG_NOT_READY == GV_NOT_READY,
              "dutyfirst.h restates layout.h");

// Every lane of the wave calls this.  A voting lane folds v into words[stride k]; k < the words' count
// is the caller's check (a lane with k out of range does not vote).
__device__ __forceinline__ void seg_wave_min(bool vote, uint32_t k, uint32_t v, uint32_t* __restrict__ words,
                                             uint32_t stride) {
  const uint32_t lane = threadIdx.x & 63u;
  uint64_t todo = __ballot(vote);  // wave-uniform: every lane walks the same leaders
  while (todo) {
    const int leader = __ffsll((unsigned long long)todo) - 1;
    const uint32_t k0 = __shfl(k, leader);
    const bool mine = vote && k == k0;
    uint32_t x = mine ? v : SEG_NONE;
    for (uint32_t d = 32; d; d >>= 1) x = min(x, (uint32_t)__shfl_xor(x, d));
    if (lane == (uint32_t)leader) atomicMin(words + (size_t)stride * k0, x);
    todo &= ~__ballot(mine);
  }
}

// gseg: the segment of every group of the call (indexed g0 + lg); gst / bver: the chunk's
__global__ __launch_bounds__(64) void k_seg_first_batch(const uint8_t* __restrict__ gst, const uint8_t* __restrict__ bver,
                                                         uint32_t ng, const uint8_t* __restrict__ guard, uint32_t fb,
                                                         uint32_t g0, const uint32_t* __restrict__ gseg, uint32_t n_seg,
                                                         uint32_t* __restrict__ sfirst) {
  if (guard && *guard == 0) return;
  const uint32_t lg = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = lg < ng;
  const uint32_t key = in ? seg_batch_key(g0, lg, fb) : 0;
  const bool vote = in && gst[lg] == G_READY && bver[lg / fb] != 0 && seg_votes(gseg, n_seg, key, g0 + lg);
  seg_wave_min(vote, vote ? gseg[g0 + lg] : SEG_NONE, key, sfirst, 2);
}

__global__ __launch_bounds__(64) void k_seg_batch_verdict(const uint8_t* __restrict__ gst, const uint8_t* __restrict__ bver,
                                                           uint32_t ng, uint8_t* __restrict__ gver,
                                                           uint32_t* __restrict__ list, uint32_t* __restrict__ count,
                                                           const uint8_t* __restrict__ guard, uint32_t fb, uint32_t g0,
                                                           const uint32_t* __restrict__ gseg, uint32_t n_seg,
                                                           const uint32_t* __restrict__ sfirst) {
  if (guard && *guard == 0) return;
  const uint32_t lg = blockIdx.x * blockDim.x + threadIdx.x;
  if (lg >= ng) return;
  const uint8_t v = seg_group_verdict(gst[lg] == G_READY, bver[lg / fb] != 0, gseg, n_seg, sfirst,
                                      seg_batch_key(g0, lg, fb), g0 + lg);
  if (v == SEG_DESCEND) list[atomicAdd(count, 1u)] = lg;
  else gver[lg] = v;
}

__global__ __launch_bounds__(64) void k_seg_first_group(const uint8_t* __restrict__ gver, uint32_t n_groups,
                                                         const uint32_t* __restrict__ gseg, uint32_t n_seg,
                                                         uint32_t* __restrict__ sfirst) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t k = g < n_groups ? gseg[g] : SEG_NONE;
  const bool vote = g < n_groups && k < n_seg && gv_failed(gver[g]);
  seg_wave_min(vote, k, g, sfirst + 1, 2);
}

__global__ __launch_bounds__(64) void k_seg_scatter(ScatterArgs a, const uint32_t* __restrict__ gseg, uint32_t n_seg,
                                                     const uint32_t* __restrict__ sfirst) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const uint32_t g = a.item_grp[i];
  uint8_t s;
  if (a.pk_st[i]) s = ST_BAD_PUBKEY;
  else if (a.sig_st[i]) s = ST_BAD_SIGNATURE;
  else if (a.pk[i].inf || a.sig[i].inf || a.hm[a.msg_idx[i]].h.inf) s = ST_NOT_VERIFIED;  // verify_core
  else if (a.gverdict[g] == GV_PASS) s = ST_OK;
  else if (seg_item_unchecked(a.gverdict[g], gseg, n_seg, sfirst, g)) s = ST_UNCHECKED;
  else if (!a.grp_off || a.grp_off[g + 1] - a.grp_off[g] <= 1) s = ST_NOT_VERIFIED;  // a group of one item
  else {
    a.list[atomicAdd(a.count, 1u)] = i;
    return;
  }
  a.status[i] = s;
}

__global__ __launch_bounds__(64) void k_seg_first_item(const uint8_t* __restrict__ status, const uint32_t* __restrict__ item_seg,
                                                        const uint32_t* __restrict__ arrival, uint32_t n,
                                                        uint32_t* __restrict__ set_first, uint32_t n_seg) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t k = q < n ? item_seg[q] : SEG_NONE;
  const bool vote = q < n && k < n_seg && status[q] != ST_OK && status[q] != ST_UNCHECKED;
  seg_wave_min(vote, k, vote ? arrival[q] : SEG_NONE, set_first, 1);
}

void launch_seg_batch_verdict(const uint8_t* gst, const uint8_t* bver, uint32_t ng, uint8_t* gver, uint32_t* list,
                              uint32_t* count, hipStream_t s, const uint8_t* guard, uint32_t fe_batch, uint32_t g0,
                              const uint32_t* gseg, uint32_t n_seg, uint32_t* sfirst) {
  if (!ng) return;
  const uint32_t fb = fe_batch ? fe_batch : FE_BATCH;
  hipLaunchKernelGGL(k_seg_first_batch, dim3((ng + 63) / 64), dim3(64), 0, s, gst, bver, ng, guard, fb, g0, gseg, n_seg,
                     sfirst);
  hipLaunchKernelGGL(k_seg_batch_verdict, dim3((ng + 63) / 64), dim3(64), 0, s, gst, bver, ng, gver, list, count, guard, fb,
                     g0, gseg, n_seg, (const uint32_t*)sfirst);
}
void launch_seg_first_group(const uint8_t* gver, uint32_t n_groups, const uint32_t* gseg, uint32_t n_seg, uint32_t* sfirst,
                            hipStream_t s) {
  if (n_groups)
    hipLaunchKernelGGL(k_seg_first_group, dim3((n_groups + 63) / 64), dim3(64), 0, s, gver, n_groups, gseg, n_seg, sfirst);
}
void launch_seg_scatter(const ScatterArgs& a, const uint32_t* gseg, uint32_t n_seg, const uint32_t* sfirst, hipStream_t s) {
  if (a.n) hipLaunchKernelGGL(k_seg_scatter, dim3((a.n + 63) / 64), dim3(64), 0, s, a, gseg, n_seg, sfirst);
}
void launch_seg_first_item(const uint8_t* status, const uint32_t* item_seg, const uint32_t* arrival, uint32_t n,
                           uint32_t* set_first, uint32_t n_seg, hipStream_t s) {
  if (n && n_seg)
    hipLaunchKernelGGL(k_seg_first_item, dim3((n + 63) / 64), dim3(64), 0, s, status, item_seg, arrival, n, set_first, n_seg);
}

}  // namespace hb
