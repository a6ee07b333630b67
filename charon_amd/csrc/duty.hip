// Duty sessions (hbls_duty_add; hipbls.hip duty_add_shard): what an arriving set does to the
// validators' resident state, behind the verification's final verdicts.
//   k_duty_store  1 lane / touched group: the rule (dutysel.h duty_store_group) over the group's new
//                 partials in arrival order -> stored[], the record updates, the list of (destination
//                 slot, source item) copies and the list of fired groups, each compacted with one
//                 atomicAdd per wave (as vbatch.hip k_pk_lookup compacts its misses)
//   k_duty_copy   16 lanes / listed copy, 13 of them moving 16 bytes each: the stored partials'
//                 decompressed points from the verification's workspace into the duty's store
//   k_duty_gather 1 lane / fired group, in ascending group order (the host sorted the list): its
//                 members, share indices, class key and message into the tables threshold.hip's
//                 k_ta_sel_fill reads, its members' serials and its DV key (none for a duty on a cluster)
// hbls_duty_add_sets puts two kernels between the verification and k_duty_store:
//   k_duty_set_first 1 lane / item: a lane whose verification failed folds its arrival index into its
//                 set's entry of set_first with atomicMin; the failing lanes of a wave that share a
//                 set combine first (one atomic per distinct failing set of the wave, none on a clean add)
//   k_duty_gate   1 lane / item: the status byte k_duty_store reads (dutysel.h duty_admit), so that no
//                 partial of a rejected set is admitted
// The aggregation itself is threshold.hip's, over the duty's store.
#include <hip/hip_runtime.h>

#include "dutysel.h"
#include "layout.h"

namespace hb {

static_assert(DUTY_MAX_T == TASEL_MAX, "dutysel.h restates tasel.h");
static_assert(sizeof(HmEntry) % 16 == 0 && sizeof(HmEntry) / 16 <= 16, "k_duty_copy: 16 lanes of 16 bytes per point");

static inline unsigned duty_blocks(size_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }

__global__ __launch_bounds__(64) void k_duty_store(DutyStoreArgs a) {
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  // a group outside the shard is never an address (the host plan lists none)
  const uint32_t g = u < a.n_touched ? a.tgroup[u] : DUTY_NONE;
  const bool valid = g < a.n_groups;
  uint32_t b = 0, e = 0;
  DutyStep st{};
  if (valid) {
    b = min(a.toff[u], a.n_pos);
    e = min(max(a.toff[u + 1], b), a.n_pos);
    const size_t r0 = (size_t)g * a.max_stored;
    const DutyRecords r{a.rec_idx + r0, a.rec_msg + r0, a.rec_serial + r0, a.count + g, a.fired + g};
    const size_t m0 = (size_t)u * a.t;
    st = duty_store_group(r, a.max_stored, a.t, a.vstatus, a.msg_idx, a.serial, a.n, a.tpos, a.tidx, b, e, a.stored,
                          a.slot, a.mslot + m0, a.mserial + m0, a.midx + m0);
    if (st.fired) {
      a.fmsg[u] = st.msg;
      a.fkey[u] = st.key;
    }
  }
  // the copies: an inclusive scan of the lanes' counts, one atomicAdd for the wave
  uint32_t x = st.n_stored;
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  const uint32_t total = __shfl(x, 63);
  const uint64_t fm = __ballot(st.fired != 0);
  uint32_t full = st.n_full;
  for (uint32_t d = 32; d; d >>= 1) full += __shfl_xor(full, d);
  uint32_t cbase = 0, fbase = 0;
  if (lane == 0) {
    if (total) cbase = atomicAdd(a.ctr + DUTY_CTR_COPIES, total);
    if (fm) fbase = atomicAdd(a.ctr + DUTY_CTR_FIRED, (uint32_t)__popcll(fm));
    if (full) atomicAdd(a.ctr + DUTY_CTR_FULL, full);
  }
  cbase = __shfl(cbase, 0);
  fbase = __shfl(fbase, 0);
  if (st.fired) {
    const uint32_t k = fbase + __popcll(fm & ((1ull << lane) - 1));
    if (k < a.n_touched) a.fired_u[k] = u;
  }
  uint32_t k = cbase + x - st.n_stored;
  for (uint32_t j = b; j < e; j++) {  // (b == e for a lane without a group)
    const uint32_t q = a.tpos[j];
    if (q >= a.n || a.slot[q] == DUTY_NONE) continue;
    if (k < a.n) a.copies[k] = make_uint2(g * a.max_stored + a.slot[q], q);
    k++;
  }
}

__global__ __launch_bounds__(64) void k_duty_set_first(const uint8_t* __restrict__ vstatus, const uint32_t* __restrict__ set_id,
                                                       const uint32_t* __restrict__ arrival, uint32_t n,
                                                       uint32_t* __restrict__ set_first, uint32_t n_sets) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  // a set id outside the call's sets is never an address (the host plan gives none)
  const uint32_t sid = q < n ? set_id[q] : DUTY_NONE;
  const bool fail = q < n && sid < n_sets && vstatus[q] != 0;
  const uint32_t arr = fail ? arrival[q] : DUTY_NONE;
  uint64_t todo = __ballot(fail);  // wave-uniform: every lane walks the same leaders
  while (todo) {
    const int leader = __ffsll((unsigned long long)todo) - 1;
    const uint32_t s0 = __shfl(sid, leader);
    const bool mine = fail && sid == s0;
    uint32_t v = mine ? arr : DUTY_NONE;
    for (uint32_t d = 32; d; d >>= 1) v = min(v, (uint32_t)__shfl_xor(v, d));
    if (lane == (uint32_t)leader) atomicMin(set_first + s0, v);
    todo &= ~__ballot(mine);
  }
}

__global__ __launch_bounds__(64) void k_duty_gate(const uint8_t* __restrict__ vstatus, const uint32_t* __restrict__ set_id,
                                                  uint32_t n, const uint32_t* __restrict__ set_first, uint32_t n_sets,
                                                  uint8_t* __restrict__ admit) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  admit[q] = duty_admit(vstatus[q], set_id[q], set_first, n_sets);
}

__global__ __launch_bounds__(256) void k_duty_copy(const HmEntry* __restrict__ src, uint32_t n_src,
                                                   const uint2* __restrict__ copies, const uint32_t* __restrict__ count,
                                                   uint32_t max_copies, HmEntry* __restrict__ store, uint32_t n_slots) {
  constexpr uint32_t W = sizeof(HmEntry) / 16;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t c = i >> 4, l = i & 15u;
  if (c >= min(*count, max_copies) || l >= W) return;
  const uint2 cp = copies[c];
  if (cp.x >= n_slots || cp.y >= n_src) return;
  reinterpret_cast<uint4*>(store)[(size_t)cp.x * W + l] = reinterpret_cast<const uint4*>(src)[(size_t)cp.y * W + l];
}

__global__ __launch_bounds__(64) void k_duty_gather(DutyGatherArgs a) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= a.n_fired) return;
  const uint32_t u = min(a.frow[k], a.n_touched - 1);
  const uint32_t g = min(a.tgroup[u], a.n_groups - 1);
  for (uint32_t j = 0; j < a.t; j++) {
    const uint32_t s = min(a.mslot[(size_t)u * a.t + j], a.max_stored - 1);
    a.chosen[(size_t)k * a.t + j] = g * a.max_stored + s;
    a.cidx[(size_t)k * a.t + j] = a.midx[(size_t)u * a.t + j];
    a.serials[(size_t)k * a.t + j] = a.mserial[(size_t)u * a.t + j];
  }
  const uint32_t key = a.fkey[u] & 0xffffu;
  a.key[k] = key;
  a.state[k] = TASEL_OK;
  a.gmsg[k] = a.fmsg[u];
  atomicAdd(a.hist + key, 1u);
  a.fired_g[k] = a.group_base + g;
  if (!a.dv_pks) return;  // a cluster duty: the DV keys come from the cluster by fired_g
  const uint4* in = reinterpret_cast<const uint4*>(a.dv_pks) + 3ull * g;
  uint4* o = reinterpret_cast<uint4*>(a.dv_out) + 3ull * k;
  HB_UNROLL for (int w = 0; w < 3; w++) o[w] = in[w];
}

void launch_duty_store(const DutyStoreArgs& a, hipStream_t s) {
  if (!a.n_touched) return;
  hipLaunchKernelGGL(k_duty_store, dim3(duty_blocks(a.n_touched, 64)), dim3(64), 0, s, a);
}
void launch_duty_set_first(const uint8_t* vstatus, const uint32_t* set_id, const uint32_t* arrival, uint32_t n,
                           uint32_t* set_first, uint32_t n_sets, hipStream_t s) {
  if (!n || !n_sets) return;
  hipLaunchKernelGGL(k_duty_set_first, dim3(duty_blocks(n, 64)), dim3(64), 0, s, vstatus, set_id, arrival, n, set_first,
                     n_sets);
}
void launch_duty_gate(const uint8_t* vstatus, const uint32_t* set_id, uint32_t n, const uint32_t* set_first,
                      uint32_t n_sets, uint8_t* admit, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_duty_gate, dim3(duty_blocks(n, 64)), dim3(64), 0, s, vstatus, set_id, n, set_first, n_sets, admit);
}
void launch_duty_copy(const HmEntry* src, uint32_t n_src, const uint2* copies, const uint32_t* count, uint32_t max_copies,
                      HmEntry* store, uint32_t n_slots, hipStream_t s) {
  if (!max_copies) return;
  hipLaunchKernelGGL(k_duty_copy, dim3(duty_blocks((size_t)max_copies * 16, 256)), dim3(256), 0, s, src, n_src, copies,
                     count, max_copies, store, n_slots);
}
void launch_duty_gather(const DutyGatherArgs& a, hipStream_t s) {
  if (!a.n_fired) return;
  hipLaunchKernelGGL(k_duty_gather, dim3(duty_blocks(a.n_fired, 64)), dim3(64), 0, s, a);
}

}  // namespace hb
