// hbls_cluster_check (the rule is lockcheck.h's): do the pubshares of a cluster's rows interpolate to
// their DV keys -- the t-th forward differences of every row over the shard's resident, read-only keys.
//   k_lock_check  1 lane / (row, window), lane = row * W + k: D_k = sum_i c_i P_{k+i} by one joint
//                 MSB-first ladder over the t + 1 affine entries k .. k + t of the row -- one doubling
//                 per bit plane, one mixed addition of +-P_{k+i} per set bit, the sign folded into the
//                 y of the affine operand -- and the verdict D_k != O as one byte.  The plan is a
//                 kernel argument, the same for every lane, so which entries a bit plane adds is
//                 wave-uniform: lanes part only at the exceptional branches of the additions, which
//                 are the complete ones of ec28.h (at t = 1 every honest window cancels exactly, equal
//                 neighbours double, keys at infinity are the identity).  A lane whose row holds a key
//                 with a non-zero status writes nothing.
//   k_lock_fold   1 lane / row: HBLS_BAD_PUBKEY for a row with such a key (row_windows left as it is),
//                 else the row's W verdict bytes as the mask row_windows and HBLS_OK / HBLS_NOT_VERIFIED.
// Plain vector stores only.  Compiled like cluster.hip and vbatch.hip (HB_FAST_FPMUL).
#define HB_FAST_FPMUL 1
#include "lines.h"
#include "rlc.h"

#include "lockcheck.h"

// two waves per SIMD, as the other G1 ladders (HB_OCC_SUBG): 256 registers a lane
#define HB_OCC_LOCK 2

namespace hb {

// the row's first key with a non-zero status decides: nothing is computed for such a row
__device__ __forceinline__ bool lock_row_bad(const uint8_t* __restrict__ st, uint32_t row_keys) {
  uint32_t bad = 0;
  for (uint32_t j = 0; j < row_keys; j++) bad |= st[j];
  return bad != 0;
}

__global__ KB_OCC(HB_OCC_LOCK) void k_lock_check(const G1AEntry* __restrict__ ent, const uint8_t* __restrict__ st,
                                                 uint32_t n_rows, LockPlan plan, uint8_t* __restrict__ verdict) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= (uint64_t)n_rows * plan.windows) return;
  const uint32_t row_keys = 1 + plan.n_shares;
  const uint64_t row = lane / plan.windows;
  const uint32_t k = (uint32_t)(lane % plan.windows);  // k + t <= n_shares: every entry read is the row's own
  if (lock_row_bad(st + row * row_keys, row_keys)) return;
  const G1AEntry* __restrict__ win = ent + row * row_keys + k;
  G1L R = g1l_infinity();
  HB_NOUNROLL for (int b = (int)plan.bits - 1; b >= 0; b--) {
    R = g1l_dbl(R);
    HB_NOUNROLL for (uint32_t i = 0; i <= plan.t; i++) {
      const int64_t c = plan.c[i];
      const uint64_t mag = (uint64_t)(c < 0 ? -c : c);
      if (!((mag >> b) & 1)) continue;  // wave-uniform
      if (win[i].inf) continue;         // the identity
      const Fp y = win[i].y;
      R = g1l_madd(R, l_from(win[i].x), l_from(c < 0 ? fp_neg(y) : y));
    }
  }
  verdict[lane] = (R.inf || l_is_zero(R.Z)) ? 0 : 1;
#endif
}

__global__ __launch_bounds__(64) void k_lock_fold(const uint8_t* __restrict__ st, uint32_t n_rows, uint32_t n_shares,
                                                  uint32_t windows, const uint8_t* __restrict__ verdict,
                                                  uint8_t* __restrict__ row_status, uint64_t* __restrict__ row_windows) {
  const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_rows) return;
  if (lock_row_bad(st + row * (1 + n_shares), 1 + n_shares)) {
    row_status[row] = (uint8_t)ST_BAD_PUBKEY;
    return;
  }
  uint64_t mask = 0;
  for (uint32_t k = 0; k < windows; k++) mask |= (uint64_t)(verdict[row * windows + k] != 0) << k;
  row_status[row] = mask ? (uint8_t)ST_NOT_VERIFIED : (uint8_t)ST_OK;
  row_windows[row] = mask;
}

void launch_lock_check(const G1AEntry* ent, const uint8_t* st, uint32_t n_rows, const LockPlan& plan, uint8_t* verdict,
                       uint8_t* row_status, uint64_t* row_windows, hipStream_t s) {
  if (!n_rows) return;
  const uint64_t lanes = (uint64_t)n_rows * plan.windows;
  hipLaunchKernelGGL(k_lock_check, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, s, ent, st, n_rows, plan, verdict);
  hipLaunchKernelGGL(k_lock_fold, dim3((n_rows + 63) / 64), dim3(64), 0, s, st, n_rows, plan.n_shares, plan.windows, verdict,
                     row_status, row_windows);
}

}  // namespace hb
