// msm.hip: the signature side of a whole verification as ONE multi-scalar multiplication
// (bucket method), for the batched check of vbatch.hip / vgroup.hip.
//
// With random r_i = a_i + b_i lambda (rlc.h) the check over every READY group g of a call is
//     prod_g e(P_g, H(m_g)) * e(-g1, S) == 1,   S = sum_i [r_i] sig_i = sum_i [a_i] sig_i + [b_i] (-psi^2 sig_i),
// so the signature side needs no per-group sums: S is one MSM of 2 (n + n_agg) affine points with
// 32-bit scalars.  Bucket method with c = 16-bit windows (two windows): every (point, window) pair
// with a nonzero digit d is one entry of bucket (window, d); the entries are sorted by bucket with
// a counting sort (histogram, scan, scatter); one lane sums a bucket with mixed additions; buckets
// are weighed by running sums over chunks of 16 (plus one 16-bit multiple per chunk) and the chunk
// results summed by wave butterflies.  Per entry that is ONE mixed G2 addition (~29 Fp products)
// where the per-group ladders spent ~1 400 Fp products per item.
//
// Only items whose group is READY (group_scan, vgroup.hip) with a nonzero coefficient enter the
// sum.  If the slot-wide check fails, the per-group path runs (hipbls.hip verify_pipeline), so
// verdicts are those of the per-group check.
//
// The same counting sort and bucket sums serve the batched G2 subgroup test of large calls
// (k_subg_*, below; subgbatch.h): five buckets per signature keyed by base-13 digit vectors, and 20
// weighted bucket sums tested for psi(S) = [x] S in place of one 63-doubling ladder per signature.
#define HB_FAST_FPMUL 1
#include "lines.h"
#include "pair3.h"

namespace hb {

constexpr int BLOCK = 64;

// The reduction and the butterflies run 128 and at most 64 waves: far fewer than the SIMDs, so
// they are latency-bound and take one wave per SIMD's full register file (no scratch spills).
#define HB_OCC_MSMBUCKET HB_OCC_RLC
#define HB_OCC_MSMTAIL 1

__device__ __forceinline__ bool msm_take(const G2MsmArgs& a, uint32_t i, uint2& ab) {
  ab = a.coef[i];
  if ((ab.x | ab.y) == 0) return false;
  // coefficients are drawn from the keys alone (the combination runs beside the signatures'
  // subgroup checks and the aggregation): an item enters as group_scan takes it -- signature
  // status OK, not at infinity
  if (i < a.n) return a.gst[a.igrp[i]] == G_READY && !a.sig_st[i] && !a.sig[i].inf;
  const uint32_t g = i - a.n;
  return a.gst[g] == G_READY && !a.agg_st[g] && !a.agg_sig[g].inf;
}

// The counting sort and the bucket sums, shared by the slot-wide MSM and the batched subgroup test
// (k_subg_*).  A source S names the sort's arrays (cnt, off, cur, ent, order, bucket), its number
// of buckets KEYS and of items, each item's entries -- each_entry(i, f) calls f(bucket, entry) --
// and the affine point an entry stands for (point(entry)).
struct MsmSlotSrc {
  const G2MsmArgs& a;
  static constexpr uint32_t KEYS = MSM_KEYS;
  uint32_t *cnt, *off, *cur, *ent, *order;
  G2JEntry* bucket;
  __device__ __forceinline__ MsmSlotSrc(const G2MsmArgs& a_)
      : a(a_), cnt(a_.cnt), off(a_.off), cur(a_.cur), ent(a_.ent), order(a_.order), bucket(a_.bucket) {}
  __device__ __forceinline__ uint32_t items() const { return a.n + a.n_agg; }
  // entries (item << 1 | half), one per nonzero 16-bit digit of the item's two coefficients
  template <class F>
  __device__ __forceinline__ void each_entry(uint32_t i, F f) const {
    uint2 ab;
    if (!msm_take(a, i, ab)) return;
    HB_UNROLL for (int h = 0; h < 2; h++) {
      const uint32_t s = h ? ab.y : ab.x;
      HB_UNROLL for (int w = 0; w < MSM_WINDOWS; w++) {
        const uint32_t d = (s >> (MSM_C * w)) & MSM_MASK;
        if (d) f(((uint32_t)w << MSM_C) + d, (i << 1) | (uint32_t)h);
      }
    }
  }
  // half 1: -psi^2 of the signature
  __device__ __forceinline__ G2A point(uint32_t u) const {
    const uint32_t i = u >> 1;
    const HmEntry se = i < a.n ? a.sig[i] : a.agg_sig[i - a.n];
    G2A P = {se.x, se.y, false};
    if (u & 1u) P = {f2_mul_fp(P.x, fp_from_const(PSI2_CX[0])), f2_neg(f2_mul_fp(P.y, fp_from_const(PSI2_CY[0]))), false};
    return P;
  }
};

// the batched subgroup test: bucket (window, value) of k_subg_digits' window values, entry = item
struct SubgSrc {
  const SubgArgs& a;
  static constexpr uint32_t KEYS = SG_KEYS;
  uint32_t *cnt, *off, *cur, *ent, *order;
  G2JEntry* bucket;
  __device__ __forceinline__ SubgSrc(const SubgArgs& a_)
      : a(a_), cnt(a_.cnt), off(a_.off), cur(a_.cur), ent(a_.ent), order(a_.order), bucket(a_.bucket) {}
  __device__ __forceinline__ uint32_t items() const { return a.n; }
  template <class F>
  __device__ __forceinline__ void each_entry(uint32_t i, F f) const {
    HB_UNROLL for (uint32_t w = 0; w < SG_WINDOWS; w++) {
      const uint32_t d = a.dig[(size_t)SG_WINDOWS * i + w];
      if (d) f(w * SG_RANGE + d, i);
    }
  }
  __device__ __forceinline__ G2A point(uint32_t u) const {
    const HmEntry se = a.sig[u];
    return {se.x, se.y, false};
  }
};

// one lane per item: bucket sizes
template <class S>
__device__ __forceinline__ void msm_count(const S& src) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= src.items()) return;
  src.each_entry(i, [&](uint32_t k, uint32_t) { atomicAdd(src.cnt + k, 1u); });
}

// one lane per item: entries into their buckets' ranges
template <class S>
__device__ __forceinline__ void msm_fill(const S& src) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= src.items()) return;
  src.each_entry(i, [&](uint32_t k, uint32_t u) { src.ent[src.off[k] + atomicAdd(src.cur + k, 1u)] = u; });
}

// one workgroup: the buckets in decreasing order of size (counting sort on the sizes, capped at
// 255), so that the lanes of a wave of the bucket sums take buckets of nearly equal size (lane per
// bucket in key order: Poisson sizes, a wave waits for its largest)
template <uint32_t KEYS>
__device__ __forceinline__ void msm_order(const uint32_t* __restrict__ cnt, uint32_t* __restrict__ order) {
  __shared__ uint32_t hist[256];
  const uint32_t t = threadIdx.x;
  if (t < 256) hist[t] = 0;
  __syncthreads();
  for (uint32_t k = t; k < KEYS; k += 1024) atomicAdd(&hist[255u - min(cnt[k], 255u)], 1u);
  __syncthreads();
  if (t == 0) {  // exclusive scan, largest sizes first
    uint32_t run = 0;
    for (int b = 0; b < 256; b++) {
      const uint32_t c = hist[b];
      hist[b] = run;
      run += c;
    }
  }
  __syncthreads();
  for (uint32_t k = t; k < KEYS; k += 1024) order[atomicAdd(&hist[255u - min(cnt[k], 255u)], 1u)] = k;
}

// one lane per bucket (in the order of msm_order): the sum of its points, in lazily reduced 28-bit
// limbs (ec28.h g2l_madd: equal points double, opposite ones give infinity)
template <class S>
__device__ __forceinline__ void msm_bucket(const S& src) {
  const uint32_t L = blockIdx.x * blockDim.x + threadIdx.x;
  if (L >= S::KEYS) return;
  const uint32_t k = src.order[L];
  const uint32_t b = src.off[k], e = src.off[k + 1];
  G2L acc = g2l_infinity();
  HB_NOUNROLL for (uint32_t j = b; j < e; j++) {
    const G2A P = src.point(src.ent[j]);
    acc = g2l_madd(acc, f2l_from(P.x), f2l_from(P.y));
  }
  const G2J r = g2l_to_jac(acc);
  src.bucket[k] = {r.X, r.Y, r.Z};
}

__global__ __launch_bounds__(64) void k_msm_count(G2MsmArgs a) { msm_count(MsmSlotSrc(a)); }
__global__ __launch_bounds__(64) void k_msm_fill(G2MsmArgs a) { msm_fill(MsmSlotSrc(a)); }
__global__ __launch_bounds__(1024) void k_msm_order(const uint32_t* __restrict__ cnt, uint32_t* __restrict__ order) {
  msm_order<MSM_KEYS>(cnt, order);
}
__global__ KB_OCC(HB_OCC_MSMBUCKET) void k_msm_bucket(G2MsmArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
  msm_bucket(MsmSlotSrc(a));
#endif
}

// [m] p for a 16-bit m (uniform control flow: every step's addition computed, kept per lane)
__device__ __forceinline__ G2J mul16(const G2J& p, uint32_t m) {
  G2J r = jac_infinity<Fp2>();
  HB_NOUNROLL for (int bit = 15; bit >= 0; bit--) {
    r = jac_dbl(r);
    const G2J t = jac_add(r, p);
    const bool take = ((m >> bit) & 1u) != 0;
    r = {take ? t.X : r.X, take ? t.Y : r.Y, take ? t.Z : r.Z};
  }
  return r;
}

// one lane per chunk of MSM_CHUNK buckets of one window: sum_d d * 2^(16 w) B_d over the chunk,
// as running sums T = sum_j (j + 1) B_(lo + j), R = sum_j B_(lo + j), then T + (lo - 1) R
__global__ KB_OCC(HB_OCC_MSMTAIL) void k_msm_reduce(G2MsmArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= MSM_PARTS) return;
  constexpr uint32_t per_w = (1u << MSM_C) / MSM_CHUNK;
  const uint32_t w = c / per_w, lo = (c % per_w) * MSM_CHUNK;
  const G2JEntry* B = a.bucket + ((size_t)w << MSM_C) + lo;
  G2J R = jac_infinity<Fp2>(), T = jac_infinity<Fp2>();
  HB_NOUNROLL for (int j = (int)MSM_CHUNK - 1; j >= 0; j--) {
    const G2JEntry q = B[j];
    R = jac_add(R, G2J{q.X, q.Y, q.Z});
    T = jac_add(T, R);
  }
  G2J W;
  if (lo == 0) W = jac_add(T, jac_neg(R));  // (lo - 1) = -1
  else W = jac_add(T, mul16(R, lo - 1));
  HB_NOUNROLL for (uint32_t k = 0; k < MSM_C * w; k++) W = jac_dbl(W);  // wave-uniform
  a.part[c] = {W.X, W.Y, W.Z};
#endif
}

// sum of m Jacobian points: workgroup b (one wave) sums in[b * 64 q, (b + 1) * 64 q) into out[b]
__global__ KB_OCC(HB_OCC_MSMTAIL) void k_msm_sum(const G2JEntry* __restrict__ in, uint32_t m, uint32_t q,
                                             G2JEntry* __restrict__ out) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t lane = threadIdx.x & 63u, base = blockIdx.x * 64u * q;
  G2J S = jac_infinity<Fp2>();
  HB_NOUNROLL for (uint32_t j = 0; j < q; j++) {
    const uint32_t i = base + j * 64u + lane;
    if (i < m) {
      const G2JEntry e = in[i];
      S = jac_add(S, G2J{e.X, e.Y, e.Z});
    }
  }
  HB_NOUNROLL for (int off = 32; off; off >>= 1) {
    const int addr = (int)((lane ^ (uint32_t)off) << 2);
    const G2J T = {xch(S.X, addr), xch(S.Y, addr), xch(S.Z, addr)};
    S = jac_add(S, T);
  }
  if (lane == 0) out[blockIdx.x] = {S.X, S.Y, S.Z};
#endif
}

// ---- the batched G2 subgroup test (subgbatch.h) ----

// one lane per signature: its window values; an item enters only if it decoded and is not the
// infinity encoding -- the items k_g2_subgroup would ladder
__global__ __launch_bounds__(64) void k_subg_digits(SubgArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  uint32_t d[SG_WINDOWS];
  sg_windows(a.key.w, i, d);
  const bool take = !a.sig_st[i] && !a.sig[i].inf;
  HB_UNROLL for (uint32_t w = 0; w < SG_WINDOWS; w++) a.dig[(size_t)SG_WINDOWS * i + w] = take ? d[w] : 0u;
}
__global__ __launch_bounds__(64) void k_subg_count(SubgArgs a) { msm_count(SubgSrc(a)); }
__global__ __launch_bounds__(64) void k_subg_fill(SubgArgs a) { msm_fill(SubgSrc(a)); }
__global__ __launch_bounds__(1024) void k_subg_order(const uint32_t* __restrict__ cnt, uint32_t* __restrict__ order) {
  msm_order<SG_KEYS>(cnt, order);
}
__global__ KB_OCC(HB_OCC_MSMBUCKET) void k_subg_bucket(SubgArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
  msm_bucket(SubgSrc(a));
#endif
}

// one wave per class (w, j, c), c = 1..12: the sum of the SG_CLASS_SIZE buckets of window w whose
// digit j is c.  Lane l takes the members l, l + 64, ... (35 at most), then a butterfly as k_msm_sum.
__global__ KB_OCC(HB_OCC_MSMTAIL) void k_subg_class(const G2JEntry* __restrict__ bucket, G2JEntry* __restrict__ cls) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t lane = threadIdx.x & 63u, q = blockIdx.x;
  const uint32_t c = q % (SG_BASE - 1) + 1, wj = q / (SG_BASE - 1), j = wj % SG_DIGITS, w = wj / SG_DIGITS;
  const G2JEntry* B = bucket + (size_t)w * SG_RANGE;
  G2J S = jac_infinity<Fp2>();
  HB_NOUNROLL for (uint32_t m = lane; m < SG_CLASS_SIZE; m += 64u) {
    const G2JEntry e = B[sg_class_member(j, c, m)];
    S = jac_add(S, G2J{e.X, e.Y, e.Z});
  }
  HB_NOUNROLL for (int off = 32; off; off >>= 1) {
    const int addr = (int)((lane ^ (uint32_t)off) << 2);
    const G2J T = {xch(S.X, addr), xch(S.Y, addr), xch(S.Z, addr)};
    S = jac_add(S, T);
  }
  if (lane == 0) cls[q] = {S.X, S.Y, S.Z};
#endif
}

// one lane per (w, j): S_(w,j) = sum_c c C_c as running sums from c = 12 down
__global__ KB_OCC(HB_OCC_MSMTAIL) void k_subg_weigh(const G2JEntry* __restrict__ cls, G2JEntry* __restrict__ sums) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= SG_SUMS) return;
  const G2JEntry* C = cls + (size_t)t * (SG_BASE - 1);
  G2J R = jac_infinity<Fp2>(), T = jac_infinity<Fp2>();
  HB_NOUNROLL for (int c = (int)SG_BASE - 2; c >= 0; c--) {
    const G2JEntry q = C[c];
    R = jac_add(R, G2J{q.X, q.Y, q.Z});
    T = jac_add(T, R);
  }
  sums[t] = {T.X, T.Y, T.Z};
#endif
}

// one lane per sum: S in G2 (infinity passes), else the flag rec[0] that k_g2_subgroup runs behind
__global__ KB_OCC(HB_OCC_MSMTAIL) void k_subg_verdict(const G2JEntry* __restrict__ sums, uint32_t* __restrict__ rec,
                                                       SubgCtr* __restrict__ ctr) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= SG_SUMS) return;
  if (t == 0) atomicAdd(&ctr->run, 1ull);
  const G2JEntry e = sums[t];
  const G2A q = jac_to_aff(G2J{e.X, e.Y, e.Z});
  if (!g2_in_subgroup28(q) && atomicExch(rec, 1u) == 0u) atomicAdd(&ctr->failed, 1ull);
#endif
}

__global__ void k_subg_skipped(SubgCtr* ctr) { atomicAdd(&ctr->skipped, 1ull); }

static inline unsigned blocks_for(size_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

void launch_subg_digits(const SubgArgs& a, hipStream_t s) {
  if (a.n) hipLaunchKernelGGL(k_subg_digits, dim3(blocks_for(a.n)), dim3(BLOCK), 0, s, a);
}
void launch_subg_count(const SubgArgs& a, hipStream_t s) {
  if (a.n) hipLaunchKernelGGL(k_subg_count, dim3(blocks_for(a.n)), dim3(BLOCK), 0, s, a);
}
void launch_subg_fill(const SubgArgs& a, hipStream_t s) {
  if (a.n) hipLaunchKernelGGL(k_subg_fill, dim3(blocks_for(a.n)), dim3(BLOCK), 0, s, a);
}
void launch_subg_bucket(const SubgArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_subg_order, dim3(1), dim3(1024), 0, s, (const uint32_t*)a.cnt, a.order);
  hipLaunchKernelGGL(k_subg_bucket, dim3(blocks_for(SG_KEYS)), dim3(BLOCK), 0, s, a);
}
void launch_subg_class(const G2JEntry* bucket, G2JEntry* cls, hipStream_t s) {
  hipLaunchKernelGGL(k_subg_class, dim3(SG_CLASSES), dim3(BLOCK), 0, s, bucket, cls);
}
void launch_subg_weigh(const G2JEntry* cls, G2JEntry* sums, hipStream_t s) {
  hipLaunchKernelGGL(k_subg_weigh, dim3(1), dim3(BLOCK), 0, s, cls, sums);
}
void launch_subg_verdict(const G2JEntry* sums, uint32_t* rec, SubgCtr* ctr, hipStream_t s) {
  hipLaunchKernelGGL(k_subg_verdict, dim3(1), dim3(BLOCK), 0, s, sums, rec, ctr);
}
void launch_subg_skipped(SubgCtr* ctr, hipStream_t s) { hipLaunchKernelGGL(k_subg_skipped, dim3(1), dim3(1), 0, s, ctr); }

void launch_msm_count(const G2MsmArgs& a, hipStream_t s) {
  const size_t n = (size_t)a.n + a.n_agg;
  if (n) hipLaunchKernelGGL(k_msm_count, dim3(blocks_for(n)), dim3(BLOCK), 0, s, a);
}
void launch_msm_fill(const G2MsmArgs& a, hipStream_t s) {
  const size_t n = (size_t)a.n + a.n_agg;
  if (n) hipLaunchKernelGGL(k_msm_fill, dim3(blocks_for(n)), dim3(BLOCK), 0, s, a);
}
void launch_msm_bucket(const G2MsmArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_msm_order, dim3(1), dim3(1024), 0, s, (const uint32_t*)a.cnt, a.order);
  hipLaunchKernelGGL(k_msm_bucket, dim3(blocks_for(MSM_KEYS)), dim3(BLOCK), 0, s, a);
}
void launch_msm_reduce(const G2MsmArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_msm_reduce, dim3(blocks_for(MSM_PARTS)), dim3(BLOCK), 0, s, a);
}
// part[MSM_PARTS] -> part2[n2 <= 64] -> total[0]: q entries per lane in the first pass
void launch_msm_sum(const G2MsmArgs& a, hipStream_t s) {
  constexpr uint32_t q = MSM_PARTS >= 64 * 64 ? MSM_PARTS / (64 * 64) : 1u, n2 = MSM_PARTS / (64 * q);
  static_assert(MSM_PARTS % (64 * q) == 0 && n2 <= 64 && n2 <= MSM_PARTS / 128, "two butterfly passes");
  hipLaunchKernelGGL(k_msm_sum, dim3(n2), dim3(BLOCK), 0, s, (const G2JEntry*)a.part, MSM_PARTS, q, a.part2);
  hipLaunchKernelGGL(k_msm_sum, dim3(1), dim3(BLOCK), 0, s, (const G2JEntry*)a.part2, n2, 1u, a.total);
}

}  // namespace hb
