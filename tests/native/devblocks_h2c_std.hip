// TEST-ONLY device block harness, hash-to-curve in the standard convention: no HB_FAST_FPMUL, the
// building blocks separate functions, as charon_amd/csrc/hash.hip is compiled (k_hash_to_g2,
// k_hash_to_g2_1).  One lane per case around hash_to_field_fp2, sswu_map + iso3_map,
// g2_clear_cofactor (of Q0 + Q1), g2_psi, g2_psi2 and hash_to_g2, so tests/test_gpu_hash.py can
// compare them with the oracle on chosen inputs.  A unit of the hash harness (devblocks_h2c.hip,
// build.py DEVBLOCKS_HASH).  The product library never loads this.
#define DB_STD_CONVENTION 1
#include "devblocks.h"

#if defined(HB_FAST_FPMUL)
#error "the standard-convention unit must not see HB_FAST_FPMUL"
#endif

using namespace hb;

enum { DB_H2C_MAX = 256 };

// ---- points.  Case i: 144 input words (S_MAP: u, 24 words; S_CLEAR: the Jacobian Q0, Q1; S_PSI,
// S_PSI2: one Jacobian point); out: one Jacobian point, 72 words
enum { S_MAP, S_CLEAR, S_PSI, S_PSI2, S_OPS };

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ Fp2 hs_ld2(const uint32_t* p) {
  Fp2 r;
  HB_UNROLL for (int i = 0; i < NL; i++) {
    r.c0.v[i] = p[i];
    r.c1.v[i] = p[12 + i];
  }
  return r;
}
__device__ __forceinline__ void hs_st2(uint32_t* p, const Fp2& a) {
  HB_UNROLL for (int i = 0; i < NL; i++) {
    p[i] = a.c0.v[i];
    p[12 + i] = a.c1.v[i];
  }
}
__device__ __forceinline__ G2J hs_ldj(const uint32_t* p) { return {hs_ld2(p), hs_ld2(p + 24), hs_ld2(p + 48)}; }
#endif

template <int OP>
__global__ KB_OCC(HB_OCC_HASH) void k_h2c_std(const uint32_t* __restrict__ in, int n, uint32_t* __restrict__ out) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int i = t < n ? t : n - 1;  // lanes past the last case shadow it and store nothing
  const uint32_t* p = in + 144 * (size_t)i;
  G2J r;
  if constexpr (OP == S_MAP) {
    Fp2 x, y;
    sswu_map(x, y, hs_ld2(p));
    r = iso3_map(x, y);
  }
  if constexpr (OP == S_CLEAR) r = g2_clear_cofactor(jac_add(hs_ldj(p), hs_ldj(p + 72)));
  if constexpr (OP == S_PSI) r = g2_psi(hs_ldj(p));
  if constexpr (OP == S_PSI2) r = g2_psi2(hs_ldj(p));
  if (t < n) {
    uint32_t* o = out + 72 * (size_t)t;
    hs_st2(o, r.X);
    hs_st2(o + 24, r.Y);
    hs_st2(o + 48, r.Z);
  }
#endif
}

template <int OP>
static int h2c_std_run(int n, const uint32_t* in, uint32_t* out) {
  DbDev dev;
  uint32_t *din, *dout;
  DB_MAKE(dev, din, in, (size_t)n * 144 * 4);
  DB_MAKE(dev, dout, nullptr, (size_t)n * 72 * 4);
  hipLaunchKernelGGL(k_h2c_std<OP>, dim3((n + 63) / 64), dim3(64), 0, 0, (const uint32_t*)din, n, dout);
  if (const int rc = db_finish()) return rc;
  return db_fetch(out, dout, (size_t)n * 72 * 4);
}

extern "C" int db_h2c_std(int op, int n, const uint32_t* in, uint32_t* out) {
  if (n < 1 || n > DB_H2C_MAX || !in || !out) return DB_E_ARG;
  switch (op) {
    case S_MAP: return h2c_std_run<S_MAP>(n, in, out);
    case S_CLEAR: return h2c_std_run<S_CLEAR>(n, in, out);
    case S_PSI: return h2c_std_run<S_PSI>(n, in, out);
    case S_PSI2: return h2c_std_run<S_PSI2>(n, in, out);
  }
  return DB_E_OP;
}

// ---- messages.  M_FIELD: out = (u0, u1), 48 words; M_HASH: out = hash_to_g2's Jacobian point, 72
// words; 72 words per message either way
enum { M_FIELD, M_HASH, M_OPS };

template <int OP>
__global__ KB_OCC(HB_OCC_HASH) void k_h2c_std_msg(const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ off,
                                                 const uint32_t* __restrict__ len, int n, uint32_t* __restrict__ out) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (t >= n) return;  // as k_hash_to_g2_1
  uint32_t* o = out + 72 * (size_t)t;
  if constexpr (OP == M_FIELD) {
    Fp2 u0, u1;
    hash_to_field_fp2(u0, u1, msgs + off[t], len[t]);
    hs_st2(o, u0);
    hs_st2(o + 24, u1);
  } else {
    const G2J r = hash_to_g2(msgs + off[t], len[t]);
    hs_st2(o, r.X);
    hs_st2(o + 24, r.Y);
    hs_st2(o + 48, r.Z);
  }
#endif
}

extern "C" int db_h2c_std_msg(int op, int n, const uint8_t* msgs, size_t msgs_bytes, const uint64_t* off,
                              const uint32_t* len, uint32_t* out) {
  if (n < 1 || n > DB_H2C_MAX || !msgs || !off || !len || !out || !db_ranges_ok(n, msgs_bytes, off, len)) return DB_E_ARG;
  if (op != M_FIELD && op != M_HASH) return DB_E_OP;
  DbDev dev;
  uint8_t* dmsgs;
  uint64_t* doff;
  uint32_t *dlen, *dout;
  DB_MAKE(dev, dmsgs, msgs, msgs_bytes);
  DB_MAKE(dev, doff, off, (size_t)n * 8);
  DB_MAKE(dev, dlen, len, (size_t)n * 4);
  DB_MAKE(dev, dout, nullptr, (size_t)n * 72 * 4);
  const dim3 grid((n + 63) / 64), block(64);
  if (op == M_FIELD)
    hipLaunchKernelGGL(k_h2c_std_msg<M_FIELD>, grid, block, 0, 0, (const uint8_t*)dmsgs, (const uint64_t*)doff,
                       (const uint32_t*)dlen, n, dout);
  else
    hipLaunchKernelGGL(k_h2c_std_msg<M_HASH>, grid, block, 0, 0, (const uint8_t*)dmsgs, (const uint64_t*)doff,
                       (const uint32_t*)dlen, n, dout);
  if (const int rc = db_finish()) return rc;
  return db_fetch(out, dout, (size_t)n * 72 * 4);
}
