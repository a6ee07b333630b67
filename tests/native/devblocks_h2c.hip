// TEST-ONLY device block harness, hash-to-curve in the fast convention (HB_FAST_FPMUL, as
// hashsplit.hip is compiled).  With devblocks_h2c_std.hip it is a harness of its own (build.py
// DEVBLOCKS_HASH: its own library and id), so tests/test_gpu_hash.py can run every stage of
// hash_to_curve G2 on chosen inputs and compare it with the oracle.  The product library never
// loads this.
//
// build.py compiles the file once per part:
//   -DDB_H2C=1  the stages: this part compiles the product's charon_amd/csrc/hashsplit.hip itself and
//               launches its own kernels (k_h2c_field, k_h2c_map, k_h2c_clear1 / 1h, k_h2c_clear1b,
//               k_h2c_clear2 / 2h, k_h2c_clear3) on an explicit MsgEntry array, from a first to a
//               last stage, the host writing u0, u1 or Q0, Q1 into the hand-over slots where
//               h2c_u / h2c_q put them (their offsets are asked of the device functions themselves).
//   -DDB_H2C=2  the leaves: one lane per case around fp_pow_win (the four constant schedules),
//               fp_sqrt, fp_is_square, f2_sqrt, f2_sgn0, f2_is_lex_largest, fp_from_mont,
//               fp_from_be512, xmd_bi, sswu_iso_map and xmd_b0.
// Launches are at most DB_H2C_MAX cases; every message range is checked on the host against the
// uploaded buffer before a kernel may read it.
#if !defined(DB_H2C)
#error "compile with -DDB_H2C=1 or 2"
#endif

#if DB_H2C == 1
#include "../../charon_amd/csrc/hashsplit.hip"
#endif

#include "devblocks.h"

#include <cstddef>
#include <cstring>
#include <vector>

using namespace hb;

enum { DB_H2C_MAX = 256 };

#if DB_H2C == 1
extern "C" const char* db_build_id() { return DB_BUILD_ID; }
extern "C" int db_h2c_max() { return DB_H2C_MAX; }

// stages of db_h2c_stages, in launch order
enum { ST_FIELD, ST_MAP, ST_CLEAR1, ST_CLEAR1B, ST_CLEAR2, ST_CLEAR3, ST_N };

// byte offsets of the hand-over slots inside a MsgEntry, from the product's own accessors
__global__ void k_h2c_slots(MsgEntry* hm, uint32_t* o) {
#if defined(__HIP_DEVICE_COMPILE__)
  o[0] = (uint32_t)(reinterpret_cast<char*>(h2c_u(hm)) - reinterpret_cast<char*>(hm));
  o[1] = (uint32_t)(reinterpret_cast<char*>(h2c_q(hm)) - reinterpret_cast<char*>(hm));
#endif
}

// Runs stages first .. last over n messages.  Input: first == ST_FIELD the messages (msgs, off, len);
// first == ST_MAP `in` = n x (u0, u1), 48 words each; first == ST_CLEAR1 `in` = n x (Q0, Q1), 144
// words each; a later first stage is refused.  pair != 0: the lane-pair ladders (k_h2c_clear1h /
// 2h).  Output, whatever the last stage: per message u (48 words: h2c_u's slot), q (216 words:
// h2c_q's three Jacobian records) and h (52 words: the HmEntry).
extern "C" int db_h2c_stages(int first, int last, int pair, int n, const uint8_t* msgs, size_t msgs_bytes,
                             const uint64_t* off, const uint32_t* len, const uint32_t* in, uint32_t* out_u,
                             uint32_t* out_q, uint32_t* out_h) {
  static_assert(sizeof(HmEntry) == 52 * 4 && sizeof(G2JEntry) == 72 * 4 && sizeof(Fp2) == 24 * 4,
                "raw-word layouts of layout.h");
  if (n < 1 || n > DB_H2C_MAX || first < ST_FIELD || first > ST_CLEAR1 || last < first || last >= ST_N || !out_u ||
      !out_q || !out_h)
    return DB_E_ARG;
  if (first == ST_FIELD) {
    if (!msgs || !off || !len || !db_ranges_ok(n, msgs_bytes, off, len)) return DB_E_ARG;
  } else if (!in) {
    return DB_E_ARG;
  }
  DbDev dev;
  MsgEntry* dhm;
  uint32_t* dslots;
  uint8_t* dmsgs = nullptr;
  uint64_t* doff = nullptr;
  uint32_t* dlen = nullptr;
  DB_MAKE(dev, dhm, nullptr, (size_t)n * sizeof(MsgEntry));
  DB_MAKE(dev, dslots, nullptr, 8);
  hipLaunchKernelGGL(k_h2c_slots, dim3(1), dim3(1), 0, 0, dhm, dslots);
  if (const int rc = db_finish()) return rc;
  uint32_t slot[2];
  if (const int rc = db_fetch(slot, dslots, 8)) return rc;
  if (slot[0] + 2 * sizeof(Fp2) > sizeof(MsgEntry) || slot[1] + 3 * sizeof(G2JEntry) > sizeof(MsgEntry)) return DB_E_ARG;
  if (first == ST_FIELD) {
    DB_MAKE(dev, dmsgs, msgs, msgs_bytes);
    DB_MAKE(dev, doff, off, (size_t)n * 8);
    DB_MAKE(dev, dlen, len, (size_t)n * 4);
  } else {
    const size_t at = first == ST_MAP ? slot[0] : slot[1], bytes = first == ST_MAP ? 2 * sizeof(Fp2) : 2 * sizeof(G2JEntry);
    for (int i = 0; i < n; i++)
      if (hipMemcpy(reinterpret_cast<char*>(dhm + i) + at, reinterpret_cast<const char*>(in) + (size_t)i * bytes, bytes,
                    hipMemcpyHostToDevice) != hipSuccess)
        return DB_E_UPLOAD;
  }
  const unsigned g1 = (unsigned)((n + HBLOCK - 1) / HBLOCK), g2 = (unsigned)((2 * n + HBLOCK - 1) / HBLOCK);
  const uint32_t un = (uint32_t)n;
  for (int st = first; st <= last; st++) {  // the launches of launch_hash_to_g2_split, one checked at a time
    switch (st) {
      case ST_FIELD:
        hipLaunchKernelGGL(k_h2c_field, dim3(g1), dim3(HBLOCK), 0, 0, (const uint8_t*)dmsgs, (const uint64_t*)doff,
                           (const uint32_t*)dlen, un, dhm);
        break;
      case ST_MAP: hipLaunchKernelGGL(k_h2c_map, dim3(g2), dim3(HBLOCK), 0, 0, un, dhm); break;
      case ST_CLEAR1:
        if (pair)
          hipLaunchKernelGGL(k_h2c_clear1h, dim3(g2), dim3(HBLOCK), 0, 0, un, dhm);
        else
          hipLaunchKernelGGL(k_h2c_clear1, dim3(g1), dim3(HBLOCK), 0, 0, un, dhm);
        break;
      case ST_CLEAR1B: hipLaunchKernelGGL(k_h2c_clear1b, dim3(g1), dim3(HBLOCK), 0, 0, un, dhm); break;
      case ST_CLEAR2:
        if (pair)
          hipLaunchKernelGGL(k_h2c_clear2h, dim3(g2), dim3(HBLOCK), 0, 0, un, dhm);
        else
          hipLaunchKernelGGL(k_h2c_clear2, dim3(g1), dim3(HBLOCK), 0, 0, un, dhm);
        break;
      case ST_CLEAR3: hipLaunchKernelGGL(k_h2c_clear3, dim3(g1), dim3(HBLOCK), 0, 0, un, dhm); break;
    }
    if (const int rc = db_finish()) return rc;
  }
  for (int i = 0; i < n; i++) {
    const char* e = reinterpret_cast<const char*>(dhm + i);
    if (const int rc = db_fetch(out_u + 48 * (size_t)i, e + slot[0], 2 * sizeof(Fp2))) return rc;
    if (const int rc = db_fetch(out_q + 216 * (size_t)i, e + slot[1], 3 * sizeof(G2JEntry))) return rc;
    if (const int rc = db_fetch(out_h + 52 * (size_t)i, e + offsetof(MsgEntry, h), sizeof(HmEntry))) return rc;
  }
  return 0;
}
#endif  // DB_H2C == 1

#if DB_H2C == 2
// ---- leaves.  Case i: 24 input words (an Fp2 a = (a.c0, a.c1); the Fp operations take a.c0;
// L_FROM_BE512 takes 16 big-endian words W; L_XMD_BI takes x (8 words) and i in word 8); out: 72
// words (r.c0, r.c1 first; L_XMD_BI 8 words; L_SSWU_ISO the Jacobian X, Y, Z); flag[i] the verdict.
enum {
  L_POW_P_MINUS_2, L_POW_SQRT, L_POW_P_M3_4, L_POW_LEGENDRE, L_FP_SQRT, L_FP_IS_SQUARE, L_F2_SQRT, L_F2_SGN0,
  L_F2_LEX, L_FROM_MONT, L_FROM_BE512, L_XMD_BI, L_SSWU_ISO, L_OPS
};

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ Fp hl_ld(const uint32_t* p) {
  Fp r;
  HB_UNROLL for (int i = 0; i < NL; i++) r.v[i] = p[i];
  return r;
}
__device__ __forceinline__ void hl_st(uint32_t* p, const Fp& a) {
  HB_UNROLL for (int i = 0; i < NL; i++) p[i] = a.v[i];
}
__device__ __forceinline__ void hl_st2(uint32_t* p, const Fp2& a) {
  hl_st(p, a.c0);
  hl_st(p + 12, a.c1);
}
#endif

template <int OP>
__global__ KB_OCC(HB_OCC_HASH) void k_h2c_leaf(const uint32_t* __restrict__ in, int n, uint32_t* __restrict__ out,
                                              int* __restrict__ flag) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int i = t < n ? t : n - 1;  // lanes past the last case shadow it and store nothing
  const uint32_t* p = in + 24 * (size_t)i;
  const Fp2 a = {hl_ld(p), hl_ld(p + 12)};
  uint32_t* o = out + 72 * (size_t)t;
  Fp2 r = f2_zero();
  int fl = 0;
  if constexpr (OP == L_POW_P_MINUS_2) r.c0 = fp_pow_win(a.c0, WIN_P_MINUS_2, WIN_P_MINUS_2_N);
  if constexpr (OP == L_POW_SQRT) r.c0 = fp_pow_win(a.c0, WIN_SQRT, WIN_SQRT_N);
  if constexpr (OP == L_POW_P_M3_4) r.c0 = fp_pow_win(a.c0, WIN_P_M3_4, WIN_P_M3_4_N);
  if constexpr (OP == L_POW_LEGENDRE) r.c0 = fp_pow_win(a.c0, WIN_LEGENDRE, WIN_LEGENDRE_N);
  if constexpr (OP == L_FP_SQRT) fl = fp_sqrt(r.c0, a.c0) ? 1 : 0;
  if constexpr (OP == L_FP_IS_SQUARE) fl = fp_is_square(a.c0) ? 1 : 0;
  if constexpr (OP == L_F2_SQRT) fl = f2_sqrt(r, a) ? 1 : 0;
  if constexpr (OP == L_F2_SGN0) fl = f2_sgn0(a);
  if constexpr (OP == L_F2_LEX) fl = f2_is_lex_largest(a) ? 1 : 0;
  if constexpr (OP == L_FROM_MONT) r.c0 = fp_from_mont(a.c0);
  if constexpr (OP == L_FROM_BE512) {
    uint32_t W[16];
    HB_UNROLL for (int k = 0; k < 16; k++) W[k] = p[k];
    r.c0 = fp_from_be512(W);
  }
  if constexpr (OP == L_XMD_BI) {
    uint32_t x[8];
    HB_UNROLL for (int k = 0; k < 8; k++) x[k] = p[k];
    const Sha256State s = xmd_bi(x, p[8]);
    if (t < n) {
      HB_UNROLL for (int k = 0; k < 8; k++) o[k] = s.h[k];
    }
  } else if constexpr (OP == L_SSWU_ISO) {
    const G2J q = sswu_iso_map(a);
    if (t < n) {
      hl_st2(o, q.X);
      hl_st2(o + 24, q.Y);
      hl_st2(o + 48, q.Z);
    }
  } else {
    if (t < n) hl_st2(o, r);
  }
  if (t < n) flag[t] = fl;
#endif
}

template <int OP>
static int h2c_leaf_run(int n, const uint32_t* in, uint32_t* out, int* flag) {
  DbDev dev;
  uint32_t *din, *dout;
  int* dflag;
  DB_MAKE(dev, din, in, (size_t)n * 24 * 4);
  DB_MAKE(dev, dout, nullptr, (size_t)n * 72 * 4);
  DB_MAKE(dev, dflag, nullptr, (size_t)n * 4);
  hipLaunchKernelGGL(k_h2c_leaf<OP>, dim3((n + 63) / 64), dim3(64), 0, 0, (const uint32_t*)din, n, dout, dflag);
  if (const int rc = db_finish()) return rc;
  if (const int rc = db_fetch(out, dout, (size_t)n * 72 * 4)) return rc;
  return db_fetch(flag, dflag, (size_t)n * 4);
}

extern "C" int db_h2c_leaf(int op, int n, const uint32_t* in, uint32_t* out, int* flag) {
  if (n < 1 || n > DB_H2C_MAX || !in || !out || !flag) return DB_E_ARG;
  switch (op) {
    case L_POW_P_MINUS_2: return h2c_leaf_run<L_POW_P_MINUS_2>(n, in, out, flag);
    case L_POW_SQRT: return h2c_leaf_run<L_POW_SQRT>(n, in, out, flag);
    case L_POW_P_M3_4: return h2c_leaf_run<L_POW_P_M3_4>(n, in, out, flag);
    case L_POW_LEGENDRE: return h2c_leaf_run<L_POW_LEGENDRE>(n, in, out, flag);
    case L_FP_SQRT: return h2c_leaf_run<L_FP_SQRT>(n, in, out, flag);
    case L_FP_IS_SQUARE: return h2c_leaf_run<L_FP_IS_SQUARE>(n, in, out, flag);
    case L_F2_SQRT: return h2c_leaf_run<L_F2_SQRT>(n, in, out, flag);
    case L_F2_SGN0: return h2c_leaf_run<L_F2_SGN0>(n, in, out, flag);
    case L_F2_LEX: return h2c_leaf_run<L_F2_LEX>(n, in, out, flag);
    case L_FROM_MONT: return h2c_leaf_run<L_FROM_MONT>(n, in, out, flag);
    case L_FROM_BE512: return h2c_leaf_run<L_FROM_BE512>(n, in, out, flag);
    case L_XMD_BI: return h2c_leaf_run<L_XMD_BI>(n, in, out, flag);
    case L_SSWU_ISO: return h2c_leaf_run<L_SSWU_ISO>(n, in, out, flag);
  }
  return DB_E_OP;
}

// xmd_b0 of message i (msgs + off[i], len[i]): out = 8 state words each
__global__ __launch_bounds__(64) void k_h2c_b0(const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ off,
                                               const uint32_t* __restrict__ len, int n, uint32_t* __restrict__ out) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (t >= n) return;  // as k_h2c_field: lanes past the last message leave
  const Sha256State s = xmd_b0(msgs + off[t], len[t]);
  HB_UNROLL for (int k = 0; k < 8; k++) out[8 * (size_t)t + k] = s.h[k];
#endif
}

extern "C" int db_h2c_b0(int n, const uint8_t* msgs, size_t msgs_bytes, const uint64_t* off, const uint32_t* len,
                         uint32_t* out) {
  if (n < 1 || n > DB_H2C_MAX || !msgs || !off || !len || !out || !db_ranges_ok(n, msgs_bytes, off, len)) return DB_E_ARG;
  DbDev dev;
  uint8_t* dmsgs;
  uint64_t* doff;
  uint32_t *dlen, *dout;
  DB_MAKE(dev, dmsgs, msgs, msgs_bytes);
  DB_MAKE(dev, doff, off, (size_t)n * 8);
  DB_MAKE(dev, dlen, len, (size_t)n * 4);
  DB_MAKE(dev, dout, nullptr, (size_t)n * 8 * 4);
  hipLaunchKernelGGL(k_h2c_b0, dim3((n + 63) / 64), dim3(64), 0, 0, (const uint8_t*)dmsgs, (const uint64_t*)doff,
                     (const uint32_t*)dlen, n, dout);
  if (const int rc = db_finish()) return rc;
  return db_fetch(out, dout, (size_t)n * 8 * 4);
}
#endif  // DB_H2C == 2
