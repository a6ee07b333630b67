// TEST-ONLY device block harness, leaves: the Fp / Fp2 products, the carry chains, the inversion
// and the lazy-limb products and lane-pair / six-lane policies of charon_amd/csrc (fp.h, ec28.h,
// pair6.h fp_dot2, pair28.h F2Hex), each run by one kernel on chosen raw limbs, so
// tests/test_gpu_blocks.py can compare the gfx950 code with Python integers.  The product library
// never loads this.  Values cross the interface as raw limbs (devblocks.h describes the builds).
#include "devblocks.h"

using namespace hb;

extern "C" const char* db_build_id() { return DB_BUILD_ID; }
extern "C" int db_arg_lanes() { return DB_BLOCK; }  // == HB_ARG_LANES (devblocks.h)

// ---- A. stored words: one lane per case.  Case i: four Fp (a0, a1, b0, b1), 48 words; out: two Fp
// (r0, r1), 24 words; flag[i]: fp_dot2's neg; aux[i]: the inversion's batch count.  Lanes past the
// last case shadow it (whole waves run, as in the product's kernels) and store nothing.
enum { A_ADD, A_SUB, A_NEG, A_MUL, A_SQR, A_F2MUL, A_F2SQR, A_DOT2, A_MUL28, A_SQR28, A_INV, A_INVCT, A_OPS };

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ Fp db_ld(const uint32_t* p) {
  Fp r;
  HB_UNROLL for (int i = 0; i < NL; i++) r.v[i] = p[i];
  return r;
}
__device__ __forceinline__ void db_st(uint32_t* p, const Fp& a) {
  HB_UNROLL for (int i = 0; i < NL; i++) p[i] = a.v[i];
}
__device__ __forceinline__ L28 db_ldl(const uint32_t* p) {
  L28 r;
  HB_UNROLL for (int i = 0; i < 14; i++) r.l[i] = p[i];
  return r;
}
__device__ __forceinline__ void db_stl(uint32_t* p, const L28& a) {
  HB_UNROLL for (int i = 0; i < 14; i++) p[i] = a.l[i];
}
#endif

template <int OP>
__global__ __launch_bounds__(DB_BLOCK) void k_db_fp(const uint32_t* __restrict__ in, const int* __restrict__ flag, int n,
                                                   uint32_t* __restrict__ out, int* __restrict__ aux) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = t < n ? t : n - 1;
  const Fp a0 = db_ld(in + 48 * i), a1 = db_ld(in + 48 * i + 12), b0 = db_ld(in + 48 * i + 24),
           b1 = db_ld(in + 48 * i + 36);
  Fp r0 = fp_zero(), r1 = fp_zero();
  int bt = 0;
  if constexpr (OP == A_ADD) r0 = fp_add(a0, b0);
  if constexpr (OP == A_SUB) r0 = fp_sub(a0, b0);
  if constexpr (OP == A_NEG) r0 = fp_neg(a0);
  if constexpr (OP == A_MUL) r0 = fp_mul(a0, b0);
  if constexpr (OP == A_SQR) r0 = fp_sqr(a0);
  if constexpr (OP == A_F2MUL) fp2_mul_pair(r0, r1, a0, a1, b0, b1);
  if constexpr (OP == A_F2SQR) fp2_sqr_pair(r0, r1, a0, a1);
  if constexpr (OP == A_DOT2) r0 = fp_dot2(a0, b0, a1, b1, flag[i] != 0);  // a0 b0 +- a1 b1
  if constexpr (OP == A_MUL28) r0 = fp28_to(fp28_mul(fp28_from(a0), fp28_from(b0)));
  if constexpr (OP == A_SQR28) r0 = fp28_to(fp28_sqr(fp28_from(a0)));
  if constexpr (OP == A_INV) r0 = fp_inv(a0, &bt);
  if constexpr (OP == A_INVCT) r0 = fp_inv_ct(a0, &bt);
  if (t < n) {
    db_st(out + 24 * t, r0);
    db_st(out + 24 * t + 12, r1);
    aux[t] = bt;
  }
#endif
}

template <int OP>
static int db_fp_run(int n, const uint32_t* in, const int* flag, uint32_t* out, int* aux) {
  DbDev dev;
  uint32_t *din, *dout;
  int *dflag, *daux;
  DB_MAKE(dev, din, in, (size_t)n * 48 * 4);
  DB_MAKE(dev, dflag, flag, (size_t)n * 4);
  DB_MAKE(dev, dout, nullptr, (size_t)n * 24 * 4);
  DB_MAKE(dev, daux, nullptr, (size_t)n * 4);
  hipLaunchKernelGGL(k_db_fp<OP>, dim3((n + DB_BLOCK - 1) / DB_BLOCK), dim3(DB_BLOCK), 0, 0, din, dflag, n, dout, daux);
  if (const int rc = db_finish()) return rc;
  if (const int rc = db_fetch(out, dout, (size_t)n * 24 * 4)) return rc;
  return db_fetch(aux, daux, (size_t)n * 4);
}

extern "C" int db_fp(int op, int n, const uint32_t* in, const int* flag, uint32_t* out, int* aux) {
  if (n < 1 || !in || !flag || !out || !aux) return DB_E_ARG;
  switch (op) {
    case A_ADD: return db_fp_run<A_ADD>(n, in, flag, out, aux);
    case A_SUB: return db_fp_run<A_SUB>(n, in, flag, out, aux);
    case A_NEG: return db_fp_run<A_NEG>(n, in, flag, out, aux);
    case A_MUL: return db_fp_run<A_MUL>(n, in, flag, out, aux);
    case A_SQR: return db_fp_run<A_SQR>(n, in, flag, out, aux);
    case A_F2MUL: return db_fp_run<A_F2MUL>(n, in, flag, out, aux);
    case A_F2SQR: return db_fp_run<A_F2SQR>(n, in, flag, out, aux);
    case A_DOT2: return db_fp_run<A_DOT2>(n, in, flag, out, aux);
    case A_MUL28: return db_fp_run<A_MUL28>(n, in, flag, out, aux);
    case A_SQR28: return db_fp_run<A_SQR28>(n, in, flag, out, aux);
    case A_INV: return db_fp_run<A_INV>(n, in, flag, out, aux);
    case A_INVCT: return db_fp_run<A_INVCT>(n, in, flag, out, aux);
  }
  return DB_E_OP;
}

// ---- B. lazy limbs.  Case i: twelve L28 (x0 .. x11), 168 words.  Every LANE writes what it holds:
// out[84 t ..] = six L28 (r0 .. r5) of thread t, so that the test sees that both lanes of a pair /
// all six lanes of a role hold the same value.  One lane per case (B_L*, B_F2*), one case per lane
// pair (B_H_*: ec28.h F2Half / G1Half over lanes (2i, 2i + 1)) or one case per six lanes of a
// pair28.h Grp18 role (B_X_*: F2Hex; nine roles per wave, lanes 54..63 shadow).  Lanes without a
// case shadow the last one and store nothing (the output is cleared first).
enum {
  B_LMUL, B_LSQR, B_LMUL2, B_LSQR2, B_F2MUL, B_F2SQR36, B_F2SQR78, B_F2SQR9, B_LDOT,
  B_H_FM, B_H_FS36, B_H_FS78, B_H_PMUL2, B_H_PSQR2,
  B_X_FM3, B_X_FM2, B_X_FS3,
  B_OPS
};
static constexpr int db_lanes_per_case(int op) { return op < B_H_FM ? 1 : op < B_X_FM3 ? 2 : 6; }
static constexpr int db_cases_per_block(int op) {
  return op < B_H_FM ? DB_BLOCK : op < B_X_FM3 ? DB_BLOCK / 2 : 9 * (DB_BLOCK / 64);
}

template <int OP>
__global__ __launch_bounds__(DB_BLOCK) void k_db_lazy(const uint32_t* __restrict__ in, int n, uint32_t* __restrict__ out) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  constexpr int LPC = db_lanes_per_case(OP);
  int c;
  bool valid;
  if constexpr (LPC == 6) {
    const int lane = (int)(threadIdx.x & 63u);
    c = (t >> 6) * 9 + lane / 6;
    valid = lane < 54 && c < n;
  } else {
    c = t / LPC;
    valid = c < n;
  }
  const int i = valid ? c : n - 1;
  L28 x[12], r[6];
  HB_UNROLL for (int k = 0; k < 12; k++) x[k] = db_ldl(in + 168 * i + 14 * k);
  HB_UNROLL for (int k = 0; k < 6; k++) r[k] = l_zero();
  F2L t0 = f2l_zero(), t1 = f2l_zero(), t2 = f2l_zero();
  const F2L A = {x[0], x[1]}, B = {x[2], x[3]};
  if constexpr (OP == B_LMUL) r[0] = l_mul(x[0], x[1]);
  if constexpr (OP == B_LSQR) r[0] = l_sqr(x[0]);
  if constexpr (OP == B_LMUL2) l_mul2(x[0], x[1], x[2], x[3], r[0], r[1]);
  if constexpr (OP == B_LSQR2) l_sqr2(x[0], x[1], r[0], r[1]);
  if constexpr (OP == B_LDOT) r[0] = l_dot(x[0], x[1], x[2], x[3]);  // x0 x2 + x1 x3
  if constexpr (OP == B_H_PMUL2) p_mul2(g1half_make(), x[0], x[1], x[2], x[3], r[0], r[1]);
  if constexpr (OP == B_H_PSQR2) p_sqr2(g1half_make(), x[0], x[1], r[0], r[1]);
  if constexpr (OP == B_F2MUL) t0 = f2l_mul(A, B);
  if constexpr (OP == B_F2SQR36) t0 = f2l_sqr_k<36, 1>(A);
  if constexpr (OP == B_F2SQR78) t0 = f2l_sqr_k<78, 1>(A);
  if constexpr (OP == B_F2SQR9) t0 = f2l_sqr_k<9, 2>(A);
  if constexpr (OP == B_H_FM) t0 = fm(f2half_make(), A, B);
  if constexpr (OP == B_H_FS36) t0 = fs<36, 1>(f2half_make(), A);
  if constexpr (OP == B_H_FS78) t0 = fs<78, 1>(f2half_make(), A);
  if constexpr (OP == B_X_FM3)
    fm3(grp18_make().hx, A, B, F2L{x[4], x[5]}, F2L{x[6], x[7]}, F2L{x[8], x[9]}, F2L{x[10], x[11]}, t0, t1, t2);
  if constexpr (OP == B_X_FM2) fm2(grp18_make().hx, A, B, F2L{x[4], x[5]}, F2L{x[6], x[7]}, t0, t1);
  if constexpr (OP == B_X_FS3) fs3<9, 2>(grp18_make().hx, A, B, F2L{x[4], x[5]}, t0, t1, t2);
  if constexpr (OP >= B_F2MUL && OP != B_LDOT && OP != B_H_PMUL2 && OP != B_H_PSQR2) {
    r[0] = t0.c0;
    r[1] = t0.c1;
    r[2] = t1.c0;
    r[3] = t1.c1;
    r[4] = t2.c0;
    r[5] = t2.c1;
  }
  if (valid) {
    HB_UNROLL for (int k = 0; k < 6; k++) db_stl(out + 84 * (size_t)t + 14 * k, r[k]);
  }
#endif
}

template <int OP>
static int db_lazy_run(int n, const uint32_t* in, uint32_t* out) {
  const int per = db_cases_per_block(OP), blocks = (n + per - 1) / per;
  const size_t out_bytes = (size_t)blocks * DB_BLOCK * 84 * 4;
  DbDev dev;
  uint32_t *din, *dout;
  DB_MAKE(dev, din, in, (size_t)n * 168 * 4);
  DB_MAKE(dev, dout, nullptr, out_bytes);
  hipLaunchKernelGGL(k_db_lazy<OP>, dim3(blocks), dim3(DB_BLOCK), 0, 0, din, n, dout);
  if (const int rc = db_finish()) return rc;
  return db_fetch(out, dout, out_bytes);
}

// threads launched for n cases of op (out holds 84 words for each), or DB_E_OP
extern "C" int db_lazy_threads(int op, int n) {
  if (op < 0 || op >= B_OPS || n < 1) return DB_E_OP;
  const int per = db_cases_per_block(op);
  return (n + per - 1) / per * DB_BLOCK;
}

extern "C" int db_lazy(int op, int n, const uint32_t* in, uint32_t* out) {
  if (n < 1 || !in || !out) return DB_E_ARG;
  switch (op) {
    case B_LMUL: return db_lazy_run<B_LMUL>(n, in, out);
    case B_LSQR: return db_lazy_run<B_LSQR>(n, in, out);
    case B_LMUL2: return db_lazy_run<B_LMUL2>(n, in, out);
    case B_LSQR2: return db_lazy_run<B_LSQR2>(n, in, out);
    case B_F2MUL: return db_lazy_run<B_F2MUL>(n, in, out);
    case B_F2SQR36: return db_lazy_run<B_F2SQR36>(n, in, out);
    case B_F2SQR78: return db_lazy_run<B_F2SQR78>(n, in, out);
    case B_F2SQR9: return db_lazy_run<B_F2SQR9>(n, in, out);
    case B_LDOT: return db_lazy_run<B_LDOT>(n, in, out);
    case B_H_FM: return db_lazy_run<B_H_FM>(n, in, out);
    case B_H_FS36: return db_lazy_run<B_H_FS36>(n, in, out);
    case B_H_FS78: return db_lazy_run<B_H_FS78>(n, in, out);
    case B_H_PMUL2: return db_lazy_run<B_H_PMUL2>(n, in, out);
    case B_H_PSQR2: return db_lazy_run<B_H_PSQR2>(n, in, out);
    case B_X_FM3: return db_lazy_run<B_X_FM3>(n, in, out);
    case B_X_FM2: return db_lazy_run<B_X_FM2>(n, in, out);
    case B_X_FS3: return db_lazy_run<B_X_FS3>(n, in, out);
  }
  return DB_E_OP;
}
