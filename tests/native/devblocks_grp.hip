// TEST-ONLY device block harness, lane groups: one Fp12 value per group of 3 (pair3.h Grp), 6
// (pair6.h Grp6) or 18 lanes (pair28.h Grp18), the lazy-limb lane operations of pair28.h and the
// stored-word ones the product still calls (k_pair3<P3_PROD>'s g_mul, the final exponentiation's
// g_inv / g6_inv and g_is_one / g6_is_one), each run by one kernel on chosen raw limbs so
// tests/test_gpu_blocks.py can compare them with the oracle's Fp12.  Units, idle groups and shadow
// lanes are indexed as pipeline.hip's k_pair3 / k_pair6_fin index them.  The product library never
// loads this.
#include "devblocks.h"

using namespace hb;

enum { G_GRP = 0, G_GRP6 = 1, G_GRP18 = 2 };
enum {
  C_SQR, C_MUL, C_MUL_LINE, C_CYC, C_CONJ, C_FROB1, C_FROB2, C_FEXP, C_IS_ONE,  // pair28.h g4_*, any group
  C_S_MUL,                                                                      // g_mul (Grp)
  C_S_INV, C_S_IS_ONE,                                                          // g_inv / g6_inv, g_is_one / g6_is_one
  C_OPS
};
static constexpr bool db_has(int gk, int op) {
  return op < C_S_MUL || (op == C_S_MUL && gk == G_GRP) || (op > C_S_MUL && op < C_OPS && gk != G_GRP18);
}
static constexpr int db_lanes(int gk) { return gk == G_GRP ? 3 : gk == G_GRP6 ? 6 : 18; }
static constexpr int db_per_wave(int gk) { return gk == G_GRP ? 21 : gk == G_GRP6 ? 10 : 3; }

#if defined(__HIP_DEVICE_COMPILE__)
template <int GK>
__device__ __forceinline__ auto db_group() {
  if constexpr (GK == G_GRP) return grp_make();
  else if constexpr (GK == G_GRP6) return grp6_make();
  else return grp18_make();
}
#endif

// A, B: n values, three Fp4Entry each (role k at [3 u + k]); for C_MUL_LINE B[3 u ..] holds the
// line (a0, a1, b1: one LineEntry in the first 72 words).  Every lane writes the Fp4 it holds to
// out[t] and its verdict (C_IS_ONE, C_S_IS_ONE: of A; C_FEXP: of the result) to flag[t]; lanes of
// idle groups shadow the last unit and store nothing (both outputs are cleared first).
template <int GK, int OP>
__global__ KB_OCC(HB_OCC_PAIR3) void k_db_grp(const Fp4Entry* __restrict__ A, const Fp4Entry* __restrict__ B, int n,
                                              Fp4Entry* __restrict__ out, int* __restrict__ flag) {
#if defined(__HIP_DEVICE_COMPILE__)
  const auto g = db_group<GK>();
  constexpr int LANES = db_lanes(GK), PER_WAVE = db_per_wave(GK);
  const int grp = (int)(threadIdx.x & 63u) / LANES;
  const int unit = (int)blockIdx.x * PER_WAVE + grp;
  const bool valid = grp < PER_WAVE && unit < n;
  const int u = valid ? unit : n - 1;
  const Fp4Entry a = A[3 * (size_t)u + g.k], b = B[3 * (size_t)u + g.k];
  Fp4Entry r = {f2_zero(), f2_zero()};
  int fl = 0;
  if constexpr (OP < C_S_MUL) {
    const F4L fa = f4l_from(a.x, a.y), fb = f4l_from(b.x, b.y);
    F4L fr = fa;
    if constexpr (OP == C_SQR) fr = g4_sqr(g, fa);
    if constexpr (OP == C_MUL) fr = g4_mul(g, fa, fb);
    if constexpr (OP == C_MUL_LINE) {
      const LineEntry* L = reinterpret_cast<const LineEntry*>(B + 3 * (size_t)u);
      F2L l0, l1, l2;
      line_split(*L, l0, l1, l2);
      fr = g4_mul_line(g, fa, l0, l1, l2);
    }
    if constexpr (OP == C_CYC) fr = g4_cyc(g, fa);
    if constexpr (OP == C_CONJ) fr = g4_conj(g.k, fa);
    if constexpr (OP == C_FROB1) fr = g4_frob<1>(g.k, fa, fe_m(g));
    if constexpr (OP == C_FROB2) fr = g4_frob<2>(g.k, fa, fe_m(g));
    if constexpr (OP == C_FEXP) {
      fr = g4_final_exp(g, fa);
      fl = g4_is_one(g, fr) ? 1 : 0;
    }
    if constexpr (OP == C_IS_ONE) fl = g4_is_one(g, fa) ? 1 : 0;
    r = f4l_store(fr);
  } else {
    const Fp4 va = {a.x, a.y}, vb = {b.x, b.y};
    Fp4 vr = va;
    if constexpr (GK == G_GRP) {
      if constexpr (OP == C_S_MUL) vr = g_mul(g, va, vb);
      if constexpr (OP == C_S_INV) vr = g_inv(g, va);
      if constexpr (OP == C_S_IS_ONE) fl = g_is_one(g, va) ? 1 : 0;
    }
    if constexpr (GK == G_GRP6) {
      if constexpr (OP == C_S_INV) vr = g6_inv(g, va);
      if constexpr (OP == C_S_IS_ONE) fl = g6_is_one(g, va) ? 1 : 0;
    }
    r = Fp4Entry{vr.x, vr.y};
  }
  if (valid) {
    const size_t t = (size_t)blockIdx.x * 64 + (threadIdx.x & 63u);
    out[t] = r;
    flag[t] = fl;
  }
#endif
}

template <int GK, int OP>
static int db_grp_run(int n, const uint32_t* A, const uint32_t* B, uint32_t* out, int* flag) {
  if constexpr (!db_has(GK, OP)) {
    return DB_E_OP;
  } else {
    const int blocks = (n + db_per_wave(GK) - 1) / db_per_wave(GK);
    const size_t lanes = (size_t)blocks * 64;
    DbDev dev;
    Fp4Entry *dA, *dB, *dout;
    int* dflag;
    DB_MAKE(dev, dA, A, (size_t)n * 3 * sizeof(Fp4Entry));
    DB_MAKE(dev, dB, B, (size_t)n * 3 * sizeof(Fp4Entry));
    DB_MAKE(dev, dout, nullptr, lanes * sizeof(Fp4Entry));
    DB_MAKE(dev, dflag, nullptr, lanes * 4);
    hipLaunchKernelGGL((k_db_grp<GK, OP>), dim3(blocks), dim3(64), 0, 0, dA, dB, n, dout, dflag);
    if (const int rc = db_finish()) return rc;
    if (const int rc = db_fetch(out, dout, lanes * sizeof(Fp4Entry))) return rc;
    return db_fetch(flag, dflag, lanes * 4);
  }
}

template <int GK>
static int db_grp_op(int op, int n, const uint32_t* A, const uint32_t* B, uint32_t* out, int* flag) {
  switch (op) {
    case C_SQR: return db_grp_run<GK, C_SQR>(n, A, B, out, flag);
    case C_MUL: return db_grp_run<GK, C_MUL>(n, A, B, out, flag);
    case C_MUL_LINE: return db_grp_run<GK, C_MUL_LINE>(n, A, B, out, flag);
    case C_CYC: return db_grp_run<GK, C_CYC>(n, A, B, out, flag);
    case C_CONJ: return db_grp_run<GK, C_CONJ>(n, A, B, out, flag);
    case C_FROB1: return db_grp_run<GK, C_FROB1>(n, A, B, out, flag);
    case C_FROB2: return db_grp_run<GK, C_FROB2>(n, A, B, out, flag);
    case C_FEXP: return db_grp_run<GK, C_FEXP>(n, A, B, out, flag);
    case C_IS_ONE: return db_grp_run<GK, C_IS_ONE>(n, A, B, out, flag);
    case C_S_MUL: return db_grp_run<GK, C_S_MUL>(n, A, B, out, flag);
    case C_S_INV: return db_grp_run<GK, C_S_INV>(n, A, B, out, flag);
    case C_S_IS_ONE: return db_grp_run<GK, C_S_IS_ONE>(n, A, B, out, flag);
  }
  return DB_E_OP;
}

// This unit's lane group (build.py compiles the file once per group kind, -DDB_GK=0 / 1 / 2: Grp,
// Grp6, Grp18 -- three units of a third of the compile time each): db_grp<K>(op, n, A, B, out,
// flag), and db_grp<K>_lanes(n), the lanes launched for n values (out: 48 words, flag: one int for
// each).
#if !defined(DB_GK)
#error "compile with -DDB_GK=0, 1 or 2"
#endif
#define DB_CAT_(a, b, c) a##b##c
#define DB_CAT(a, b, c) DB_CAT_(a, b, c)

extern "C" int DB_CAT(db_grp, DB_GK, _lanes)(int n) {
  if (n < 1) return DB_E_ARG;
  return (n + db_per_wave(DB_GK) - 1) / db_per_wave(DB_GK) * 64;
}

extern "C" int DB_CAT(db_grp, DB_GK, )(int op, int n, const uint32_t* A, const uint32_t* B, uint32_t* out, int* flag) {
  static_assert(sizeof(Fp4Entry) == 48 * 4 && sizeof(LineEntry) == 72 * 4, "raw-limb layouts of layout.h");
  if (n < 1 || !A || !B || !out || !flag) return DB_E_ARG;
  return db_grp_op<DB_GK>(op, n, A, B, out, flag);
}
