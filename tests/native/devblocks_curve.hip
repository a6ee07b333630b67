// TEST-ONLY device block harness, curve layer: the point arithmetic in lazy 28-bit limbs (ec28.h),
// the stored-word Jacobian arithmetic (ec.h), the zero test and partial reduction the lazy formulas
// branch on, the endomorphism subgroup tests with their ladders and the chunk ladders of the random
// linear combination, each run by one kernel on chosen raw inputs so tests/test_gpu_curve.py can
// compare them with the oracle's group law (tests/blocks_ref.py).  The product library never loads
// this.  With devblocks_msm.hip it is a harness of its own (build.py DEVBLOCKS_CURVE: its own library
// and id), built with fp.h's default HB_ARG_LANES only (the curve kernels of vbatch.hip,
// threshold.hip, msm.hip and hashsplit.hip use that default).
//
// build.py compiles the file once per part, -DDB_CV=1 (G1 point operations), 2 (G2 point
// operations), 3 (zero test / reduction, subgroup tests and ladders, chunk ladders).
//
// Formats.  A point record is 88 words: six coordinate slots of 14 words (X.c0, X.c1, Y.c0, Y.c1,
// Z.c0, Z.c1; G1 uses the c0 slots), then the `inf` flag and three words of padding.  A slot holds
// 14 lazy limbs or, for the stored-word operations, 12 words.  The ladders take the product's own
// records (layout.h G1AEntry, HmEntry, G1JEntry, G2JEntry).  Every LANE writes what it holds, so a
// lane-pair run (ec28.h G1Half / F2Half over lanes (2i, 2i + 1)) shows both lanes' results; lanes
// without a case shadow the last one and store nothing (the outputs are cleared first).
//
// Left at verdict level: the two ladders inside ec28.h g1_in_subgroup28 are local to that function
// (it returns the verdict only), so [x^2] P is returned from ec.h jac_mul_by_xabs and
// g1_in_subgroup28 is checked by its verdict.
#include "devblocks.h"

using namespace hb;

#if !defined(DB_CV)
#error "compile with -DDB_CV=1, 2 or 3"
#endif

enum { PT_WORDS = 88, PT_INF = 84 };
enum { M_ONE = 0, M_HALF = 1 };
// point operations: P_L_* lazy limbs in and out (P_L_TOJAC: stored words out; P_L_FROMJAC, G2:
// stored words in), P_J_* stored words.  Q is affine (X, Y, inf) for P_L_MADD and P_J_ADD_AFF.
enum { P_L_DBL, P_L_MADD, P_L_ADD, P_L_TOJAC, P_L_FROMJAC, P_J_DBL, P_J_ADD, P_J_ADD_AFF, P_J_EQ, P_OPS };

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ Fp cv_ld(const uint32_t* p) {
  Fp r;
  HB_UNROLL for (int i = 0; i < NL; i++) r.v[i] = p[i];
  return r;
}
__device__ __forceinline__ void cv_st(uint32_t* p, const Fp& a) {
  HB_UNROLL for (int i = 0; i < NL; i++) p[i] = a.v[i];
}
__device__ __forceinline__ L28 cv_ldl(const uint32_t* p) {
  L28 r;
  HB_UNROLL for (int i = 0; i < 14; i++) r.l[i] = p[i];
  return r;
}
__device__ __forceinline__ void cv_stl(uint32_t* p, const L28& a) {
  HB_UNROLL for (int i = 0; i < 14; i++) p[i] = a.l[i];
}

template <int F>
struct Cv;
template <>
struct Cv<1> {
  using LP = G1L;
  using JP = G1J;
  using AP = G1A;
  static __device__ __forceinline__ Fp lds(const uint32_t* p) { return cv_ld(p); }
  static __device__ __forceinline__ void sts(uint32_t* p, const Fp& a) { cv_st(p, a); }
  static __device__ __forceinline__ L28 ldl(const uint32_t* p) { return cv_ldl(p); }
  static __device__ __forceinline__ void stl(uint32_t* p, const L28& a) { cv_stl(p, a); }
};
template <>
struct Cv<2> {
  using LP = G2L;
  using JP = G2J;
  using AP = G2A;
  static __device__ __forceinline__ Fp2 lds(const uint32_t* p) { return {cv_ld(p), cv_ld(p + 14)}; }
  static __device__ __forceinline__ void sts(uint32_t* p, const Fp2& a) {
    cv_st(p, a.c0);
    cv_st(p + 14, a.c1);
  }
  static __device__ __forceinline__ F2L ldl(const uint32_t* p) { return {cv_ldl(p), cv_ldl(p + 14)}; }
  static __device__ __forceinline__ void stl(uint32_t* p, const F2L& a) {
    cv_stl(p, a.c0);
    cv_stl(p + 14, a.c1);
  }
};

template <int F, int MODE>
__device__ __forceinline__ auto cv_mode() {
  if constexpr (F == 1) {
    if constexpr (MODE == M_HALF) return g1half_make();
    else return G1One{};
  } else {
    if constexpr (MODE == M_HALF) return f2half_make();
    else return F2One{};
  }
}

template <class M>
__device__ __forceinline__ G1L cvl_dbl(const G1L& p, M m) { return g1l_dbl(p, m); }
template <class M>
__device__ __forceinline__ G2L cvl_dbl(const G2L& p, M m) { return g2l_dbl(p, m); }
template <class M>
__device__ __forceinline__ G1L cvl_madd(const G1L& p, const G1L& q, M m) { return g1l_madd(p, q.X, q.Y, m); }
template <class M>
__device__ __forceinline__ G2L cvl_madd(const G2L& p, const G2L& q, M m) { return g2l_madd(p, q.X, q.Y, m); }
template <class M>
__device__ __forceinline__ G1L cvl_add(const G1L& p, const G1L& q, M m) { return g1l_add(p, q, m); }
template <class M>
__device__ __forceinline__ G2L cvl_add(const G2L& p, const G2L& q, M m) { return g2l_add(p, q, m); }
__device__ __forceinline__ G1J cvl_to_jac(const G1L& p) { return g1l_to_jac(p); }
__device__ __forceinline__ G2J cvl_to_jac(const G2L& p) { return g2l_to_jac(p); }
#endif

// ---- point operations: case i = two point records (P, Q); out[88 t ..] and flag[t] of thread t
template <int F, int MODE, int OP>
__global__ KB_OCC(HB_OCC_RLC) void k_cv_point(const uint32_t* __restrict__ in, int n, uint32_t* __restrict__ out,
                                             int* __restrict__ flag) {
#if defined(__HIP_DEVICE_COMPILE__)
  using C = Cv<F>;
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int c = MODE == M_HALF ? t >> 1 : t;
  const bool valid = c < n;
  const int i = valid ? c : n - 1;
  const uint32_t* pp = in + 2 * PT_WORDS * (size_t)i;
  const uint32_t* qp = pp + PT_WORDS;
  uint32_t* o = out + PT_WORDS * (size_t)t;
  int fl = 0;
  if constexpr (OP <= P_L_TOJAC) {
    const typename C::LP p = {C::ldl(pp), C::ldl(pp + 28), C::ldl(pp + 56), pp[PT_INF] != 0};
    const typename C::LP q = {C::ldl(qp), C::ldl(qp + 28), C::ldl(qp + 56), qp[PT_INF] != 0};
    const auto m = cv_mode<F, MODE>();
    if constexpr (OP == P_L_TOJAC) {
      const typename C::JP r = cvl_to_jac(p);
      if (valid) {
        C::sts(o, r.X);
        C::sts(o + 28, r.Y);
        C::sts(o + 56, r.Z);
      }
    } else {
      typename C::LP r = p;
      if constexpr (OP == P_L_DBL) r = cvl_dbl(p, m);
      if constexpr (OP == P_L_MADD) r = cvl_madd(p, q, m);
      if constexpr (OP == P_L_ADD) r = cvl_add(p, q, m);
      if (valid) {
        C::stl(o, r.X);
        C::stl(o + 28, r.Y);
        C::stl(o + 56, r.Z);
        o[PT_INF] = r.inf ? 1u : 0u;
      }
    }
  } else {
    const typename C::JP p = {C::lds(pp), C::lds(pp + 28), C::lds(pp + 56)};
    const typename C::JP q = {C::lds(qp), C::lds(qp + 28), C::lds(qp + 56)};
    if constexpr (OP == P_L_FROMJAC) {
      if constexpr (F == 2) {
        const G2L r = g2l_from_jac(p);
        if (valid) {
          C::stl(o, r.X);
          C::stl(o + 28, r.Y);
          C::stl(o + 56, r.Z);
          o[PT_INF] = r.inf ? 1u : 0u;
        }
      }
    } else {
      typename C::JP r = p;
      if constexpr (OP == P_J_DBL) r = jac_dbl(p);
      if constexpr (OP == P_J_ADD) r = jac_add(p, q);
      if constexpr (OP == P_J_ADD_AFF) r = jac_add_aff(p, typename C::AP{q.X, q.Y, qp[PT_INF] != 0});
      if constexpr (OP == P_J_EQ) fl = jac_eq(p, q) ? 1 : 0;
      if (valid) {
        C::sts(o, r.X);
        C::sts(o + 28, r.Y);
        C::sts(o + 56, r.Z);
      }
    }
  }
  if (valid) flag[t] = fl;
#endif
}

static constexpr bool cv_point_has(int f, int mode, int op) {
  if (op < 0 || op >= P_OPS) return false;
  if (mode == M_HALF) return op <= P_L_ADD;  // the policies reach the formulas' products only
  return op != P_L_FROMJAC || f == 2;
}
static int cv_threads(int mode, int n) { return ((mode == M_HALF ? 2 * n : n) + 63) / 64 * 64; }

template <int F, int MODE, int OP>
static int cv_point_run(int n, const uint32_t* in, uint32_t* out, int* flag) {
  if constexpr (!cv_point_has(F, MODE, OP)) {
    return DB_E_OP;
  } else {
    const int threads = cv_threads(MODE, n);
    DbDev dev;
    uint32_t *din, *dout;
    int* dflag;
    DB_MAKE(dev, din, in, (size_t)n * 2 * PT_WORDS * 4);
    DB_MAKE(dev, dout, nullptr, (size_t)threads * PT_WORDS * 4);
    DB_MAKE(dev, dflag, nullptr, (size_t)threads * 4);
    hipLaunchKernelGGL((k_cv_point<F, MODE, OP>), dim3(threads / 64), dim3(64), 0, 0, din, n, dout, dflag);
    if (const int rc = db_finish()) return rc;
    if (const int rc = db_fetch(out, dout, (size_t)threads * PT_WORDS * 4)) return rc;
    return db_fetch(flag, dflag, (size_t)threads * 4);
  }
}

template <int F, int MODE>
static int cv_point_op(int op, int n, const uint32_t* in, uint32_t* out, int* flag) {
  switch (op) {
    case P_L_DBL: return cv_point_run<F, MODE, P_L_DBL>(n, in, out, flag);
    case P_L_MADD: return cv_point_run<F, MODE, P_L_MADD>(n, in, out, flag);
    case P_L_ADD: return cv_point_run<F, MODE, P_L_ADD>(n, in, out, flag);
    case P_L_TOJAC: return cv_point_run<F, MODE, P_L_TOJAC>(n, in, out, flag);
    case P_L_FROMJAC: return cv_point_run<F, MODE, P_L_FROMJAC>(n, in, out, flag);
    case P_J_DBL: return cv_point_run<F, MODE, P_J_DBL>(n, in, out, flag);
    case P_J_ADD: return cv_point_run<F, MODE, P_J_ADD>(n, in, out, flag);
    case P_J_ADD_AFF: return cv_point_run<F, MODE, P_J_ADD_AFF>(n, in, out, flag);
    case P_J_EQ: return cv_point_run<F, MODE, P_J_EQ>(n, in, out, flag);
  }
  return DB_E_OP;
}

#if DB_CV == 1 || DB_CV == 2
// db_point_g<F>(mode, op, n, in, out, flag): in = n cases of two point records; out = one record
// and flag = one int for each of db_curve_threads(mode, n) threads (db_curve_threads: part 3)
#define DB_CAT_(a, b) a##b
#define DB_CAT(a, b) DB_CAT_(a, b)
extern "C" int DB_CAT(db_point_g, DB_CV)(int mode, int op, int n, const uint32_t* in, uint32_t* out, int* flag) {
  if (n < 1 || !in || !out || !flag) return DB_E_ARG;
  if (mode == M_ONE) return cv_point_op<DB_CV, M_ONE>(op, n, in, out, flag);
  if (mode == M_HALF) return cv_point_op<DB_CV, M_HALF>(op, n, in, out, flag);
  return DB_E_OP;
}
#endif

#if DB_CV == 3
extern "C" const char* db_build_id() { return DB_BUILD_ID; }
extern "C" int db_curve_threads(int mode, int n) {
  if (n < 1 || (mode != M_ONE && mode != M_HALF)) return DB_E_ARG;
  return cv_threads(mode, n);
}
extern "C" int db_g_ready() { return (int)G_READY; }

// ---- a. zero test and reductions.  Case i: two L28 (a, b), 28 words; out: 14 limbs; flag[i]
enum { S_IS_ZERO, S_F2_IS_ZERO, S_NORM, S_RED, S_OPS };

template <int OP>
__global__ __launch_bounds__(64) void k_cv_scalar(const uint32_t* __restrict__ in, int n, uint32_t* __restrict__ out,
                                                  int* __restrict__ flag) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int i = t < n ? t : n - 1;
  const L28 a = cv_ldl(in + 28 * (size_t)i), b = cv_ldl(in + 28 * (size_t)i + 14);
  L28 r = a;
  int fl = 0;
  if constexpr (OP == S_IS_ZERO) fl = l_is_zero(a) ? 1 : 0;
  if constexpr (OP == S_F2_IS_ZERO) fl = f2l_is_zero(F2L{a, b}) ? 1 : 0;
  if constexpr (OP == S_NORM) r = l_norm(a);
  if constexpr (OP == S_RED) r = l_red(a);
  if (t < n) {
    cv_stl(out + 14 * (size_t)t, r);
    flag[t] = fl;
  }
#endif
}

template <int OP>
static int cv_scalar_run(int n, const uint32_t* in, uint32_t* out, int* flag) {
  DbDev dev;
  uint32_t *din, *dout;
  int* dflag;
  DB_MAKE(dev, din, in, (size_t)n * 28 * 4);
  DB_MAKE(dev, dout, nullptr, (size_t)n * 14 * 4);
  DB_MAKE(dev, dflag, nullptr, (size_t)n * 4);
  hipLaunchKernelGGL(k_cv_scalar<OP>, dim3((n + 63) / 64), dim3(64), 0, 0, din, n, dout, dflag);
  if (const int rc = db_finish()) return rc;
  if (const int rc = db_fetch(out, dout, (size_t)n * 14 * 4)) return rc;
  return db_fetch(flag, dflag, (size_t)n * 4);
}

extern "C" int db_lazy_scalar(int op, int n, const uint32_t* in, uint32_t* out, int* flag) {
  if (n < 1 || !in || !out || !flag) return DB_E_ARG;
  switch (op) {
    case S_IS_ZERO: return cv_scalar_run<S_IS_ZERO>(n, in, out, flag);
    case S_F2_IS_ZERO: return cv_scalar_run<S_F2_IS_ZERO>(n, in, out, flag);
    case S_NORM: return cv_scalar_run<S_NORM>(n, in, out, flag);
    case S_RED: return cv_scalar_run<S_RED>(n, in, out, flag);
  }
  return DB_E_OP;
}

// ---- c. ladders and subgroup tests.  LD_MUL: G2 [|x|] P of a G2JEntry (g2l_mul_by_xabs_l, P read
// again from memory at each addition as hashsplit.hip reads it) into a G2JEntry; G1 [x^2] P of a
// G1AEntry (jac_mul_by_xabs twice) into a G1JEntry.  LD_SUB: flag = g1_in_subgroup28 of a G1AEntry
// / g2_in_subgroup28_l of an HmEntry (read again from memory, as vbatch.hip k_g2_subgroup).
enum { LD_MUL, LD_SUB };

template <int F, int MODE, int OP>
__global__ KB_OCC(HB_OCC_SUBG) void k_cv_ladder(const void* __restrict__ in, int n, void* __restrict__ out,
                                               int* __restrict__ flag) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int c = MODE == M_HALF ? t >> 1 : t;
  const bool valid = c < n;
  const int i = valid ? c : n - 1;
  const auto m = cv_mode<F, MODE>();
  int fl = 0;
  if constexpr (F == 2 && OP == LD_MUL) {
    const G2JEntry* src = (const G2JEntry*)in + i;
    const G2J r = g2l_mul_by_xabs_l([src]() { return G2J{src->X, src->Y, src->Z}; }, m);
    if (valid) ((G2JEntry*)out)[t] = {r.X, r.Y, r.Z};
  }
  if constexpr (F == 2 && OP == LD_SUB) {
    const HmEntry* src = (const HmEntry*)in + i;
    fl = g2_in_subgroup28_l([src]() { return G2A{src->x, src->y, src->inf != 0}; }, m) ? 1 : 0;
  }
  if constexpr (F == 1 && OP == LD_MUL) {
    const G1J r = jac_mul_by_xabs(jac_mul_by_xabs_aff(g1a_load(((const G1AEntry*)in)[i])));
    if (valid) ((G1JEntry*)out)[t] = {r.X, r.Y, r.Z};
  }
  if constexpr (F == 1 && OP == LD_SUB) fl = g1_in_subgroup28(g1a_load(((const G1AEntry*)in)[i]), m) ? 1 : 0;
  if (valid) flag[t] = fl;
#endif
}

template <int F, int MODE, int OP>
static int cv_ladder_run(int n, const void* in, void* out, int* flag) {
  constexpr size_t in_rec = F == 1 ? sizeof(G1AEntry) : (OP == LD_MUL ? sizeof(G2JEntry) : sizeof(HmEntry));
  constexpr size_t out_rec = F == 1 ? sizeof(G1JEntry) : sizeof(G2JEntry);
  const int threads = cv_threads(MODE, n);
  DbDev dev;
  void *din, *dout;
  int* dflag;
  DB_MAKE(dev, din, in, (size_t)n * in_rec);
  DB_MAKE(dev, dout, nullptr, (size_t)threads * out_rec);
  DB_MAKE(dev, dflag, nullptr, (size_t)threads * 4);
  hipLaunchKernelGGL((k_cv_ladder<F, MODE, OP>), dim3(threads / 64), dim3(64), 0, 0, (const void*)din, n, dout, dflag);
  if (const int rc = db_finish()) return rc;
  if (OP == LD_MUL)
    if (const int rc = db_fetch(out, dout, (size_t)threads * out_rec)) return rc;
  return db_fetch(flag, dflag, (size_t)threads * 4);
}

// db_ladder(field 1 / 2, mode, op, n, in, out, flag): records as above; out (LD_MUL) one Jacobian
// record and flag one int for each of db_curve_threads(mode, n) threads
extern "C" int db_ladder(int field, int mode, int op, int n, const void* in, void* out, int* flag) {
  static_assert(sizeof(G1AEntry) == 28 * 4 && sizeof(HmEntry) == 52 * 4 && sizeof(G1JEntry) == 36 * 4 &&
                    sizeof(G2JEntry) == 72 * 4 && sizeof(G1J) == sizeof(G1JEntry) && sizeof(G2J) == sizeof(G2JEntry),
                "raw-word layouts of layout.h");
  if (n < 1 || !in || !out || !flag) return DB_E_ARG;
  const int key = field * 100 + mode * 10 + op;
  switch (key) {
    case 100 + LD_MUL: return cv_ladder_run<1, M_ONE, LD_MUL>(n, in, out, flag);
    case 100 + LD_SUB: return cv_ladder_run<1, M_ONE, LD_SUB>(n, in, out, flag);
    case 110 + LD_SUB: return cv_ladder_run<1, M_HALF, LD_SUB>(n, in, out, flag);
    case 200 + LD_MUL: return cv_ladder_run<2, M_ONE, LD_MUL>(n, in, out, flag);
    case 210 + LD_MUL: return cv_ladder_run<2, M_HALF, LD_MUL>(n, in, out, flag);
    case 200 + LD_SUB: return cv_ladder_run<2, M_ONE, LD_SUB>(n, in, out, flag);
    case 210 + LD_SUB: return cv_ladder_run<2, M_HALF, LD_SUB>(n, in, out, flag);
  }
  return DB_E_OP;
}

// ---- chunk ladders: lane t runs the ladder over items first[t] .. first[t] + cnt[t] - 1 of one
// explicit table (dense: 3 affine Z = 1 records per item and a uint2; sparse: 4 records and a
// uint4) and writes its Jacobian sum to out[t]
template <int F, bool SPARSE>
__global__ KB_OCC(HB_OCC_RLC) void k_cv_chunk(const void* __restrict__ tab, const void* __restrict__ coef,
                                             const uint32_t* __restrict__ first, const uint32_t* __restrict__ cnt, int n,
                                             void* __restrict__ out) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int i = t < n ? t : n - 1;
  if constexpr (F == 1) {
    const G1J r = SPARSE ? g1l_msm_ladder_sparse((const G1J*)tab, (const uint4*)coef, first[i], cnt[i])
                         : g1l_msm_ladder((const G1J*)tab, (const uint2*)coef, first[i], cnt[i]);
    if (t < n) ((G1JEntry*)out)[t] = {r.X, r.Y, r.Z};
  } else {
    const G2J r = SPARSE ? g2l_msm_ladder_sparse((const G2J*)tab, (const uint4*)coef, first[i], cnt[i])
                         : g2l_msm_ladder((const G2J*)tab, (const uint2*)coef, first[i], cnt[i]);
    if (t < n) ((G2JEntry*)out)[t] = {r.X, r.Y, r.Z};
  }
#endif
}

template <int F, bool SPARSE>
static int cv_chunk_run(int n, int items, const void* tab, const uint32_t* coef, const uint32_t* first,
                        const uint32_t* cnt, void* out) {
  constexpr size_t rec = F == 1 ? sizeof(G1JEntry) : sizeof(G2JEntry);
  for (int t = 0; t < n; t++)  // every lane's range inside the table
    if ((uint64_t)first[t] + cnt[t] > (uint64_t)items) return DB_E_ARG;
  DbDev dev;
  void *dtab, *dcoef, *dout;
  uint32_t *dfirst, *dcnt;
  DB_MAKE(dev, dtab, tab, (size_t)items * (SPARSE ? 4 : 3) * rec);
  DB_MAKE(dev, dcoef, coef, (size_t)items * (SPARSE ? 16 : 8));
  DB_MAKE(dev, dfirst, first, (size_t)n * 4);
  DB_MAKE(dev, dcnt, cnt, (size_t)n * 4);
  DB_MAKE(dev, dout, nullptr, (size_t)n * rec);
  hipLaunchKernelGGL((k_cv_chunk<F, SPARSE>), dim3((n + 63) / 64), dim3(64), 0, 0, (const void*)dtab, (const void*)dcoef,
                     (const uint32_t*)dfirst, (const uint32_t*)dcnt, n, dout);
  if (const int rc = db_finish()) return rc;
  return db_fetch(out, dout, (size_t)n * rec);
}

extern "C" int db_chunk_ladder(int field, int sparse, int n, int items, const void* tab, const uint32_t* coef,
                               const uint32_t* first, const uint32_t* cnt, void* out) {
  if (n < 1 || items < 1 || !tab || !coef || !first || !cnt || !out) return DB_E_ARG;
  if (field == 1) return sparse ? cv_chunk_run<1, true>(n, items, tab, coef, first, cnt, out)
                                : cv_chunk_run<1, false>(n, items, tab, coef, first, cnt, out);
  if (field == 2) return sparse ? cv_chunk_run<2, true>(n, items, tab, coef, first, cnt, out)
                                : cv_chunk_run<2, false>(n, items, tab, coef, first, cnt, out);
  return DB_E_OP;
}
#endif
