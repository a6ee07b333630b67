// TEST-ONLY device harness of the learned keys' ladder tables (tests/test_gpu_key_wide.py): ec28.h
// g1_wide_build, g1l_msm_ladder_wide and g1l_mul_wide run by two kernels on chosen keys, chunks and
// coefficients, as vbatch.hip k_pk_wide, k_rlc_msm<1, 2> and k_rlc<1> run them (the same headers,
// included as the product's fast translation units include them).  Points go in and out
// compressed, so the test compares with the oracle's group law.  The product library never loads
// this.  A library and an id of its own (build.py build_widedev).
#include "devblocks.h"

using namespace hb;

// one lane per key: decompressed (no subgroup check: the test gives points of G1), its table at
// wide[15 ent[i] ..] -- the entry numbers are the test's, not the items' positions
__global__ __launch_bounds__(64) void k_wd_tables(int n, const uint8_t* __restrict__ pks,
                                                  const uint32_t* __restrict__ ent, G1WidePt* __restrict__ wide,
                                                  uint8_t* __restrict__ bad) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  G1A p;
  bad[i] = g1_decompress(p, pks + 48ull * i, false);
  if (bad[i] || p.inf) {
    bad[i] = 1;
    return;
  }
  g1_wide_build(p, wide + (uint64_t)KEY_WIDE_PTS * ent[i]);
#endif
}

// one lane per chunk (chunks of different sizes in neighbouring lanes): its sum through the tables,
// and its first item alone through the one-item ladder, both compressed
__global__ __launch_bounds__(64, 2) void k_wd_chunks(int nc, const uint32_t* __restrict__ cfirst,
                                                     const uint32_t* __restrict__ ccount,
                                                     const uint2* __restrict__ coef, const uint32_t* __restrict__ ent,
                                                     const G1WidePt* __restrict__ wide, uint8_t* __restrict__ out,
                                                     uint8_t* __restrict__ one) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const uint32_t first = cfirst[c], cnt = ccount[c];
  g1_compress(out + 48ull * c, jac_to_aff(g1l_msm_ladder_wide(wide, ent, coef, first, cnt)));
  const uint2 ab = coef[first];
  g1_compress(one + 48ull * c, jac_to_aff(g1l_mul_wide(wide + (uint64_t)KEY_WIDE_PTS * ent[first], ab.x, ab.y)));
#endif
}

extern "C" const char* wd_build_id() { return WD_BUILD_ID; }

// n keys (48 bytes each) with their coefficient pairs, nc chunks (first item, count) over them;
// out / one: 48 bytes per chunk.  Returns 0, a DB_E_* code, or 1 when a key does not decode.
extern "C" int wd_chunks(int n, const uint8_t* pks, const uint32_t* coef, int nc, const uint32_t* cfirst,
                         const uint32_t* ccount, uint8_t* out, uint8_t* one) {
  if (n < 1 || nc < 1 || !pks || !coef || !cfirst || !ccount || !out || !one) return DB_E_ARG;
  for (int c = 0; c < nc; c++)  // every chunk inside the items
    if (ccount[c] < 1 || cfirst[c] >= (uint32_t)n || ccount[c] > (uint32_t)n - cfirst[c]) return DB_E_ARG;
  uint32_t* hent = new uint32_t[n];
  for (int i = 0; i < n; i++) hent[i] = (uint32_t)(n - 1 - i);  // entry numbers in reverse item order
  DbDev d, o;
  uint8_t *dpk, *dbad, *dout, *done;
  uint32_t *dent, *dcf, *dcc;
  uint2* dcoef;
  G1WidePt* dwide;
  const int rc_ent = d.make((void**)&dent, hent, (size_t)n * 4);
  delete[] hent;
  if (rc_ent) return rc_ent;
  DB_MAKE(d, dpk, pks, (size_t)n * 48);
  DB_MAKE(d, dcoef, coef, (size_t)n * sizeof(uint2));
  DB_MAKE(d, dcf, cfirst, (size_t)nc * 4);
  DB_MAKE(d, dcc, ccount, (size_t)nc * 4);
  DB_MAKE(d, dwide, nullptr, (size_t)n * KEY_WIDE_PTS * sizeof(G1WidePt));
  DB_MAKE(d, dbad, nullptr, (size_t)n);
  DB_MAKE(o, dout, nullptr, (size_t)nc * 48);
  DB_MAKE(o, done, nullptr, (size_t)nc * 48);
  hipLaunchKernelGGL(k_wd_tables, dim3((n + 63) / 64), dim3(64), 0, 0, n, dpk, dent, dwide, dbad);
  if (const int rc = db_finish()) return rc;
  uint8_t* hbad = new uint8_t[n];
  int rc = db_fetch(hbad, dbad, (size_t)n);
  for (int i = 0; !rc && i < n; i++)
    if (hbad[i]) rc = 1;
  delete[] hbad;
  if (rc) return rc;
  hipLaunchKernelGGL(k_wd_chunks, dim3((nc + 63) / 64), dim3(64), 0, 0, nc, dcf, dcc, dcoef, dent, dwide, dout, done);
  if (const int rc2 = db_finish()) return rc2;
  if (const int rc2 = db_fetch(out, dout, (size_t)nc * 48)) return rc2;
  return db_fetch(one, done, (size_t)nc * 48);
}
