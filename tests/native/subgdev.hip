// TEST-ONLY device harness of the batched subgroup test's second level (tests/test_gpu_subgroup_batch.py):
// this unit compiles the product's charon_amd/csrc/msm.hip itself and runs launch_subg_class and
// launch_subg_weigh -- the class sums of one wave per (window, digit place, digit value) and the 20
// weighted sums -- on explicit bucket contents.  Buckets go in as (bucket number, compressed point)
// pairs, every other bucket at infinity, and the 20 sums come out compressed, so the test compares
// with the oracle's group law.  The product library never loads this.  A library and an id of its
// own (build.py build_subgdev), built with fp.h's default HB_ARG_LANES as msm.hip in the library.
#include "../../charon_amd/csrc/msm.hip"

#include "devblocks.h"

using namespace hb;

// one lane per given bucket: decompressed (no subgroup check: the test gives curve points of any
// order), stored Jacobian with Z = 1; the infinity encoding leaves the bucket at infinity
__global__ __launch_bounds__(64) void k_sd_put(int m, const uint32_t* __restrict__ key, const uint8_t* __restrict__ pts,
                                               G2JEntry* __restrict__ bucket, uint8_t* __restrict__ bad) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  G2A p;
  bad[i] = g2_decompress(p, pts + 96ull * i, false);
  if (bad[i] || p.inf) return;
  const G2J j = jac_from_aff(p);
  bucket[key[i]] = {j.X, j.Y, j.Z};
#endif
}

__global__ __launch_bounds__(64) void k_sd_out(const G2JEntry* __restrict__ sums, uint8_t* __restrict__ out) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= SG_SUMS) return;
  const G2JEntry e = sums[t];
  g2_compress(out + 96ull * t, jac_to_aff(G2J{e.X, e.Y, e.Z}));
#endif
}

extern "C" const char* sd_build_id() { return SD_BUILD_ID; }
extern "C" int sd_keys() { return (int)SG_KEYS; }

// m buckets: key[i] = window * 13^4 + value (distinct), pts 96 bytes each; out: 20 x 96 bytes, sum
// (w, j) at w * 4 + j.  Returns 0, a DB_E_* code, or 1 when a point does not decode.
extern "C" int sd_sums(int m, const uint32_t* key, const uint8_t* pts, uint8_t* out) {
  if (m < 1 || !key || !pts || !out) return DB_E_ARG;
  for (int i = 0; i < m; i++) {
    if (key[i] >= SG_KEYS) return DB_E_ARG;
    for (int k = 0; k < i; k++)
      if (key[k] == key[i]) return DB_E_ARG;
  }
  DbDev d;
  uint32_t* dkey;
  uint8_t *dpts, *dbad, *dout;
  G2JEntry *bucket, *cls, *sums;
  DB_MAKE(d, dkey, key, (size_t)m * 4);
  DB_MAKE(d, dpts, pts, (size_t)m * 96);
  DB_MAKE(d, dbad, nullptr, (size_t)m);
  DB_MAKE(d, bucket, nullptr, (size_t)SG_KEYS * sizeof(G2JEntry));  // zero-filled: Z = 0, every bucket at infinity
  DB_MAKE(d, cls, nullptr, (size_t)SG_CLASSES * sizeof(G2JEntry));
  DB_MAKE(d, sums, nullptr, (size_t)SG_SUMS * sizeof(G2JEntry));
  DB_MAKE(d, dout, nullptr, (size_t)SG_SUMS * 96);
  hipLaunchKernelGGL(k_sd_put, dim3((m + 63) / 64), dim3(64), 0, 0, m, dkey, dpts, bucket, dbad);
  if (const int rc = db_finish()) return rc;
  uint8_t* hbad = new uint8_t[m];
  int rc = db_fetch(hbad, dbad, (size_t)m);
  for (int i = 0; !rc && i < m; i++)
    if (hbad[i]) rc = 1;
  delete[] hbad;
  if (rc) return rc;
  launch_subg_class(bucket, cls, 0);
  if (const int rc2 = db_finish()) return rc2;
  launch_subg_weigh(cls, sums, 0);
  if (const int rc2 = db_finish()) return rc2;
  hipLaunchKernelGGL(k_sd_out, dim3(1), dim3(64), 0, 0, sums, dout);
  if (const int rc2 = db_finish()) return rc2;
  return db_fetch(out, dout, (size_t)SG_SUMS * 96);
}
