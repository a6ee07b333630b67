// TEST-ONLY device harness of hbls_cluster_verify_aggregate's row kernel (tests/test_gpu_cluster_sum_kernels.py):
// this unit compiles the product's charon_amd/csrc/cluster.hip itself and runs launch_cluster_row_sum on
// the test's keys and statuses.  Every output array is uploaded as the caller filled it, `pad` sentinel
// entries behind its last element included, and copied back in full, so that what the kernel must not
// write is visible to the test.  The product library never loads this.  A library and an id of its own
// (build.py build_clustersumdev).
#include "../../../charon_amd/csrc/cluster.hip"

#include <vector>

#include "../devblocks.h"

using namespace hb;

extern "C" const char* csd_build_id() { return CSD_BUILD_ID; }
extern "C" int csd_sum_bytes() { return (int)sizeof(G1JEntry); }

// the test's keys into entries, as the product's decompression leaves a good key (no subgroup check:
// the test gives points of G1, the point at infinity among them); bad[i]: the key did not decode
__global__ __launch_bounds__(64) void k_csd_entries(int n, const uint8_t* __restrict__ pks, G1AEntry* __restrict__ ent,
                                                    uint8_t* __restrict__ bad) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  G1A p;
  bad[i] = g1_decompress(p, pks + 48ull * i, false);
  if (bad[i]) p = g1_generator();
  G1AEntry e;
  e.x = p.x;
  e.y = p.y;
  e.inf = p.inf ? 1u : 0u;
  e.pad[0] = e.pad[1] = e.pad[2] = 0;
  ent[i] = e;
#endif
}

// k_cluster_row_sum: n_rows rows of 1 + n_shares keys (pks: 48 bytes each, row-major; st: the statuses the
// test gives them) under (share_mask, with_dv).  Out, each with `pad` sentinel entries behind it: sums
// (n_rows Jacobian points of sizeof(G1JEntry) bytes), flags (n_rows bytes).
// -> 0; 1: a key did not decode; 2: clustersel.h refuses the selection; DB_E_*
extern "C" int csd_row_sum(int n_rows, uint32_t n_shares, uint64_t share_mask, uint32_t with_dv, const uint8_t* pks,
                           const uint8_t* st, int pad, uint8_t* sums, uint8_t* flags) {
  if (n_rows < 1 || pad < 0 || !pks || !st || !sums || !flags) return DB_E_ARG;
  if (!cluster_sel_valid(share_mask, with_dv, n_shares)) return 2;
  const size_t nk = (size_t)n_rows * (1 + n_shares);
  DbIo io;
  const uint8_t *dpk, *dst;
  G1AEntry* dent;
  uint8_t *dbad, *dflags;
  G1JEntry* dsums;
  std::vector<uint8_t> zero(nk * sizeof(G1AEntry), 0);
  DB_IN(io, dpk, pks, nk * 48);
  DB_IN(io, dst, st, nk);
  DB_IN(io, dent, zero.data(), nk * sizeof(G1AEntry));
  DB_IN(io, dbad, zero.data(), nk);
  DB_IO(io, dsums, sums, ((size_t)n_rows + pad) * sizeof(G1JEntry));
  DB_IO(io, dflags, flags, (size_t)n_rows + pad);
  hipLaunchKernelGGL(k_csd_entries, dim3(((int)nk + 63) / 64), dim3(64), 0, 0, (int)nk, dpk, dent, dbad);
  if (const int rc = db_finish()) return rc;
  std::vector<uint8_t> hbad(nk);
  if (const int rc = db_fetch(hbad.data(), dbad, nk)) return rc;
  for (size_t i = 0; i < nk; i++)
    if (hbad[i]) return 1;
  launch_cluster_row_sum(dent, dst, (uint32_t)n_rows, n_shares, share_mask, with_dv, dsums, dflags, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}
