// TEST-ONLY device harness of hbls_cluster_check's kernels (tests/test_gpu_lock_check_kernels.py): this
// unit compiles the product's charon_amd/csrc/lockcheck.hip itself and runs launch_lock_check on the
// test's keys and statuses.  Every output array is uploaded as the caller filled it, `pad` sentinel
// entries behind its last element included, and copied back in full, so that what a kernel must not
// write is visible to the test.  The product library never loads this.  A library and an id of its own
// (build.py build_lockcheckdev).
#include "../../charon_amd/csrc/lockcheck.hip"

#include <vector>

#include "devblocks.h"

using namespace hb;

extern "C" const char* ld_build_id() { return LD_BUILD_ID; }

// the test's keys into entries, as the product's decompression leaves a good key (no subgroup check:
// the test gives points of G1, the point at infinity among them); bad[i]: the key did not decode
__global__ __launch_bounds__(64) void k_ld_entries(int n, const uint8_t* __restrict__ pks, G1AEntry* __restrict__ ent,
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

// k_lock_check + k_lock_fold: n_rows rows of 1 + n_shares keys (pks: 48 bytes each, row-major; st: the
// statuses the test gives them) at threshold t.  Out, each with `pad` sentinel entries behind it:
// verdict (n_rows * (n_shares - t + 1) bytes), row_status (bytes), row_windows (64-bit words).
// -> 0; 1: a key did not decode; 2: lockcheck.h refuses (n_shares, t); DB_E_*
extern "C" int ld_check(int n_rows, uint32_t n_shares, uint32_t t, const uint8_t* pks, const uint8_t* st, int pad,
                        uint8_t* verdict, uint8_t* row_status, uint64_t* row_windows) {
  if (n_rows < 1 || pad < 0 || !pks || !st || !verdict || !row_status || !row_windows) return DB_E_ARG;
  LockPlan plan;
  if (!lock_plan(n_shares, t, plan)) return 2;
  const size_t nk = (size_t)n_rows * (1 + n_shares), lanes = (size_t)n_rows * plan.windows;
  DbIo io;
  const uint8_t *dpk, *dst;
  G1AEntry* dent;
  uint8_t *dbad, *dverdict, *dstatus;
  uint64_t* dwindows;
  std::vector<uint8_t> zero(nk * sizeof(G1AEntry), 0);
  DB_IN(io, dpk, pks, nk * 48);
  DB_IN(io, dst, st, nk);
  DB_IN(io, dent, zero.data(), nk * sizeof(G1AEntry));
  DB_IN(io, dbad, zero.data(), nk);
  DB_IO(io, dverdict, verdict, lanes + pad);
  DB_IO(io, dstatus, row_status, (size_t)n_rows + pad);
  DB_IO(io, dwindows, row_windows, ((size_t)n_rows + pad) * 8);
  hipLaunchKernelGGL(k_ld_entries, dim3(((int)nk + 63) / 64), dim3(64), 0, 0, (int)nk, dpk, dent, dbad);
  if (const int rc = db_finish()) return rc;
  std::vector<uint8_t> hbad(nk);
  if (const int rc = db_fetch(hbad.data(), dbad, nk)) return rc;
  for (size_t i = 0; i < nk; i++)
    if (hbad[i]) return 1;
  launch_lock_check(dent, dst, (uint32_t)n_rows, plan, dverdict, dstatus, dwindows, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}
