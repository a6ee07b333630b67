// TEST-ONLY device harness of the cluster handles' kernels (tests/test_gpu_cluster_kernels.py): this
// unit compiles the product's charon_amd/csrc/cluster.hip itself and runs launch_cluster_keys and
// launch_cluster_wide on explicit words.  Every output array is uploaded as the caller filled it, `pad`
// sentinel entries behind its last element included, and copied back in full, so that what a kernel
// must not write is visible to the test.  The product library never loads this.  A library and an id
// of its own (build.py build_clusterdev).
#include "../../charon_amd/csrc/cluster.hip"

#include <algorithm>
#include <vector>

#include "devblocks.h"

using namespace hb;

extern "C" const char* cd_build_id() { return CD_BUILD_ID; }
extern "C" int cd_entry_bytes() { return (int)sizeof(G1AEntry); }
extern "C" int cd_wide_bytes() { return (int)sizeof(G1WidePt); }

// k_cluster_keys: n items (group, share_idx; share_idx null: the DV-key mode) against a shard's table of
// n_keys entries (ent: n_keys x sizeof(G1AEntry) bytes as the test wrote them, st: n_keys bytes).
// Out, each with `pad` sentinel entries behind it: vpk (entries), vpkst (bytes), went (words; nullable).
extern "C" int cd_keys(int n, const uint32_t* group, const int64_t* share_idx, uint32_t group_base, uint32_t n_groups,
                       uint32_t n_shares, uint32_t n_keys, uint32_t tables, const uint8_t* ent, const uint8_t* st, int pad,
                       uint8_t* vpk, uint8_t* vpkst, uint32_t* went) {
  if (n < 1 || pad < 0 || n_keys < 1 || !group || !ent || !st || !vpk || !vpkst) return DB_E_ARG;
  // the table the kernel indexes is as large as the rule's key numbers can get
  if ((uint64_t)n_groups * (1ull + n_shares) > n_keys) return DB_E_ARG;
  DbIo io;
  ClusterKeysArgs a{};
  DB_IN(io, a.group, group, (size_t)n * 4);
  DB_IN(io, a.share_idx, share_idx, (size_t)n * 8);
  DB_IN(io, a.ent, ent, (size_t)n_keys * sizeof(G1AEntry));
  DB_IN(io, a.st, st, (size_t)n_keys);
  DB_IO(io, a.vpk, vpk, ((size_t)n + pad) * sizeof(G1AEntry));
  DB_IO(io, a.vpkst, vpkst, (size_t)n + pad);
  DB_IO(io, a.went, went, ((size_t)n + pad) * 4);
  a.n = (uint32_t)n;
  a.group_base = group_base;
  a.n_groups = n_groups;
  a.n_shares = n_shares;
  a.n_keys = n_keys;
  a.tables = tables;
  launch_cluster_keys(a, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// the test's keys into entries, as the product's decompression leaves a good key (no subgroup check:
// the test gives points of G1); bad[i]: the key did not decode
__global__ __launch_bounds__(64) void k_cd_entries(int n, const uint8_t* __restrict__ pks, G1AEntry* __restrict__ ent,
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

// one lane per table slot: the point compressed (a slot the kernel left alone holds the test's sentinel
// bytes, which the test reads from `wide` itself and never from here)
__global__ __launch_bounds__(64) void k_cd_compress(int n, const uint8_t* __restrict__ skip, const G1WidePt* __restrict__ wide,
                                                    uint8_t* __restrict__ out) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || skip[i / (int)KEY_WIDE_PTS]) return;
  const G1WidePt w = wide[i];
  g1_compress(out + 48ull * i, G1A{w.x, w.y, false});
#endif
}

// k_cluster_wide: n keys (48 bytes each, points of G1) with the statuses the test gives them (st: a
// non-zero status must be skipped).  wide: (15 n + pad) table points, preset by the caller and copied
// back in full; out: 48 bytes per table point of the keys with status 0, compressed.
extern "C" int cd_wide(int n, const uint8_t* pks, const uint8_t* st, int pad, uint8_t* wide, uint8_t* out) {
  if (n < 1 || pad < 0 || !pks || !st || !wide || !out) return DB_E_ARG;
  DbIo io;
  const uint8_t *dpk, *dst;
  G1AEntry* dent;
  uint8_t *dbad, *dout;
  G1WidePt* dwide;
  const size_t slots = (size_t)n * KEY_WIDE_PTS;
  std::vector<uint8_t> zero(std::max((size_t)n * sizeof(G1AEntry), slots * 48), 0);
  DB_IN(io, dpk, pks, (size_t)n * 48);
  DB_IN(io, dst, st, (size_t)n);
  DB_IN(io, dent, zero.data(), (size_t)n * sizeof(G1AEntry));
  DB_IN(io, dbad, zero.data(), (size_t)n);
  DB_IO(io, dwide, wide, (slots + pad) * sizeof(G1WidePt));
  DB_IO(io, dout, out, slots * 48);
  hipLaunchKernelGGL(k_cd_entries, dim3((n + 63) / 64), dim3(64), 0, 0, n, dpk, dent, dbad);
  if (const int rc = db_finish()) return rc;
  std::vector<uint8_t> hbad(n);
  if (const int rc = db_fetch(hbad.data(), dbad, (size_t)n)) return rc;
  for (int i = 0; i < n; i++)
    if (hbad[i]) return 1;
  launch_cluster_wide(dent, dst, (uint32_t)n, dwide, 0);
  if (const int rc = db_finish()) return rc;
  hipLaunchKernelGGL(k_cd_compress, dim3(((int)slots + 63) / 64), dim3(64), 0, 0, (int)slots, dst, dwide, dout);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}
