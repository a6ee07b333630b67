// Cluster handles (hbls_cluster_open / hbls_duty_open_cluster; the rule is cluster.h's): the keys of
// a cluster lock, resident and immutable, and the key phase of a duty that takes its keys from them.
//   k_cluster_wide  1 lane / key of the cluster, once at open: the ladder table (ec28.h g1_wide_build)
//                   of every good, finite key into the cluster's own G1WidePt array; any other key's
//                   slots are left as they are, and k_cluster_keys never reports such a key's number
//   k_cluster_keys  8 lanes / item, 7 of them moving 16 bytes each (as duty.hip k_duty_copy moves its
//                   records, so the loads and stores coalesce): the item's key by (group, share index)
//                   -- or, share_idx null, the DV key of a fired group -- through cluster.h cluster_key
//                   into what the verification's key phase leaves: the entry, its status (an entry at
//                   infinity with ST_BAD_PUBKEY when the pair names no key) and the key's number for
//                   the ladder tables
// Compiled like vbatch.hip (HB_FAST_FPMUL): k_cluster_wide is vbatch.hip k_pk_wide's arithmetic.
#define HB_FAST_FPMUL 1
#include "lines.h"
#include "rlc.h"

#include <cstddef>

#include "cluster.h"

namespace hb {

constexpr uint32_t CK_WORDS = sizeof(G1AEntry) / 16;  // 16-byte words of an entry
constexpr uint32_t CK_LANES = 8;                      // lanes per item
static_assert(sizeof(G1AEntry) % 16 == 0 && CK_WORDS <= CK_LANES, "k_cluster_keys: 8 lanes of 16 bytes per entry");
static_assert(offsetof(G1AEntry, inf) == 16 * (CK_WORDS - 1), "k_cluster_keys: the last word holds the infinity flag");

__global__ KB_OCC(HB_OCC_DECPK) void k_cluster_wide(const G1AEntry* __restrict__ ent, const uint8_t* __restrict__ st,
                                                    uint32_t n, G1WidePt* __restrict__ wide) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || st[i]) return;
  const G1AEntry pe = ent[i];
  if (pe.inf) return;
  g1_wide_build(G1A{pe.x, pe.y, false}, wide + (uint64_t)KEY_WIDE_PTS * i);
#endif
}

__global__ __launch_bounds__(256) void k_cluster_keys(ClusterKeysArgs a) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t i = j / CK_LANES;
  const uint32_t l = (uint32_t)(j % CK_LANES);
  if (i >= a.n || l >= CK_WORDS) return;
  // the one place a value of the caller's becomes an address: the rule, then the shard's own size
  uint32_t k = cluster_key(a.group[i], a.share_idx ? a.share_idx[i] : 0, a.group_base, a.n_groups, a.n_shares,
                           a.share_idx == nullptr);
  if (k != CLUSTER_NO_KEY && k >= a.n_keys) k = CLUSTER_NO_KEY;
  uint4 w = make_uint4(0u, 0u, 0u, 0u);
  if (k != CLUSTER_NO_KEY) w = reinterpret_cast<const uint4*>(a.ent)[(size_t)k * CK_WORDS + l];
  else if (l == CK_WORDS - 1) w.x = 1u;  // no key: the point at infinity
  reinterpret_cast<uint4*>(a.vpk)[(size_t)i * CK_WORDS + l] = w;
  if (l != CK_WORDS - 1) return;  // the lane that holds the infinity flag writes the item's two words
  const uint8_t s = k != CLUSTER_NO_KEY ? a.st[k] : (uint8_t)ST_BAD_PUBKEY;
  a.vpkst[i] = s;
  if (a.went) a.went[i] = (a.tables && k != CLUSTER_NO_KEY && !s && !w.x) ? k : KEY_WIDE_NONE;
}

static inline unsigned cluster_blocks(size_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }

void launch_cluster_wide(const G1AEntry* ent, const uint8_t* st, uint32_t n, G1WidePt* wide, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_cluster_wide, dim3(cluster_blocks(n, 64)), dim3(64), 0, s, ent, st, n, wide);
}
void launch_cluster_keys(const ClusterKeysArgs& a, hipStream_t s) {
  if (a.n) hipLaunchKernelGGL(k_cluster_keys, dim3(cluster_blocks((size_t)a.n * CK_LANES, 256)), dim3(256), 0, s, a);
}

}  // namespace hb
