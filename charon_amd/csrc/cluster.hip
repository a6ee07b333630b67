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
//                   the ladder tables.  any_entry (hbls_cluster_verify_batch): an item's own index may be 0,
//                   its validator's DV key; the duty paths leave it 0
//   k_cluster_row_sum  1 lane / row (hbls_cluster_verify_aggregate; the rule is clustersel.h's): the sum
//                   of the row's selected entries straight from the resident table, by ec28.h's complete
//                   mixed additions (equal keys double, cancelling keys give the identity, an entry at
//                   infinity is the identity), as a Jacobian point for vbatch.hip k_seg_sum<false>, with
//                   the OR of the selected entries' statuses.  Which entries a row adds is a kernel
//                   argument, so the loop is wave-uniform; a selected entry with a non-zero status sets
//                   the flag and is not added (k_va_status answers before the sum is looked at).  Only
//                   reads the cluster; plain vector stores only.
// Compiled like vbatch.hip (HB_FAST_FPMUL): k_cluster_wide is vbatch.hip k_pk_wide's arithmetic.
#define HB_FAST_FPMUL 1
#include "lines.h"
#include "rlc.h"

#include <cstddef>

#include "cluster.h"
#include "clustersel.h"

// two waves per SIMD, as lockcheck.hip's ladder over the same additions (HB_OCC_LOCK)
#define HB_OCC_ROWSUM 2

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
                           a.share_idx == nullptr || a.any_entry != 0);
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

__global__ KB_OCC(HB_OCC_ROWSUM) void k_cluster_row_sum(const G1AEntry* __restrict__ ent, const uint8_t* __restrict__ st,
                                                         uint32_t n_rows, uint32_t n_shares, uint64_t share_mask,
                                                         uint32_t with_dv, G1JEntry* __restrict__ out,
                                                         uint8_t* __restrict__ st_out) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_rows) return;
  const uint64_t first = row * (1ull + n_shares);  // j <= n_shares below: every entry read is the row's own
  G1L R = g1l_infinity();
  uint8_t bad = 0;
  HB_NOUNROLL for (uint32_t j = 0; j <= n_shares; j++) {
    if (!cluster_sel_entry(j, share_mask, with_dv)) continue;  // wave-uniform
    const uint8_t s = st[first + j];
    bad |= s;
    if (s || ent[first + j].inf) continue;  // no point to add / the identity
    R = g1l_madd(R, l_from(ent[first + j].x), l_from(ent[first + j].y));
  }
  const G1J J = g1l_to_jac(R);
  out[row] = {J.X, J.Y, J.Z};
  st_out[row] = bad;
#endif
}

static inline unsigned cluster_blocks(size_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }

void launch_cluster_wide(const G1AEntry* ent, const uint8_t* st, uint32_t n, G1WidePt* wide, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_cluster_wide, dim3(cluster_blocks(n, 64)), dim3(64), 0, s, ent, st, n, wide);
}
void launch_cluster_keys(const ClusterKeysArgs& a, hipStream_t s) {
  if (a.n) hipLaunchKernelGGL(k_cluster_keys, dim3(cluster_blocks((size_t)a.n * CK_LANES, 256)), dim3(256), 0, s, a);
}
void launch_cluster_row_sum(const G1AEntry* ent, const uint8_t* st, uint32_t n_rows, uint32_t n_shares, uint64_t share_mask,
                            uint32_t with_dv, G1JEntry* out, uint8_t* st_out, hipStream_t s) {
  if (n_rows)
    hipLaunchKernelGGL(k_cluster_row_sum, dim3(cluster_blocks(n_rows, 64)), dim3(64), 0, s, ent, st, n_rows, n_shares,
                       share_mask, with_dv, out, st_out);
}

}  // namespace hb
