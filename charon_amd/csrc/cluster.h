// The key rule of a cluster handle (hbls_cluster_open / hbls_duty_open_cluster): which key of the
// cluster lock a partial names.  The reference ties a partial's public key to its share index inside
// the verifier (core/parsigex/parsigex.go:146-170 NewEth2Verifier: the pubshare is looked up by (DV
// pubkey, ShareIdx) in the lock, "unknown pubkey, not part of cluster lock" / "invalid shareIdx" before
// any pairing runs); a cluster duty does the same on the device, from (group, share_idx).
//
// A cluster's keys are numbered row-major: row g (validator g) holds 1 + n_shares keys, entry 0 the
// validator's DV key, entry j (1 .. n_shares) its pubshare of share index j.  A shard holds the rows
// of its groups [group_base, group_base + n_groups), so a key's number within the shard is
//     (group - group_base) (1 + n_shares) + j.
// ONE function holds the rule, with the DV key of a fired group as the same function under a flag
// (`dv`: entry 0 is then allowed -- and the callers pass share 0 -- where a partial may only name 1 ..
// n_shares).  A value that comes from the caller's data is never an address without this check.
//
// No HIP in here: cluster.hip's k_cluster_keys calls cluster_key once per item, hipbls.hip counts
// hbls_cluster_stats with it on the host, and the CPU harness tests/native/clustercheck.cpp compiles
// the same function for tests/test_cluster_host.py.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CLUSTER_HD __host__ __device__ inline
#else
#define CLUSTER_HD inline
#endif

namespace hb {

constexpr uint32_t CLUSTER_NO_KEY = 0xffffffffu;  // the pair names no key of the shard
constexpr uint32_t CLUSTER_MAX_SHARES = 64;       // dutysel.h DUTY_MAX_STORED: a group never stores more

// The number of the key (group, share_idx) names within a shard of n_groups groups from group_base,
// each of 1 + n_shares keys, or CLUSTER_NO_KEY.  A partial (dv false) has a key iff group_base <= group
// < group_base + n_groups and 1 <= share_idx <= n_shares; a DV key (dv true) iff the group is the
// shard's and 0 <= share_idx <= n_shares.  Every comparison is made on the full 64 bits of share_idx
// and on 64-bit sums of the group bounds: 2^32 + 1, a negative value or INT64_MIN has no key and is
// never truncated into one.  The result is below n_groups (1 + n_shares); a caller that keeps it in
// 32 bits opens no cluster of 2^32 - 1 keys or more (hbls_cluster_open), so CLUSTER_NO_KEY is no key's number.
CLUSTER_HD uint32_t cluster_key(uint32_t group, int64_t share_idx, uint32_t group_base, uint32_t n_groups, uint32_t n_shares,
                                bool dv = false) {
  if ((uint64_t)group < (uint64_t)group_base || (uint64_t)group >= (uint64_t)group_base + n_groups) return CLUSTER_NO_KEY;
  if (share_idx < (dv ? 0 : 1) || share_idx > (int64_t)n_shares) return CLUSTER_NO_KEY;
  const uint64_t k = (uint64_t)(group - group_base) * (1ull + n_shares) + (uint64_t)share_idx;
  return k < (uint64_t)CLUSTER_NO_KEY ? (uint32_t)k : CLUSTER_NO_KEY;
}

}  // namespace hb
