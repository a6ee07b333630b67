// The selection rule of hbls_cluster_verify_aggregate: which entries of a cluster's rows a (share_mask,
// with_dv) pair sums, and which pairs are call errors.  A row is cluster.h's: entry 0 the validator's DV
// key, entry j (1 .. n_shares) its pubshare of share index j.  Bit j - 1 of share_mask selects entry j,
// with_dv (0 or 1) entry 0; the same entries of every row.  cluster/lock.go:185 and dkg/dkg.go:595 (one
// tbls.VerifyAggregate over every validator's every pubshare) are the full mask with no DV key.
//
// ONE place holds the rule.  No HIP in here: cluster.hip's k_cluster_row_sum asks cluster_sel_entry per
// entry of its row, hipbls.hip refuses a call with cluster_sel_valid and counts
// hbls_cluster_verify_stats with cluster_sel_count, and the CPU harness tests/native/more/clusterselcheck.cpp
// compiles the same functions for tests/test_cluster_sel_host.py.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CLUSTERSEL_HD __host__ __device__ inline
#else
#define CLUSTERSEL_HD inline
#endif

namespace hb {

constexpr uint32_t CLUSTERSEL_MAX_SHARES = 64;  // cluster.h CLUSTER_MAX_SHARES: a mask bit per share index

// The mask of every share of a row of n_shares (1 .. 64) pubshares; 0 for any other n_shares.
CLUSTERSEL_HD uint64_t cluster_sel_all(uint32_t n_shares) {
  if (n_shares < 1 || n_shares > CLUSTERSEL_MAX_SHARES) return 0;
  return n_shares == 64 ? ~0ull : (1ull << n_shares) - 1;  // (no shift by the word's width)
}

// A call error unless n_shares is a cluster's, no mask bit lies at or above n_shares and with_dv is 0 or 1.
// The empty selection is valid (an empty group never verifies: that is a status, not an error).
CLUSTERSEL_HD bool cluster_sel_valid(uint64_t share_mask, uint32_t with_dv, uint32_t n_shares) {
  if (n_shares < 1 || n_shares > CLUSTERSEL_MAX_SHARES) return false;
  return (share_mask & ~cluster_sel_all(n_shares)) == 0 && with_dv <= 1;
}

// Is entry j of a row selected?  Entry 0 by with_dv, entry j in 1 .. 64 by bit j - 1; no other entry is.
CLUSTERSEL_HD bool cluster_sel_entry(uint32_t j, uint64_t share_mask, uint32_t with_dv) {
  if (j == 0) return with_dv == 1;
  if (j > CLUSTERSEL_MAX_SHARES) return false;
  return ((share_mask >> (j - 1)) & 1) != 0;
}

// The selected entries of one row of a valid pair: the mask's set bits and the DV key.
CLUSTERSEL_HD uint32_t cluster_sel_count(uint64_t share_mask, uint32_t with_dv) {
  uint32_t c = with_dv == 1 ? 1 : 0;
  for (; share_mask; share_mask &= share_mask - 1) c++;
  return c;
}

}  // namespace hb
