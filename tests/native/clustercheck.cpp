// TEST-ONLY harness (tests/test_cluster_host.py): the key rule of a cluster handle compiled for the
// host CPU -- charon_amd/csrc/cluster.h cluster_key, the one function cluster.hip's k_cluster_keys runs
// per item and hipbls.hip counts hbls_cluster_stats with.  The product library never loads this; it is
// not a fallback.
#include "../../charon_amd/csrc/cluster.h"

#include <stddef.h>

using namespace hb;

extern "C" {

const char* cc_build_id() { return CC_BUILD_ID; }

uint32_t cc_no_key() { return CLUSTER_NO_KEY; }
uint32_t cc_max_shares() { return CLUSTER_MAX_SHARES; }

// out[i]: the key number of (group[i], share_idx[i]) in a shard of n_groups groups from group_base
void cc_keys(const uint32_t* group, const int64_t* share_idx, size_t n, uint32_t group_base, uint32_t n_groups,
             uint32_t n_shares, int dv, uint32_t* out) {
  for (size_t i = 0; i < n; i++) out[i] = cluster_key(group[i], share_idx[i], group_base, n_groups, n_shares, dv != 0);
}

}  // extern "C"
