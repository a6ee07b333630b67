// TEST-ONLY harness (tests/test_cluster_sel_host.py): the selection rule of hbls_cluster_verify_aggregate
// compiled for the host CPU -- charon_amd/csrc/clustersel.h's functions, the ones cluster.hip's
// k_cluster_row_sum selects a row's entries with and hipbls.hip refuses and counts a call with.  The
// product library never loads this; it is not a fallback.
#include "../../../charon_amd/csrc/clustersel.h"

using namespace hb;

extern "C" {

const char* cs_build_id() { return CS_BUILD_ID; }

uint32_t cs_max_shares() { return CLUSTERSEL_MAX_SHARES; }

uint64_t cs_all(uint32_t n_shares) { return cluster_sel_all(n_shares); }

int cs_valid(uint64_t share_mask, uint32_t with_dv, uint32_t n_shares) {
  return cluster_sel_valid(share_mask, with_dv, n_shares) ? 1 : 0;
}

int cs_entry(uint32_t j, uint64_t share_mask, uint32_t with_dv) { return cluster_sel_entry(j, share_mask, with_dv) ? 1 : 0; }

uint32_t cs_count(uint64_t share_mask, uint32_t with_dv) { return cluster_sel_count(share_mask, with_dv); }

}  // extern "C"
