// TEST-ONLY harness (tests/test_subgroup_batch_host.py): the digits of the batched G2 subgroup test
// (charon_amd/csrc/subgbatch.h, what msm.hip's k_subg_digits and k_subg_class run per lane) and the
// plan's decision for it (vplan.h) compiled for the host CPU.  The product library never loads
// this; it is not a fallback.
#include "../../charon_amd/csrc/subgbatch.h"
#include "../../charon_amd/csrc/vplan.h"

using namespace hb;

extern "C" {

const char* sg_build_id() { return SG_BUILD_ID; }

// base, digits, windows, range, keys, sums, classes, class size
void sg_constants(uint32_t* out) {
  const uint32_t c[8] = {SG_BASE, SG_DIGITS, SG_WINDOWS, SG_RANGE, SG_KEYS, SG_SUMS, SG_CLASSES, SG_CLASS_SIZE};
  for (int k = 0; k < 8; k++) out[k] = c[k];
}
uint32_t sg_window_of(uint32_t u) { return sg_window(u); }
uint32_t sg_digit_of(uint32_t d, uint32_t j) { return sg_digit(d, j); }
uint32_t sg_class_member_of(uint32_t j, uint32_t c, uint32_t m) { return sg_class_member(j, c, m); }
void sg_windows_of(const uint32_t* key, uint32_t item, uint32_t* d) { sg_windows(key, item, d); }

// The largest number of 32-bit words that sg_window sends to one value, exactly: the map is
// monotone, so value d's preimage is [lo_d, lo_(d+1)) with lo_d = ceil(d 2^32 / 13^4); each
// boundary is confirmed through sg_window itself.  Returns 0 if a boundary is not where computed.
uint64_t sg_max_multiplicity() {
  uint64_t best = 0, prev = 0;
  for (uint64_t d = 1; d <= SG_RANGE; d++) {
    const uint64_t lo = ((d << 32) + SG_RANGE - 1) / SG_RANGE;  // first u of value d (2^32 for d = 13^4)
    if (sg_window((uint32_t)(lo - 1)) != d - 1) return 0;
    if (d < SG_RANGE && sg_window((uint32_t)lo) != d) return 0;
    if (lo - prev > best) best = lo - prev;
    prev = lo;
  }
  return prev == (1ull << 32) ? best : 0;
}

// in: n, own_sigs, subg_failed, adaptive, subg_batch_min (the other fields: a slot-sized grouped
// call).  out: subg_batch, subg_skip.  Returns 0, or 1 if the plan is refused.
int sg_plan(const uint64_t* in, uint64_t* out) {
  VerifyShape sh{};
  sh.n = (size_t)in[0];
  sh.n_groups = std::max<size_t>(1, sh.n / 4);
  sh.grouped = true;
  sh.n_cu = 256;
  sh.own_sigs = in[1] != 0;
  sh.subg_failed = in[2] != 0;
  VerifyKnobs k{65536, 65536, 128, 32768, 65536, in[3] != 0};
  k.subg_batch_min = (size_t)in[4];
  VerifyPlan p{};
  if (verify_plan(sh, k, p)) return 1;
  out[0] = p.subg_batch;
  out[1] = p.subg_skip;
  return 0;
}

}  // extern "C"
