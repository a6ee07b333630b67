// TEST-ONLY harness (tests/test_lock_check_host.py): the rule of hbls_cluster_check compiled for the host
// CPU -- charon_amd/csrc/lockcheck.h's signed binomial coefficients, their bit length and the plan
// lockcheck.hip's k_lock_check takes as its argument and hipbls.hip validates a threshold with.  The
// product library never loads this; it is not a fallback.
#include "../../charon_amd/csrc/lockcheck.h"

#include <stddef.h>

using namespace hb;

extern "C" {

const char* lk_build_id() { return LK_BUILD_ID; }

uint32_t lk_max_t() { return LOCK_MAX_T; }

// c: t + 1 words (untouched when the threshold is refused) -> 1 / 0
int lk_coeffs(uint32_t t, int64_t* c) { return lock_coeffs(t, c) ? 1 : 0; }

uint32_t lk_bits(uint32_t t) { return lock_bits(t); }

// out (untouched when the pair is refused): n_shares, t, windows, bits, then c[0 .. 64] -> 1 / 0
int lk_plan(uint32_t n_shares, uint32_t t, int64_t* out) {
  LockPlan p;
  if (!lock_plan(n_shares, t, p)) return 0;
  out[0] = p.n_shares;
  out[1] = p.t;
  out[2] = p.windows;
  out[3] = p.bits;
  for (uint32_t i = 0; i <= LOCK_MAX_T; i++) out[4 + i] = p.c[i];
  return 1;
}

}  // extern "C"
