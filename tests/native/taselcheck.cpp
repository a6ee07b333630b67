// TEST-ONLY harness (tests/test_tasel_host.py): the verified-member selection rule and its class key
// (charon_amd/csrc/tasel.h, what threshold.hip's k_ta_select runs per lane) compiled for the host
// CPU.  The product library never loads this; it is not a fallback.
#include "../../charon_amd/csrc/tasel.h"

using namespace hb;

extern "C" {

const char* ts_build_id() { return TS_BUILD_ID; }

uint32_t ts_max() { return TASEL_MAX; }
uint32_t ts_key_none() { return TASEL_KEY_NONE; }

// One group: candidates [b, e).  chosen / cidx: t entries each.  res: count, key, msg, state, shifted.
void ts_select(const uint8_t* vstatus, const uint32_t* msg_idx, uint32_t n, const uint32_t* src, const int64_t* idx,
               uint32_t b, uint32_t e, uint32_t t, uint32_t* chosen, int64_t* cidx, uint32_t* res) {
  const TaSel r = ta_select(vstatus, msg_idx, n, src, idx, b, e, t, chosen, cidx);
  res[0] = r.count;
  res[1] = r.key;
  res[2] = r.msg;
  res[3] = r.state;
  res[4] = r.shifted;
}

}  // extern "C"
