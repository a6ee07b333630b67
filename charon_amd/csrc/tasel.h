// Verified-member selection of hbls_slot_select_device: which of a group's candidates are
// aggregated, and the class key the groups are ordered by before the aggregation.  The rule is the
// reference node's (parsigex.go:93-98 verifies a partial before it is stored, parsigdb/memory.go:
// 198-225 fires once `threshold` stored partials match, sigagg.go:90-97 keys them by share index):
// a group's members are its first t candidates, in the caller's order, whose verification status is
// OK and whose share index differs from every member already chosen.
//
// No HIP in here: threshold.hip's k_ta_select calls ta_select once per lane, and the CPU harness
// tests/native/taselcheck.cpp compiles the same function for tests/test_tasel_host.py.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TASEL_HD __host__ __device__ inline
#else
#define TASEL_HD inline
#endif

namespace hb {

constexpr uint32_t TASEL_MAX = 16;            // members per group (ta_small.h TA_SMALL_MAX)
constexpr uint32_t TASEL_NONE = 0xffffffffu;  // `chosen` past the last member
// class keys are 16 bits; groups without an aggregate sort behind every one of them
constexpr uint32_t TASEL_KEYS = 0x10001u, TASEL_KEY_NONE = 0x10000u;
enum : uint8_t { TASEL_OK = 0, TASEL_FEW = 1, TASEL_MIXED = 2 };

struct TaSel {
  uint32_t count;   // members found (<= t)
  uint32_t key;     // class key (below)
  uint32_t msg;     // the candidates' message (the first candidate's; 0 without one)
  uint8_t state;    // TASEL_OK: t members over one message; TASEL_MIXED wins over TASEL_FEW
  uint8_t shifted;  // t members found, and they are not candidates 0 .. t - 1
};

// The class key of a set of chosen candidate positions: their bit mask, taken as is for groups of
// up to 16 candidates (equal keys <=> equal positions) and XOR-folded to 16 bits for wider ones
// (a collision puts two classes side by side: it costs speed, never a result).
TASEL_HD uint32_t ta_class_key(uint32_t key, uint32_t pos) { return key ^ (1u << (pos & 15u)); }

// Candidates [b, e) of one group: candidate j is partial src[j] (of n, with verification status
// vstatus[src[j]] and message msg_idx[src[j]]) under share index idx[j].  Writes t entries each of
// chosen (indices among the n partials, TASEL_NONE past the last member) and cidx (their share
// indices, 0 past the last).  A candidate naming no partial (src[j] >= n) counts as not verified.
// 1 <= t <= TASEL_MAX.
TASEL_HD TaSel ta_select(const uint8_t* vstatus, const uint32_t* msg_idx, uint32_t n, const uint32_t* src,
                         const int64_t* idx, uint32_t b, uint32_t e, uint32_t t, uint32_t* chosen, int64_t* cidx) {
  TaSel r;
  r.count = 0;
  r.key = 0;
  r.msg = 0;
  r.state = TASEL_OK;
  r.shifted = 0;
  bool have_msg = false, mixed = false;
  uint32_t last = 0;
  for (uint32_t j = b; j < e; j++) {
    const uint32_t p = src[j];
    if (p >= n) continue;
    const uint32_t m = msg_idx[p];
    if (!have_msg) {
      r.msg = m;
      have_msg = true;
    } else if (m != r.msg) {
      mixed = true;
    }
    if (r.count == t || vstatus[p] != 0) continue;
    const int64_t x = idx[j];
    bool dup = false;
    for (uint32_t k = 0; k < r.count; k++) dup = dup || cidx[k] == x;
    if (dup) continue;
    chosen[r.count] = p;
    cidx[r.count] = x;
    r.count++;
    last = j - b;
    r.key = ta_class_key(r.key, last);
  }
  for (uint32_t k = r.count; k < t; k++) {
    chosen[k] = TASEL_NONE;
    cidx[k] = 0;
  }
  if (mixed) r.state = TASEL_MIXED;
  else if (r.count < t) r.state = TASEL_FEW;
  // the members are in candidate order: they are the first t exactly when the last one is t - 1
  r.shifted = (r.count == t && last != t - 1) ? 1 : 0;
  if (r.state != TASEL_OK) r.key = TASEL_KEY_NONE;
  return r;
}

// How k_ta_select picks a group's members: ta_select, or ta_select_matching below.
enum : uint32_t { TASEL_MODE_FIRST = 0, TASEL_MODE_MATCHING = 1 };

// Whether candidate j of [b, e) is stored, the reference's parsigdb/memory.go:149-160: it is verified
// and no earlier verified candidate has its share index (a second partial under a stored share index
// is dropped whatever its root).
TASEL_HD bool ta_stored(const uint8_t* vstatus, uint32_t n, const uint32_t* src, const int64_t* idx, uint32_t b,
                        uint32_t j) {
  if (src[j] >= n || vstatus[src[j]] != 0) return false;
  for (uint32_t i = b; i < j; i++)
    if (src[i] < n && vstatus[src[i]] == 0 && idx[i] == idx[j]) return false;
  return true;
}

// The reference's matching rule (parsigdb/memory.go:197-225 getThresholdMatching) for candidates
// that may span several messages; arguments and outputs as ta_select.  Walking the candidates in
// order, the stored ones are counted per message; the first message to hold t of them wins, and
// those t, in candidate order, are the members (TaSel::msg is their message; key and shifted come
// from their positions as in ta_select).  Candidates over one message give ta_select's result,
// by calling it: also below t, where its count and chosen report the stored candidates found.
// Candidates over several messages of which none holds t give no members: TASEL_FEW, count 0,
// chosen all TASEL_NONE.  TASEL_MIXED never arises.  A lane keeps no table of what it has seen: it
// walks its candidates again (cubic in their number at worst, a handful in practice), so their
// number has no bound.
TASEL_HD TaSel ta_select_matching(const uint8_t* vstatus, const uint32_t* msg_idx, uint32_t n, const uint32_t* src,
                                  const int64_t* idx, uint32_t b, uint32_t e, uint32_t t, uint32_t* chosen,
                                  int64_t* cidx) {
  bool have_msg = false, several = false;
  uint32_t m0 = 0;
  for (uint32_t j = b; j < e; j++) {
    if (src[j] >= n) continue;
    const uint32_t m = msg_idx[src[j]];
    if (!have_msg) {
      m0 = m;
      have_msg = true;
    } else if (m != m0) {
      several = true;
    }
  }
  if (!several) return ta_select(vstatus, msg_idx, n, src, idx, b, e, t, chosen, cidx);
  TaSel r;
  r.count = 0;
  r.key = TASEL_KEY_NONE;
  r.msg = m0;
  r.state = TASEL_FEW;
  r.shifted = 0;
  for (uint32_t k = 0; k < t; k++) {
    chosen[k] = TASEL_NONE;
    cidx[k] = 0;
  }
  for (uint32_t j = b; j < e; j++) {
    if (!ta_stored(vstatus, n, src, idx, b, j)) continue;
    const uint32_t m = msg_idx[src[j]];
    // the stored candidates over m up to j: the message is compared first, it is the cheap test
    uint32_t c = 1;
    for (uint32_t i = b; i < j && c < t; i++)
      if (src[i] < n && msg_idx[src[i]] == m && ta_stored(vstatus, n, src, idx, b, i)) c++;
    if (c < t) continue;
    uint32_t last = 0;
    r.key = 0;
    for (uint32_t i = b; i <= j && r.count < t; i++) {  // exactly t: an earlier t-th would have ended the walk
      if (src[i] >= n || msg_idx[src[i]] != m || !ta_stored(vstatus, n, src, idx, b, i)) continue;
      chosen[r.count] = src[i];
      cidx[r.count] = idx[i];
      r.count++;
      last = i - b;
      r.key = ta_class_key(r.key, last);
    }
    r.msg = m;
    r.state = TASEL_OK;
    r.shifted = last != t - 1 ? 1 : 0;
    return r;
  }
  return r;
}

}  // namespace hb
