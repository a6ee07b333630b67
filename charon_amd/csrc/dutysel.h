// The storing and firing rule of a duty session (hbls_duty_add): what one arriving set does to one
// validator's resident records.  The rule is the reference node's, applied as the partials arrive
// (parsigex.go:93-98 verifies a partial before it is stored; parsigdb/memory.go:149-160 drops a
// second partial under a stored share index, whatever its root; memory.go:197-225 fires once
// `threshold` stored partials match): tasel.h's ta_select_matching over a whole candidate list, cut
// into adds.  The resident records are the state: no earlier add is walked again, and every walk is
// over at most max_stored records.
//
// No HIP in here: duty.hip's k_duty_store calls duty_store_group once per lane, and the CPU harness
// tests/native/dutycheck.cpp compiles the same function for tests/test_duty_host.py.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DUTYSEL_HD __host__ __device__ inline
#else
#define DUTYSEL_HD inline
#endif

namespace hb {

constexpr uint32_t DUTY_MAX_T = 16;            // members per group (tasel.h TASEL_MAX)
constexpr uint32_t DUTY_MAX_STORED = 64;       // stored partials per group, at most
constexpr uint32_t DUTY_NONE = 0xffffffffu;    // no destination slot / no group

// hbls_duty_add_sets: a peer's set is stored whole or not at all (parsigex.go:93-98 returns at the
// first partial of a set that fails, before any subscriber sees the set).  set_first[k] is the
// smallest arrival index of set k whose verification failed, DUTY_NONE when every partial of the
// set verified.  The admission predicate: the status byte the storing rule sees for a partial of
// set `set_id` -- its own verdict when that is a failure, DUTY_SET_REJECTED when it verified but its
// set did not, 0 (admitted) otherwise.  A set id outside the call's sets admits nothing and is never
// an address.  duty.hip's k_duty_gate and the CPU harness tests/native/dutysetcheck.cpp both
// compile this one function.
constexpr uint8_t DUTY_SET_REJECTED = 0xff;
DUTYSEL_HD uint8_t duty_admit(uint8_t vstatus, uint32_t set_id, const uint32_t* set_first, uint32_t n_sets) {
  if (vstatus != 0) return vstatus;
  if (set_id >= n_sets) return DUTY_SET_REJECTED;
  return set_first[set_id] != DUTY_NONE ? DUTY_SET_REJECTED : (uint8_t)0;
}

// One group's resident records: slot k < *count holds the k-th stored partial's share index,
// message id and serial; *fired != 0 closes the group.
struct DutyRecords {
  int64_t* idx;
  uint32_t* msg;
  uint32_t* serial;
  uint32_t* count;
  uint8_t* fired;
};

struct DutyStep {
  uint32_t n_stored;  // partials this add stored
  uint32_t n_full;    // verified partials under a new share index that found the open group full
  uint32_t fired;     // the group fired in this add
  uint32_t msg;       // then: the members' message
  uint32_t key;       // then: the class key of their share indices (16 bits, as tasel.h ta_class_key)
};

// The new partials of one group, in arrival order: partial j of [b, e) is item pos[j] of the add
// (of n, with verification status vstatus[pos[j]], message id msg_idx[pos[j]] and serial
// serial[pos[j]]) under share index sidx[j].  Writes stored[pos[j]] (0 / 1) and slot[pos[j]] (the
// record slot it took, DUTY_NONE when not stored) of every partial walked; a position >= n is
// skipped.  When the group fires, mslot / mserial / midx get the t members' record slots, serials
// and share indices in stored order.  1 <= t <= DUTY_MAX_T, 1 <= max_stored <= DUTY_MAX_STORED.
DUTYSEL_HD DutyStep duty_store_group(const DutyRecords& r, uint32_t max_stored, uint32_t t, const uint8_t* vstatus,
                                     const uint32_t* msg_idx, const uint32_t* serial, uint32_t n, const uint32_t* pos,
                                     const int64_t* sidx, uint32_t b, uint32_t e, uint8_t* stored, uint32_t* slot,
                                     uint32_t* mslot, uint32_t* mserial, int64_t* midx) {
  DutyStep s;
  s.n_stored = s.n_full = s.fired = s.msg = s.key = 0;
  uint32_t count = *r.count < max_stored ? *r.count : max_stored;
  bool closed = *r.fired != 0;
  for (uint32_t j = b; j < e; j++) {
    const uint32_t q = pos[j];
    if (q >= n) continue;
    stored[q] = 0;
    slot[q] = DUTY_NONE;
    if (closed || vstatus[q] != 0) continue;
    const int64_t x = sidx[j];
    bool dup = false;
    for (uint32_t k = 0; k < count; k++) dup = dup || r.idx[k] == x;
    if (dup) continue;
    if (count == max_stored) {
      s.n_full++;
      continue;
    }
    const uint32_t m = msg_idx[q];
    r.idx[count] = x;
    r.msg[count] = m;
    r.serial[count] = serial[q];
    stored[q] = 1;
    slot[q] = count;
    count++;
    s.n_stored++;
    uint32_t c = 0;
    for (uint32_t k = 0; k < count; k++) c += r.msg[k] == m ? 1u : 0u;
    if (c < t) continue;
    // exactly t: the store before this one left the message below t, or the group had fired
    closed = true;
    s.fired = 1;
    s.msg = m;
    uint32_t f = 0;
    for (uint32_t k = 0; k < count && f < t; k++) {
      if (r.msg[k] != m) continue;
      mslot[f] = k;
      mserial[f] = r.serial[k];
      midx[f] = r.idx[k];
      s.key ^= 1u << ((uint32_t)r.idx[k] & 15u);
      f++;
    }
  }
  *r.count = count;
  if (closed) *r.fired = 1;
  return s;
}

}  // namespace hb
