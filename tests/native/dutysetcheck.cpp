// TEST-ONLY harness (tests/test_duty_sets_host.py): the host side of hbls_duty_add_sets compiled for
// the host CPU -- the validation of set_off, the plan's set ids and arrival indices and the shards'
// min-merge (charon_amd/csrc/hduty.h), the admission predicate (charon_amd/csrc/dutysel.h duty_admit,
// what duty.hip's k_duty_gate runs per lane) and, behind it, the storing rule duty_store_group over
// every touched group, as hipbls.hip's duty_add strings them together.  The verdicts are given, not
// computed: no pairing runs here.  The product library never loads this; it is not a fallback.
#include "../../charon_amd/csrc/dutysel.h"
#include "../../charon_amd/csrc/hduty.h"

#include <string.h>

using namespace hb;

namespace {

struct Shard {
  size_t gb = 0, ge = 0;
  DutyMsgTable tab;
  std::vector<int64_t> rec_idx;
  std::vector<uint32_t> rec_msg, rec_serial, count;
  std::vector<uint8_t> fired;
  DutyShardPlan plan;
  std::vector<uint32_t> set_id, set_first;
};

struct Session {
  size_t n_groups = 0, nd = 0;
  uint32_t t = 1, max_stored = 1, next_serial = 0;
  std::vector<Shard> sh;
};

}  // namespace

extern "C" {

const char* ds_build_id() { return DS_BUILD_ID; }

const char* ds_check_sets(const uint32_t* set_off, size_t n_sets, size_t n) { return duty_check_sets(set_off, n_sets, n); }
uint8_t ds_admit(uint8_t vstatus, uint32_t set_id, const uint32_t* set_first, uint32_t n_sets) {
  return duty_admit(vstatus, set_id, set_first, n_sets);
}
void ds_merge(uint32_t* merged, const uint32_t* shard, size_t n_sets) { duty_merge_set_first(merged, shard, n_sets); }

void* ds_new(size_t n_groups, size_t n_devices, uint32_t t, uint32_t max_stored) {
  Session* s = new Session;
  s->n_groups = n_groups;
  s->nd = slot_shards(n_devices, n_groups);
  s->t = t;
  s->max_stored = max_stored;
  s->sh.resize(s->nd);
  for (size_t k = 0; k < s->nd; k++) {
    Shard& h = s->sh[k];
    h.gb = n_groups * k / s->nd;
    h.ge = n_groups * (k + 1) / s->nd;
    const size_t ng = h.ge - h.gb;
    h.rec_idx.assign(ng * max_stored, 0);
    h.rec_msg.assign(ng * max_stored, 0);
    h.rec_serial.assign(ng * max_stored, 0);
    h.count.assign(ng, 0);
    h.fired.assign(ng, 0);
  }
  return s;
}
void ds_free(void* p) { delete (Session*)p; }
size_t ds_shards(const void* p) { return ((const Session*)p)->nd; }
uint32_t ds_next_serial(const void* p) { return ((const Session*)p)->next_serial; }

// One call over n partials with given verdicts; message i is the 4 bytes of msg[i].  use_sets: the
// set-atomic rule over set_off (n_sets + 1 entries); otherwise hbls_duty_add's rule.  Out, in the
// caller's order: stored (n), set_first (n_sets); fired (n at most: ascending groups) with the
// members' serials (t each); res: fired groups, partials that found their group full, first serial.
// Returns -1 (nothing done) when set_off is malformed.
int ds_add(void* p, const uint32_t* msg, const uint32_t* group, const int64_t* share_idx, const uint8_t* vstatus, size_t n,
           const uint32_t* set_off, size_t n_sets, int use_sets, uint8_t* stored, uint32_t* set_first, uint32_t* fired,
           uint32_t* chosen, uint32_t* res) {
  Session& s = *(Session*)p;
  if (use_sets && duty_check_sets(set_off, n_sets, n)) return -1;
  std::vector<uint32_t> set_of;
  if (use_sets) duty_set_ids(set_off, n_sets, n, set_of);
  std::vector<uint64_t> off(n);
  std::vector<uint32_t> len(n, 4);
  for (size_t i = 0; i < n; i++) off[i] = 4 * i;
  std::vector<std::vector<uint32_t>> items;
  duty_route(group, n, s.n_groups, s.nd, items);
  // phase one on every shard: the plan, the items' verdicts in verification order, the shard's set_first
  std::vector<std::vector<uint8_t>> vst(s.nd);
  std::vector<uint32_t> merged(use_sets ? n_sets : 0, DUTY_NONE);
  for (size_t k = 0; k < s.nd; k++) {
    Shard& h = s.sh[k];
    h.plan = DutyShardPlan{};
    duty_plan_shard((const uint8_t*)msg, off.data(), len.data(), group, share_idx, items[k], h.gb, h.ge, s.next_serial, 8,
                    h.tab, h.plan);
    const size_t m = h.plan.m();
    vst[k].resize(m);
    for (size_t q = 0; q < m; q++) vst[k][q] = vstatus[h.plan.order[q]];
    h.set_id.clear();
    h.set_first.assign(merged.size(), DUTY_NONE);
    if (!use_sets) continue;
    duty_plan_sets(set_of, h.plan, h.set_id);
    for (size_t q = 0; q < m; q++)  // k_duty_set_first, one item at a time
      if (vst[k][q] != 0 && h.set_id[q] < n_sets) h.set_first[h.set_id[q]] = std::min(h.set_first[h.set_id[q]], h.plan.order[q]);
    duty_merge_set_first(merged.data(), h.set_first.data(), n_sets);
  }
  // phase two: the gate, then the rule per touched group
  size_t nf = 0, n_full = 0;
  for (size_t i = 0; i < n; i++) stored[i] = 0;
  for (size_t k = 0; k < s.nd; k++) {
    Shard& h = s.sh[k];
    const DutyShardPlan& pl = h.plan;
    const size_t m = pl.m();
    std::vector<uint8_t> seen(vst[k]), st(m, 0);
    if (use_sets)
      for (size_t q = 0; q < m; q++) seen[q] = duty_admit(vst[k][q], h.set_id[q], merged.data(), (uint32_t)n_sets);
    std::vector<uint32_t> slot(m, DUTY_NONE), mslot(s.t), mser(s.t);
    std::vector<int64_t> midx(s.t);
    for (size_t u = 0; u < pl.n_touched(); u++) {
      const size_t g = pl.tgroup[u], r0 = g * s.max_stored;
      const DutyRecords r{h.rec_idx.data() + r0, h.rec_msg.data() + r0, h.rec_serial.data() + r0, &h.count[g], &h.fired[g]};
      const DutyStep step = duty_store_group(r, s.max_stored, s.t, seen.data(), pl.midx.data(), pl.serial.data(), (uint32_t)m,
                                             pl.tpos.data(), pl.tidx.data(), pl.toff[u], pl.toff[u + 1], st.data(), slot.data(),
                                             mslot.data(), mser.data(), midx.data());
      n_full += step.n_full;
      if (step.fired) {
        fired[nf] = (uint32_t)(h.gb + g);
        for (uint32_t j = 0; j < s.t; j++) chosen[nf * s.t + j] = mser[j];
        nf++;
      }
    }
    for (size_t q = 0; q < m; q++) stored[pl.order[q]] = st[q];
  }
  if (use_sets)
    for (size_t k = 0; k < n_sets; k++) set_first[k] = merged[k];
  res[0] = (uint32_t)nf;
  res[1] = (uint32_t)n_full;
  res[2] = s.next_serial;
  s.next_serial += (uint32_t)n;
  return 0;
}

void ds_state(const void* p, uint32_t* count, uint8_t* flag) {
  const Session& s = *(const Session*)p;
  for (const Shard& h : s.sh)
    for (size_t g = 0; g < h.ge - h.gb; g++) {
      count[h.gb + g] = h.count[g];
      flag[h.gb + g] = h.fired[g];
    }
}

// the last call's plan on shard k: its items
size_t ds_shard_m(const void* p, size_t k) { return ((const Session*)p)->sh[k].plan.m(); }
// order: the arrival index of each item in verification order; set_id: its set (m entries each, set_id only after a
// set-atomic call); set_first: the shard's own verdicts before the merge (n_sets entries)
void ds_shard_plan(const void* p, size_t k, uint32_t* order, uint32_t* set_id, uint32_t* set_first) {
  const Shard& h = ((const Session*)p)->sh[k];
  std::copy(h.plan.order.begin(), h.plan.order.end(), order);
  std::copy(h.set_id.begin(), h.set_id.end(), set_id);
  std::copy(h.set_first.begin(), h.set_first.end(), set_first);
}

}  // extern "C"
