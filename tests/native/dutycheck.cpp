// TEST-ONLY harness (tests/test_duty_host.py): the storing and firing rule of a duty session
// (charon_amd/csrc/dutysel.h duty_store_group, what duty.hip's k_duty_store runs per lane), the
// one-shot matching rule it must agree with (charon_amd/csrc/tasel.h ta_select_matching) and the
// host plan of hbls_duty_add (charon_amd/csrc/hduty.h) compiled for the host CPU.  The product
// library never loads this; it is not a fallback.
#include "../../charon_amd/csrc/dutysel.h"
#include "../../charon_amd/csrc/hduty.h"
#include "../../charon_amd/csrc/tasel.h"

using namespace hb;

extern "C" {

const char* dc_build_id() { return DC_BUILD_ID; }

// One group's add: records (max_stored entries each, *count, *fired) and new partials [b, e) as
// duty_store_group takes them.  res: n_stored, n_full, fired, msg, key.
void dc_store_group(int64_t* rec_idx, uint32_t* rec_msg, uint32_t* rec_serial, uint32_t* count, uint8_t* fired,
                    uint32_t max_stored, uint32_t t, const uint8_t* vstatus, const uint32_t* msg_idx,
                    const uint32_t* serial, uint32_t n, const uint32_t* pos, const int64_t* sidx, uint32_t b, uint32_t e,
                    uint8_t* stored, uint32_t* slot, uint32_t* mslot, uint32_t* mserial, int64_t* midx, uint32_t* res) {
  const DutyRecords r{rec_idx, rec_msg, rec_serial, count, fired};
  const DutyStep s = duty_store_group(r, max_stored, t, vstatus, msg_idx, serial, n, pos, sidx, b, e, stored, slot, mslot,
                                      mserial, midx);
  res[0] = s.n_stored;
  res[1] = s.n_full;
  res[2] = s.fired;
  res[3] = s.msg;
  res[4] = s.key;
}

// ta_select_matching over candidates [b, e).  res: count, msg, state.
void dc_select_matching(const uint8_t* vstatus, const uint32_t* msg_idx, uint32_t n, const uint32_t* src,
                        const int64_t* idx, uint32_t b, uint32_t e, uint32_t t, uint32_t* chosen, int64_t* cidx,
                        uint32_t* res) {
  const TaSel r = ta_select_matching(vstatus, msg_idx, n, src, idx, b, e, t, chosen, cidx);
  res[0] = r.count;
  res[1] = r.msg;
  res[2] = r.state;
}

// The host side of a duty over n_devices devices: the shards' message tables, and the plans of the
// last add.
struct Session {
  size_t n_groups, nd;
  std::vector<DutyMsgTable> tabs;
  std::vector<std::vector<uint32_t>> items;
  std::vector<DutyShardPlan> plans;
};

void* dc_session_new(size_t n_groups, size_t n_devices) {
  Session* s = new Session;
  s->n_groups = n_groups;
  s->nd = slot_shards(n_devices, n_groups);
  s->tabs.resize(s->nd);
  return s;
}
void dc_session_free(void* p) { delete (Session*)p; }
size_t dc_session_shards(const void* p) { return ((const Session*)p)->nd; }

void dc_session_add(void* p, const uint8_t* msgs, const uint64_t* msg_off, const uint32_t* msg_len, const uint32_t* group,
                    const int64_t* share_idx, size_t n, uint32_t first_serial, size_t gmax) {
  Session& s = *(Session*)p;
  duty_route(group, n, s.n_groups, s.nd, s.items);
  s.plans.assign(s.nd, DutyShardPlan{});
  for (size_t k = 0; k < s.nd; k++)
    duty_plan_shard(msgs, msg_off, msg_len, group, share_idx, s.items[k], s.n_groups * k / s.nd,
                    s.n_groups * (k + 1) / s.nd, first_serial, gmax, s.tabs[k], s.plans[k]);
}

// out: gb, ge, items m, verification groups, messages before the add, messages after, resident
// lookups, touched groups, partials of touched groups
void dc_shard_info(const void* p, size_t k, uint64_t* out) {
  const Session& s = *(const Session*)p;
  const DutyShardPlan& q = s.plans[k];
  out[0] = s.n_groups * k / s.nd;
  out[1] = s.n_groups * (k + 1) / s.nd;
  out[2] = q.m();
  out[3] = q.n_vgroups();
  out[4] = q.msgs_before;
  out[5] = s.tabs[k].size();
  out[6] = q.resident;
  out[7] = q.n_touched();
  out[8] = q.tpos.size();
}

// order, midx, serial: m entries; vgoff: verification groups + 1; tgroup: touched; toff: touched + 1;
// tpos, tidx: partials of touched groups
void dc_shard_copy(const void* p, size_t k, uint32_t* order, uint32_t* midx, uint32_t* serial, uint32_t* vgoff,
                   uint32_t* tgroup, uint32_t* toff, uint32_t* tpos, int64_t* tidx) {
  const DutyShardPlan& q = ((const Session*)p)->plans[k];
  std::copy(q.order.begin(), q.order.end(), order);
  std::copy(q.midx.begin(), q.midx.end(), midx);
  std::copy(q.serial.begin(), q.serial.end(), serial);
  std::copy(q.vgoff.begin(), q.vgoff.end(), vgoff);
  std::copy(q.tgroup.begin(), q.tgroup.end(), tgroup);
  std::copy(q.toff.begin(), q.toff.end(), toff);
  std::copy(q.tpos.begin(), q.tpos.end(), tpos);
  std::copy(q.tidx.begin(), q.tidx.end(), tidx);
}

// message id -> its bytes in shard k's table (len bytes at the returned pointer)
const uint8_t* dc_shard_msg(const void* p, size_t k, uint32_t id, uint32_t* len) {
  const DutyMsgTable& t = ((const Session*)p)->tabs[k];
  *len = t.t.len[id];
  return t.t.bytes.data() + t.t.off[id];
}

}  // extern "C"
