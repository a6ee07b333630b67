// TEST-ONLY harness (tests/test_hslot.py): the host plan of hbls_slot_select_batch
// (charon_amd/csrc/hslot.h) and its matching rule (charon_amd/csrc/tasel.h ta_select_matching, what
// threshold.hip's k_ta_select runs per lane in that mode) compiled for the host CPU.  The product
// library never loads this; it is not a fallback.
#include "../../charon_amd/csrc/hslot.h"
#include "../../charon_amd/csrc/tasel.h"

using namespace hb;

extern "C" {

const char* hs_build_id() { return HS_BUILD_ID; }

// One group: candidates [b, e).  chosen / cidx: t entries each.  res: count, key, msg, state, shifted.
// mode: TASEL_MODE_FIRST (ta_select) or TASEL_MODE_MATCHING.
void hs_select(uint32_t mode, const uint8_t* vstatus, const uint32_t* msg_idx, uint32_t n, const uint32_t* src,
               const int64_t* idx, uint32_t b, uint32_t e, uint32_t t, uint32_t* chosen, int64_t* cidx, uint32_t* res) {
  const TaSel r = mode == TASEL_MODE_MATCHING ? ta_select_matching(vstatus, msg_idx, n, src, idx, b, e, t, chosen, cidx)
                                              : ta_select(vstatus, msg_idx, n, src, idx, b, e, t, chosen, cidx);
  res[0] = r.count;
  res[1] = r.key;
  res[2] = r.msg;
  res[3] = r.state;
  res[4] = r.shifted;
}

// The plan of a call over n_devices devices: every shard, as slot_select_host builds them.
struct Plan {
  std::vector<SlotShard> shards;
};

void* hs_plan_new(const uint8_t* msgs, const uint64_t* msg_off, const uint32_t* msg_len, size_t n, const uint32_t* cand,
                  const uint32_t* grp_off, size_t n_groups, size_t n_devices, size_t gmax) {
  Plan* p = new Plan;
  const size_t nd = slot_shards(n_devices, n_groups);
  std::vector<uint8_t> listed;
  if (nd > 1) listed = slot_listed(cand + grp_off[0], grp_off[n_groups] - grp_off[0], n);
  p->shards.resize(nd);
  for (size_t k = 0; k < nd; k++)
    slot_plan_shard(msgs, msg_off, msg_len, n, cand, grp_off, n_groups * k / nd, n_groups * (k + 1) / nd, k, nd, listed,
                    gmax, 0, p->shards[k]);
  return p;
}
void hs_plan_free(void* p) { delete (Plan*)p; }
size_t hs_plan_shards(const void* p) { return ((const Plan*)p)->shards.size(); }

// out: gb, ge, whole, items m, verification groups, distinct messages, candidates
void hs_shard_info(const void* p, size_t k, uint64_t* out) {
  const SlotShard& s = ((const Plan*)p)->shards[k];
  out[0] = s.gb;
  out[1] = s.ge;
  out[2] = s.whole ? 1 : 0;
  out[3] = s.m();
  out[4] = s.vg.n_groups();
  out[5] = s.tab.len.size();
  out[6] = s.cand.size();
}

// order, midx: m entries; vgoff: verification groups + 1; cand: candidates; goff: ge - gb + 1;
// moff, mlen: distinct messages; mbytes: the table's bytes (hs_shard_msg_bytes of them)
size_t hs_shard_msg_bytes(const void* p, size_t k) { return ((const Plan*)p)->shards[k].tab.bytes.size(); }
void hs_shard_copy(const void* p, size_t k, uint32_t* order, uint32_t* midx, uint32_t* vgoff, uint32_t* cand,
                   uint32_t* goff, uint64_t* moff, uint32_t* mlen, uint8_t* mbytes) {
  const SlotShard& s = ((const Plan*)p)->shards[k];
  std::copy(s.order.begin(), s.order.end(), order);
  std::copy(s.vg.midx.begin(), s.vg.midx.end(), midx);
  std::copy(s.vgoff.begin(), s.vgoff.end(), vgoff);
  std::copy(s.cand.begin(), s.cand.end(), cand);
  std::copy(s.goff.begin(), s.goff.end(), goff);
  std::copy(s.tab.off.begin(), s.tab.off.end(), moff);
  std::copy(s.tab.len.begin(), s.tab.len.end(), mlen);
  std::copy(s.tab.bytes.begin(), s.tab.bytes.end(), mbytes);
}

// chosen (count entries: positions in shard k's verification order) back to caller indices, in place
void hs_chosen_to_caller(const void* p, size_t k, uint32_t* chosen, size_t count) {
  slot_chosen_to_caller(((const Plan*)p)->shards[k], chosen, count);
}

}  // extern "C"
