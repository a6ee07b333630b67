// TEST-ONLY harness (tests/test_duty_first_host.py): the host side of hbls_duty_add_sets_first compiled
// for the host CPU -- the set-major plan of a shard (charon_amd/csrc/hduty.h duty_plan_shard with set
// ids, group_by_set) and the descent rule of the segmented first-error verification
// (charon_amd/csrc/dutyfirst.h: what dutyfirst.hip's kernels run per lane), walked chunk by chunk in the
// order hipbls.hip's verify_pipeline launches them.  The groups' own verdicts are given, not computed:
// no pairing runs here.  The product library never loads this; it is not a fallback.
#include "../../charon_amd/csrc/dutyfirst.h"
#include "../../charon_amd/csrc/hduty.h"

#include <string.h>

using namespace hb;

extern "C" {

const char* df_build_id() { return DF_BUILD_ID; }

// The plan of shard k of one call over n partials; message i is the 4 bytes of msg[i].  use_sets: the
// set-major plan over set_off (n_sets + 1 entries, valid); otherwise hbls_duty_add_sets' message-sorted
// plan.  Out (each sized n, offsets n + 1): order, midx, serial; vgoff and vgset (*n_vg groups; vgset only
// with use_sets); tgroup, toff (*n_t touched groups), tpos, tidx (*n_p partials).  res: m, n_vg, n_t, n_p,
// the table's size, the resident lookups.
int df_plan(const uint32_t* msg, const uint32_t* group, const int64_t* share_idx, size_t n, const uint32_t* set_off,
            size_t n_sets, int use_sets, size_t n_groups, size_t n_devices, size_t gmax, uint32_t first_serial, size_t k,
            uint32_t* order, uint32_t* midx, uint32_t* serial, uint32_t* vgoff, uint32_t* vgset, uint32_t* tgroup,
            uint32_t* toff, uint32_t* tpos, int64_t* tidx, uint64_t* res) {
  if (duty_check_sets(set_off, n_sets, n)) return -1;
  const size_t nd = slot_shards(n_devices, n_groups);
  if (k >= nd) return -2;
  std::vector<uint32_t> set_of;
  duty_set_ids(set_off, n_sets, n, set_of);
  std::vector<uint64_t> off(n);
  std::vector<uint32_t> len(n, 4);
  for (size_t i = 0; i < n; i++) off[i] = 4 * i;
  std::vector<std::vector<uint32_t>> items;
  duty_route(group, n, n_groups, nd, items);
  DutyMsgTable tab;
  DutyShardPlan p;
  duty_plan_shard((const uint8_t*)msg, off.data(), len.data(), group, share_idx, items[k], n_groups * k / nd,
                  n_groups * (k + 1) / nd, first_serial, gmax, tab, p, use_sets ? set_of.data() : nullptr);
  std::copy(p.order.begin(), p.order.end(), order);
  std::copy(p.midx.begin(), p.midx.end(), midx);
  std::copy(p.serial.begin(), p.serial.end(), serial);
  std::copy(p.vgoff.begin(), p.vgoff.end(), vgoff);
  std::copy(p.vgset.begin(), p.vgset.end(), vgset);
  std::copy(p.tgroup.begin(), p.tgroup.end(), tgroup);
  std::copy(p.toff.begin(), p.toff.end(), toff);
  std::copy(p.tpos.begin(), p.tpos.end(), tpos);
  std::copy(p.tidx.begin(), p.tidx.end(), tidx);
  res[0] = p.m();
  res[1] = p.n_vgroups();
  res[2] = p.n_touched();
  res[3] = p.tpos.size();
  res[4] = tab.size();
  res[5] = p.resident;
  return (use_sets ? p.vgset.size() == p.n_vgroups() : p.vgset.empty()) ? 0 : -3;
}

// The rule over n_groups groups in chunks of gcap, batches of fb within a chunk: ready[g] / fail[g] say
// whether group g is READY and whether its own check would fail; a batch fails when a READY group of it
// does.  Per chunk, as the device does: every vote (seg_votes) folded into sfirst[2k], then every
// verdict; behind the last chunk the segments' first failing groups into sfirst[2k + 1], then per group
// whether its items would be left unchecked.  Out: gver (n_groups: 0 pass, 3 own check failed, 0x80
// unchecked, 0x81 not ready), sfirst (2 n_seg, preset here), unchecked (n_groups), descended (n_groups:
// the group was checked alone).
void df_rule(size_t n_groups, size_t gcap, uint32_t fb, const uint8_t* ready, const uint8_t* fail, const uint32_t* gseg,
             uint32_t n_seg, uint8_t* gver, uint32_t* sfirst, uint8_t* unchecked, uint8_t* descended) {
  for (size_t j = 0; j < 2 * (size_t)n_seg; j++) sfirst[j] = SEG_NONE;
  for (size_t g0 = 0; g0 < n_groups; g0 += gcap) {
    const uint32_t ng = (uint32_t)std::min(gcap, n_groups - g0);
    std::vector<uint8_t> bver((ng + fb - 1) / fb, 0);
    for (uint32_t lg = 0; lg < ng; lg++)
      if (ready[g0 + lg] && fail[g0 + lg]) bver[lg / fb] = 1;
    for (uint32_t lg = 0; lg < ng; lg++) {
      const uint32_t g = (uint32_t)g0 + lg, key = seg_batch_key((uint32_t)g0, lg, fb);
      if (ready[g] && bver[lg / fb] && seg_votes(gseg, n_seg, key, g)) sfirst[2 * gseg[g]] = std::min(sfirst[2 * gseg[g]], key);
    }
    for (uint32_t lg = 0; lg < ng; lg++) {
      const uint32_t g = (uint32_t)g0 + lg;
      const uint8_t v = seg_group_verdict(ready[g] != 0, bver[lg / fb] != 0, gseg, n_seg, sfirst,
                                          seg_batch_key((uint32_t)g0, lg, fb), g);
      descended[g] = v == SEG_DESCEND;
      gver[g] = v == SEG_DESCEND ? (fail[g] ? 3 : 0) : v;
    }
  }
  for (uint32_t g = 0; g < n_groups; g++)
    if (gver[g] != SEG_PASS && gver[g] < SEG_UNCHECKED && gseg[g] < n_seg)
      sfirst[2 * gseg[g] + 1] = std::min(sfirst[2 * gseg[g] + 1], g);
  for (uint32_t g = 0; g < n_groups; g++)
    unchecked[g] = gver[g] != SEG_PASS && seg_item_unchecked(gver[g], gseg, n_seg, sfirst, g);
}

}  // extern "C"
