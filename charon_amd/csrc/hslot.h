// Host-side plan of hbls_slot_select_batch (hipbls.hip slot_select_host): how one duty in host
// buffers -- n partials, and per validator (aggregation group) the candidates among them -- is cut
// into one shard per device, and what each shard uploads.  Host code only (no HIP), also compiled
// into the CPU test harness (tests/native/slothostcheck.cpp, tests/test_hslot.py).
//
// The aggregation groups are sharded, in contiguous ranges (the rule of hipbls.hip fan_out).  A
// shard's items are the partials its groups list, each once, in increasing caller index, plus the
// partials no group lists whose position falls to it (item i of n -> shard i nd / n): every partial
// is verified somewhere.  A partial listed by groups of two shards is an item of both: its verdict
// is a function of its bytes, so either shard's is the call's.  Within a shard the items are put in
// verification order -- by message, in groups of at most gmax (hgroup.h), as every host Verify path
// does -- and the candidates are rebased to positions in that order.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "hgroup.h"
#include "msgtable.h"

namespace hb {

constexpr uint32_t HSLOT_NONE = 0xffffffffu;

// shards of a call over n_devices devices (fan_out: never more shards than groups, at least one)
inline size_t slot_shards(size_t n_devices, size_t n_groups) {
  return std::min(std::max<size_t>(n_devices, 1), std::max<size_t>(n_groups, 1));
}

// listed[i] != 0: some group lists partial i (candidates naming no partial, cand[j] >= n, list nothing)
inline std::vector<uint8_t> slot_listed(const uint32_t* cand, size_t n_cand, size_t n) {
  std::vector<uint8_t> listed(n, 0);
  for (size_t j = 0; j < n_cand; j++)
    if (cand[j] < n) listed[cand[j]] = 1;
  return listed;
}

struct SlotShard {
  size_t gb = 0, ge = 0;        // its aggregation groups
  bool whole = false;           // the whole call on one device: the items are the caller's n, as they are
  std::vector<size_t> items;    // else: its items' caller indices, increasing
  MsgTable tab;                 // the items' distinct messages (idx: per item, in `items` order)
  MsgGroups vg;                 // the verification groups over positions in `items`
  std::vector<uint32_t> order;  // verification order: the caller index of each of the m items
  std::vector<uint32_t> vgoff;  // the verification groups' offsets in that order (n_vgroups + 1)
  std::vector<uint32_t> cand;   // its groups' candidates as positions in that order (m: names no partial)
  std::vector<uint32_t> goff;   // its groups' offsets into cand, from 0 (ge - gb + 1)
  size_t m() const { return order.size(); }
};

// Shard k of nd (groups gb .. ge) of a call.  listed: slot_listed over the call's candidates (unused
// by a whole shard).  par: threads of the message dedup of a whole shard (0: sequential).
inline void slot_plan_shard(const uint8_t* msgs, const uint64_t* msg_off, const uint32_t* msg_len, size_t n,
                            const uint32_t* cand, const uint32_t* grp_off, size_t gb, size_t ge, size_t k, size_t nd,
                            const std::vector<uint8_t>& listed, size_t gmax, unsigned par, SlotShard& s) {
  s.gb = gb;
  s.ge = ge;
  s.whole = nd == 1;
  const size_t cb = ge > gb ? grp_off[gb] : 0, ce = ge > gb ? grp_off[ge] : 0;
  std::vector<uint32_t> pos;  // caller index -> position in `items` (then: in verification order)
  if (s.whole) {
    if (par > 1)
      dedup_messages_par(msgs, msg_off, msg_len, n, s.tab, par);
    else
      dedup_messages(msgs, msg_off, msg_len, n, nullptr, s.tab);
  } else {
    pos.assign(n, HSLOT_NONE);
    for (size_t j = cb; j < ce; j++)
      if (cand[j] < n) pos[cand[j]] = 0;
    for (size_t i = 0; i < n; i++)
      if (pos[i] != HSLOT_NONE || (!listed[i] && i * nd / n == k)) {
        pos[i] = (uint32_t)s.items.size();
        s.items.push_back(i);
      }
    dedup_messages(msgs, msg_off, msg_len, s.items.size(), s.items.data(), s.tab);
  }
  const size_t m = s.whole ? n : s.items.size();
  s.vg = group_by_message(s.tab.idx.data(), m, s.tab.len.size(), gmax);
  s.order.resize(m);
  std::vector<uint32_t> inv(m);  // position in `items` -> position in verification order
  for (size_t q = 0; q < m; q++) {
    const uint32_t it = s.vg.order[q];
    s.order[q] = s.whole ? it : (uint32_t)s.items[it];
    inv[it] = (uint32_t)q;
  }
  s.vgoff.assign(s.vg.gstart.begin(), s.vg.gstart.end());
  s.cand.resize(ce - cb);
  for (size_t j = cb; j < ce; j++) s.cand[j - cb] = cand[j] < n ? inv[s.whole ? cand[j] : pos[cand[j]]] : (uint32_t)m;
  s.goff.clear();
  if (ge > gb)
    rebase_offsets(grp_off, gb, ge, s.goff);
  else
    s.goff.push_back(0);
}

// `chosen` of a shard's groups (positions in its verification order, HSLOT_NONE past the last
// member) back to indices among the caller's partials, in place
inline void slot_chosen_to_caller(const SlotShard& s, uint32_t* chosen, size_t count) {
  for (size_t k = 0; k < count; k++)
    if (chosen[k] != HSLOT_NONE) chosen[k] = chosen[k] < s.m() ? s.order[chosen[k]] : HSLOT_NONE;
}

}  // namespace hb
