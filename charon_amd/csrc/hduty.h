// Host-side plan of a duty session (hipbls.hip hbls_duty_add): the message table a shard keeps for
// the duty's lifetime, how one arriving set is routed to the shards, and what each shard uploads.
// Host code only (no HIP), also compiled into the CPU test harness (tests/native/dutycheck.cpp,
// tests/test_duty_host.py).
//
// The duty's groups (validators) are sharded in contiguous ranges, by the rule of hslot.h and
// hipbls.hip fan_out: shard k of nd owns groups n_groups k / nd .. n_groups (k + 1) / nd.  A
// partial goes to the shard that owns its group; a partial of no group (group[i] >= n_groups:
// verify only) goes to shard i nd / n.  Within a shard the items are put in verification order --
// by message, in groups of at most gmax (hgroup.h), as every host Verify path does -- and the
// groups the add touches are listed in CSR form over positions in that order.  hbls_duty_add_sets_first
// verifies in set-major order instead (group_by_set): the sets as they came, each group inside one set.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "hgroup.h"
#include "hslot.h"
#include "msgtable.h"

namespace hb {

// A growing message table: bytes -> duty-wide message id (per shard), an open-addressing map over
// the appended blob (msgtable.h's layout: bytes / off / len; MsgTable::idx is unused).  Ids are
// given in order of first appearance and never change.
struct DutyMsgTable {
  MsgTable t;
  std::vector<uint64_t> hash;   // per id
  std::vector<uint32_t> slot;   // id or 0xffffffff
  size_t size() const { return t.len.size(); }
  uint32_t lookup(const uint8_t* m, uint32_t l, bool* is_new) {
    if (slot.empty()) slot.assign(1024, 0xffffffffu);
    const uint64_t hv = msg_hash(m, l);
    size_t cap = slot.size(), h = (size_t)hv & (cap - 1);
    for (;;) {
      const uint32_t id = slot[h];
      if (id == 0xffffffffu) break;
      if (hash[id] == hv && t.len[id] == l && msg_eq(t.bytes.data() + t.off[id], m, l)) {
        *is_new = false;
        return id;
      }
      h = (h + 1) & (cap - 1);
    }
    const uint32_t id = (uint32_t)size();
    hash.push_back(hv);
    t.off.push_back(t.bytes.size());
    t.len.push_back(l);
    t.bytes.insert(t.bytes.end(), m, m + l);
    if (2 * hash.size() > cap) {  // grow: re-insert every id by its hash
      cap *= 2;
      slot.assign(cap, 0xffffffffu);
      for (uint32_t q = 0; q < (uint32_t)hash.size(); q++) {
        size_t g = (size_t)hash[q] & (cap - 1);
        while (slot[g] != 0xffffffffu) g = (g + 1) & (cap - 1);
        slot[g] = q;
      }
    } else {
      slot[h] = id;
    }
    *is_new = true;
    return id;
  }
};

// the shard that owns group g of n_groups over nd shards (ranges n_groups k / nd)
inline size_t duty_shard_of_group(size_t g, size_t n_groups, size_t nd) {
  size_t k = g * nd / n_groups;
  while (k + 1 < nd && n_groups * (k + 1) / nd <= g) k++;
  while (k > 0 && n_groups * k / nd > g) k--;
  return k;
}

// Route the n partials of an add: items[k] gets shard k's partials (caller indices, increasing).
inline void duty_route(const uint32_t* group, size_t n, size_t n_groups, size_t nd,
                       std::vector<std::vector<uint32_t>>& items) {
  items.assign(nd, {});
  for (size_t i = 0; i < n; i++) {
    const size_t k = group[i] < n_groups ? duty_shard_of_group(group[i], n_groups, nd) : i * nd / n;
    items[k].push_back((uint32_t)i);
  }
}

struct DutyShardPlan {
  std::vector<uint32_t> order;   // verification order: the caller index of each of the m items
  std::vector<uint32_t> midx;    // each item's duty-wide message id, in that order
  std::vector<uint32_t> vgoff;   // the verification groups' offsets in that order (n_vgroups + 1)
  std::vector<uint32_t> vgset;   // set-major plans (hbls_duty_add_sets_first) only: each verification group's set
  std::vector<uint32_t> serial;  // each item's serial, in that order
  size_t msgs_before = 0;        // the table's size before this add: ids from there on are new to the shard
  size_t resident = 0;           // message lookups answered from the table
  // the groups this add touches, ascending: tgroup (local: group - gb), and partials
  // [toff[u], toff[u + 1]) of tpos (positions in verification order, in arrival order) / tidx (their
  // share indices)
  std::vector<uint32_t> tgroup, toff, tpos;
  std::vector<int64_t> tidx;
  size_t m() const { return order.size(); }
  size_t n_vgroups() const { return vgoff.size() - 1; }
  size_t n_touched() const { return tgroup.size(); }
};

// hbls_duty_add_sets_first: the verification order is set-major and, within a set, arrival order -- the
// order of `items` itself, which are increasing caller indices and whose sets are ranges of those.  The
// groups are hgroup.h split_runs' runs (consecutive items over one message, at most gmax), taken set by
// set, so that a group belongs to exactly one set; gset gets each group's set.  sid: the set of each of
// the m items, non-decreasing.
inline MsgGroups group_by_set(const uint32_t* mid, const uint32_t* sid, size_t m, size_t gmax, std::vector<uint32_t>& gset) {
  MsgGroups g{std::vector<uint32_t>(m), std::vector<uint32_t>(mid, mid + m), {}};
  for (size_t q = 0; q < m; q++) g.order[q] = (uint32_t)q;
  gset.clear();
  std::vector<size_t> runs;
  for (size_t a = 0; a < m;) {
    size_t b = a + 1;
    while (b < m && sid[b] == sid[a]) b++;
    split_runs(mid + a, b - a, gmax, runs);
    for (size_t j = 0; j + 1 < runs.size(); j++) {
      g.gstart.push_back(a + runs[j]);
      gset.push_back(sid[a]);
    }
    a = b;
  }
  g.gstart.push_back(m);
  return g;
}

// The plan of one shard (groups gb .. ge) for its items (caller indices, increasing) of an add
// whose first partial has serial first_serial.  New messages are appended to tab.  set_of (nullable;
// hbls_duty_add_sets_first): every caller index's set id -- the plan is then set-major (group_by_set)
// and fills p.vgset; the message ids, the touched groups and the serials are what they are without it.
inline void duty_plan_shard(const uint8_t* msgs, const uint64_t* msg_off, const uint32_t* msg_len,
                            const uint32_t* group, const int64_t* share_idx, const std::vector<uint32_t>& items,
                            size_t gb, size_t ge, uint32_t first_serial, size_t gmax, DutyMsgTable& tab,
                            DutyShardPlan& p, const uint32_t* set_of = nullptr) {
  const size_t m = items.size();
  p.msgs_before = tab.size();
  p.resident = 0;
  std::vector<uint32_t> mid(m);
  for (size_t k = 0; k < m; k++) {
    const size_t i = items[k];
    bool is_new = false;
    if (k && msg_len[items[k - 1]] == msg_len[i] &&
        (!msg_len[i] || msg_off[items[k - 1]] == msg_off[i] || msg_eq(msgs + msg_off[items[k - 1]], msgs + msg_off[i], msg_len[i])))
      mid[k] = mid[k - 1];  // runs of one message: the previous item's id, as msgtable.h
    else
      mid[k] = tab.lookup(msg_len[i] ? msgs + msg_off[i] : (const uint8_t*)"", msg_len[i], &is_new);
    if (!is_new) p.resident++;
  }
  p.vgset.clear();
  std::vector<uint32_t> sid(set_of ? m : 0);
  for (size_t k = 0; k < sid.size(); k++) sid[k] = set_of[items[k]];
  const MsgGroups vg = set_of ? group_by_set(mid.data(), sid.data(), m, gmax, p.vgset)
                              : group_by_message(mid.data(), m, tab.size(), gmax);
  p.order.resize(m);
  p.serial.resize(m);
  std::vector<uint32_t> inv(m);  // position in `items` -> position in verification order
  for (size_t q = 0; q < m; q++) {
    p.order[q] = items[vg.order[q]];
    p.serial[q] = first_serial + items[vg.order[q]];
    inv[vg.order[q]] = (uint32_t)q;
  }
  p.midx = vg.midx;
  p.vgoff.assign(vg.gstart.begin(), vg.gstart.end());
  // the touched groups: a stable counting of the items by group keeps each group's arrival order
  std::vector<uint32_t> mine;  // positions in `items` of the partials of a group of this shard
  for (size_t k = 0; k < m; k++)
    if (group[items[k]] >= gb && group[items[k]] < ge) mine.push_back((uint32_t)k);
  std::stable_sort(mine.begin(), mine.end(),
                   [&](uint32_t a, uint32_t b) { return group[items[a]] < group[items[b]]; });
  p.tgroup.clear();
  p.toff.clear();
  p.tpos.resize(mine.size());
  p.tidx.resize(mine.size());
  for (size_t j = 0; j < mine.size(); j++) {
    const uint32_t g = group[items[mine[j]]] - (uint32_t)gb;
    if (p.tgroup.empty() || p.tgroup.back() != g) {
      p.tgroup.push_back(g);
      p.toff.push_back((uint32_t)j);
    }
    p.tpos[j] = inv[mine[j]];
    p.tidx[j] = share_idx[items[mine[j]]];
  }
  p.toff.push_back((uint32_t)mine.size());
}

// hbls_duty_add_sets: set k of the call is partials [set_off[k], set_off[k + 1]) in arrival order.
// What is wrong with set_off (n_sets + 1 entries: 0 first, n last, non-decreasing), nullptr when
// nothing is.  Checked before anything is enqueued, so that a set id is never past n_sets.
inline const char* duty_check_sets(const uint32_t* set_off, size_t n_sets, size_t n) {
  if (!n_sets) return n ? "n_sets is 0 with partials in the call" : nullptr;
  if (!set_off) return "set_off is required";
  if (set_off[0] != 0) return "set_off[0] must be 0";
  for (size_t k = 0; k < n_sets; k++)
    if (set_off[k + 1] < set_off[k]) return "set_off must not decrease";
  if (set_off[n_sets] != n) return "set_off[n_sets] must be n";
  return nullptr;
}

// each arrival index's set id (set_off as duty_check_sets accepts it)
inline void duty_set_ids(const uint32_t* set_off, size_t n_sets, size_t n, std::vector<uint32_t>& set_of) {
  set_of.resize(n);
  for (size_t k = 0; k < n_sets; k++)
    for (size_t i = set_off[k]; i < set_off[k + 1]; i++) set_of[i] = (uint32_t)k;
}

// A shard's items in its verification order: their set ids.  (Their arrival indices are p.order.)
inline void duty_plan_sets(const std::vector<uint32_t>& set_of, const DutyShardPlan& p, std::vector<uint32_t>& set_id) {
  set_id.resize(p.m());
  for (size_t q = 0; q < p.m(); q++) set_id[q] = set_of[p.order[q]];
}

// Several shards: a set's first failure is the smallest any shard saw (0xffffffff: none)
inline void duty_merge_set_first(uint32_t* merged, const uint32_t* shard, size_t n_sets) {
  for (size_t k = 0; k < n_sets; k++) merged[k] = std::min(merged[k], shard[k]);
}

}  // namespace hb
