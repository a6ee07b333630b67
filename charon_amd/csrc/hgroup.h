// Host-side grouping of the host-buffer Verify calls (hipbls.hip verify_host, verify_large,
// verify_first_host): from each item's message id (msgtable.h MsgTable::idx) to the verification
// groups a call uploads.  Host code only (no HIP), also compiled into the CPU test harness
// (tests/native/hostcheck.cpp hc_group_*, tests/test_hgroup.py).  The group limit gmax is a
// run-time knob (HBLS_GROUP_MAX): a caller reads it once per call, clamped to at least 1.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace hb {

// Whether a verification defers its messages' Miller lines (verify_pipeline defer_msgs): messages
// with about one group each (the chain per group is then no extra work) and the batched sizes
// (fe_min: the batched final exponentiation's group threshold, 0 = never)
inline bool defer_lines(size_t n_groups, size_t n_msgs, size_t fe_min) {
  return fe_min && n_groups >= fe_min && n_groups <= n_msgs;
}

// The group limit of an n-item call: below single_max items (default: fe_min) every item alone
constexpr size_t SINGLE_MAX_DEFAULT = ~size_t(0);
inline size_t call_gmax(size_t n, size_t single_max, size_t fe_min, size_t gmax) {
  return n < (single_max == SINGLE_MAX_DEFAULT ? fe_min : single_max) ? 1 : std::max<size_t>(1, gmax);
}

// The splitting rule: a group starts at item 0, where the message changes, and when the current
// group holds gmax items.  start: the groups' first items, then n.
template <class Off>
inline void split_runs(const uint32_t* mid, size_t n, size_t gmax, std::vector<Off>& start) {
  start.clear();
  for (size_t k = 0; k < n; k++)
    if (k == 0 || mid[k] != mid[k - 1] || k - (size_t)start.back() >= gmax) start.push_back((Off)k);
  start.push_back((Off)n);
}

// A call's items grouped by message: idx is the message id (< n_msgs) of each of the n items.
struct MsgGroups {
  std::vector<uint32_t> order;  // the items by message id, stable (a counting sort: no comparisons)
  std::vector<uint32_t> midx;   // each item's message id, in that order
  std::vector<size_t> gstart;   // group starts in `order`; n_groups + 1 entries, the last is n
  size_t n_groups() const { return gstart.size() - 1; }
};
inline MsgGroups group_by_message(const uint32_t* idx, size_t n, size_t n_msgs, size_t gmax) {
  MsgGroups g{std::vector<uint32_t>(n), std::vector<uint32_t>(n), {}};
  std::vector<uint32_t> mstart(n_msgs + 1, 0);
  for (size_t k = 0; k < n; k++) mstart[idx[k] + 1]++;
  for (size_t j = 0; j < n_msgs; j++) mstart[j + 1] += mstart[j];
  for (size_t k = 0; k < n; k++) g.order[mstart[idx[k]]++] = (uint32_t)k;
  for (size_t k = 0; k < n; k++) g.midx[k] = idx[g.order[k]];
  split_runs(g.midx.data(), n, gmax, g.gstart);
  return g;
}

// off[gb .. ge] rebased to off[gb], appended to out: one device's or one chunk's share of the groups
template <class Off>
inline void rebase_offsets(const Off* off, size_t gb, size_t ge, std::vector<uint32_t>& out) {
  for (size_t g = gb; g <= ge; g++) out.push_back((uint32_t)(off[g] - off[gb]));
}

// A large call's groups (gstart as MsgGroups') in at most K chunks of whole groups, ~n / K items
// each: boundary c is the first group starting at or after item n c / K, kept only if it lies
// beyond the previous boundary and below n_groups.
struct ChunkSplit {
  std::vector<size_t> cg;         // chunk c: groups cg[c] .. cg[c + 1]; from 0 to n_groups
  std::vector<uint32_t> goffs;    // the chunks' group offsets, concatenated, each chunk's from 0
  std::vector<size_t> goff_base;  // chunk c's offsets start at goffs[goff_base[c]]
  size_t n_chunks() const { return cg.size() - 1; }
};
inline ChunkSplit split_chunks(const size_t* gstart, size_t n_groups, size_t K) {
  const size_t n = gstart[n_groups];
  ChunkSplit s{{0}, {}, {}};
  for (size_t c = 1; c < K; c++) {
    const size_t g = (size_t)(std::lower_bound(gstart, gstart + n_groups, n * c / K) - gstart);
    if (g > s.cg.back() && g < n_groups) s.cg.push_back(g);
  }
  s.cg.push_back(n_groups);
  for (size_t c = 0; c + 1 < s.cg.size(); c++) {
    s.goff_base.push_back(s.goffs.size());
    rebase_offsets(gstart, s.cg[c], s.cg[c + 1], s.goffs);
  }
  return s;
}

}  // namespace hb
