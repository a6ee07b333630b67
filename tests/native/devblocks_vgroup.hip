// TEST-ONLY device block harness, the group stage: this unit compiles the product's
// charon_amd/csrc/vgroup.hip itself (fp.h's default HB_ARG_LANES, as in the library) and runs
// launch_slines, launch_group_prep (its three kernels), launch_batch_sum and the verdict launchers
// (launch_batch_verdict, launch_slot_verdict, launch_first_group, launch_first_item) on explicit raw words.
// The second unit of the pair harness (devblocks_pair.hip: the terms are written there): in/out
// arrays pre-filled by the caller and copied back in full, every index checked on the host first.
#include "../../charon_amd/csrc/vgroup.hip"

#include "devblocks.h"

using namespace hb;

// pts: n_pts G2JEntry; list: list_len entries or null (direct), each below n_pts; count: the value of
// *count; lines: n_lines LineEntry, in/out (unit u's line j at lines[j stride + u]); bad: n bytes or
// null, in/out
extern "C" int db_slines(uint32_t n, uint32_t n_pts, const uint32_t* pts, const uint32_t* list, uint32_t list_len,
                         uint32_t count, uint32_t* lines, uint32_t n_lines, uint32_t stride, uint8_t* bad, int guard) {
  if (n < 1 || !pts || !lines || guard > 255) return DB_E_ARG;
  const uint32_t avail = list ? (count < n ? count : n) : n;
  if (list) {
    if (avail > list_len) return DB_E_ARG;
    for (uint32_t u = 0; u < avail; u++)
      if (list[u] >= n_pts) return DB_E_ARG;
  } else if (n > n_pts) {
    return DB_E_ARG;
  }
  if (avail && (uint64_t)(N_LINES - 1) * stride + avail > n_lines) return DB_E_ARG;
  DbIo io;
  const G2JEntry* dpts;
  const uint32_t *dlist, *dcount;
  LineEntry* dlines;
  uint8_t* dbad;
  const uint8_t* dg;
  DB_IN(io, dpts, pts, (size_t)n_pts * sizeof(G2JEntry));
  DB_IN(io, dlist, list, (size_t)list_len * 4);
  DB_IN(io, dcount, list ? &count : nullptr, 4);
  DB_IO(io, dlines, lines, (size_t)n_lines * sizeof(LineEntry));
  DB_IO(io, dbad, bad, n);
  if (const int rc = io.guard(&dg, guard)) return rc;
  launch_slines(dpts, dlist, dcount, n, dlines, stride, dbad, 0, dg);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// launch_group_prep.  kind 0: k_group_prep (gP, gst, gmsg, glines); 1: k_group_prep_b (gP, gst,
// gmsg, gS, bS nullable); 2: k_group_prep_p (gP, gst, gmsg).  GroupPrepArgs as flat words and pointers:
enum {
  G_G0, G_NG,
  G_N_GROUPS,  // groups of the call: grp_off has n_groups + 1 entries; gmsg and the agg_* arrays n_groups
  G_N_ITEMS,   // entries of msg_idx, pk, pk_st, sig, sig_st, pr, sr
  G_N_MSGS, G_FE_BATCH, G_KEYS_ONLY, G_SKIP_HM,
  G_GUARD,     // the guard byte; 2: none
  G_COUNT_
};
enum {
  GA_GRP_OFF, GA_MSG_IDX, GA_HM, GA_PK, GA_PK_ST, GA_SIG, GA_SIG_ST, GA_PR, GA_SR,
  GA_AGG_PK, GA_AGG_PK_ST, GA_AGG_SIG, GA_AGG_ST, GA_AGG_PR, GA_AGG_SR,  // all six or none
  GA_GP, GA_GMSG, GA_GST, GA_GLINES, GA_GS, GA_BS,  // in/out: [ng], [n_groups], [ng], [N_LINES ng], [ng], [batches]
  GA_COUNT_
};
extern "C" int db_group_words() { return G_COUNT_; }
extern "C" int db_group_ptrs() { return GA_COUNT_; }
extern "C" int db_group_states(uint32_t* o) {
  o[0] = G_READY, o[1] = G_FALLBACK, o[2] = G_EMPTY;
  return 3;
}

extern "C" int db_group_prep(int kind, const uint32_t* w, void* const* p) {
  if (!w || !p || kind < 0 || kind > 2 || w[G_NG] < 1 || w[G_GUARD] > 2) return DB_E_ARG;
  const uint32_t g0 = w[G_G0], ng = w[G_NG], n_groups = w[G_N_GROUPS], n_items = w[G_N_ITEMS], n_msgs = w[G_N_MSGS];
  const uint32_t fb = w[G_FE_BATCH] ? w[G_FE_BATCH] : FE_BATCH;
  if ((uint64_t)g0 + ng > n_groups || n_msgs < 1 || n_items < 1) return DB_E_ARG;
  if (fb > FE_BATCH || (fb & (fb - 1))) return DB_E_ARG;
  for (int i = GA_MSG_IDX; i <= GA_SR; i++)
    if (!p[i]) return DB_E_ARG;
  int n_aggp = 0;
  for (int i = GA_AGG_PK; i <= GA_AGG_SR; i++) n_aggp += p[i] != nullptr;
  if (n_aggp != 0 && n_aggp != 6) return DB_E_ARG;
  if (!p[GA_GP] || !p[GA_GMSG] || !p[GA_GST]) return DB_E_ARG;
  if (kind == 0 && (!p[GA_GLINES] || p[GA_GS] || p[GA_BS])) return DB_E_ARG;
  if (kind == 1 && !p[GA_GS]) return DB_E_ARG;
  if (kind == 2 && (p[GA_GS] || p[GA_BS])) return DB_E_ARG;
  const uint32_t* off = (const uint32_t*)p[GA_GRP_OFF];
  if (off) {
    for (uint32_t g = 0; g < n_groups; g++)
      if (off[g] > off[g + 1]) return DB_E_ARG;
    if (off[n_groups] > n_items) return DB_E_ARG;
  } else if (n_groups > n_items) {
    return DB_E_ARG;
  }
  const uint32_t* msg_idx = (const uint32_t*)p[GA_MSG_IDX];
  for (uint32_t i = 0; i < n_items; i++)
    if (msg_idx[i] >= n_msgs) return DB_E_ARG;
  const uint32_t nb = (ng + fb - 1) / fb;
  DbIo io;
  GroupPrepArgs a{};
  DB_IN(io, a.grp_off, p[GA_GRP_OFF], (size_t)(n_groups + 1) * 4);
  DB_IN(io, a.msg_idx, p[GA_MSG_IDX], (size_t)n_items * 4);
  DB_IN(io, a.hm, p[GA_HM], (size_t)n_msgs * sizeof(MsgEntry));
  DB_IN(io, a.pk, p[GA_PK], (size_t)n_items * sizeof(G1AEntry));
  DB_IN(io, a.pk_st, p[GA_PK_ST], n_items);
  DB_IN(io, a.sig, p[GA_SIG], (size_t)n_items * sizeof(HmEntry));
  DB_IN(io, a.sig_st, p[GA_SIG_ST], n_items);
  DB_IN(io, a.pr, p[GA_PR], (size_t)n_items * sizeof(G1JEntry));
  DB_IN(io, a.sr, p[GA_SR], (size_t)n_items * sizeof(G2JEntry));
  DB_IN(io, a.agg_pk, p[GA_AGG_PK], (size_t)n_groups * sizeof(G1AEntry));
  DB_IN(io, a.agg_pk_st, p[GA_AGG_PK_ST], n_groups);
  DB_IN(io, a.agg_sig, p[GA_AGG_SIG], (size_t)n_groups * sizeof(HmEntry));
  DB_IN(io, a.agg_st, p[GA_AGG_ST], n_groups);
  DB_IN(io, a.agg_pr, p[GA_AGG_PR], (size_t)n_groups * sizeof(G1JEntry));
  DB_IN(io, a.agg_sr, p[GA_AGG_SR], (size_t)n_groups * sizeof(G2JEntry));
  DB_IO(io, a.gP, p[GA_GP], (size_t)ng * sizeof(G1AEntry));
  DB_IO(io, a.gmsg, p[GA_GMSG], (size_t)n_groups * 4);
  DB_IO(io, a.gst, p[GA_GST], ng);
  DB_IO(io, a.glines, p[GA_GLINES], (size_t)N_LINES * ng * sizeof(LineEntry));
  DB_IO(io, a.gS, p[GA_GS], (size_t)ng * sizeof(G2JEntry));
  DB_IO(io, a.bS, p[GA_BS], (size_t)nb * sizeof(G2JEntry));
  if (const int rc = io.guard(&a.guard, w[G_GUARD] == 2 ? -1 : (int)w[G_GUARD])) return rc;
  a.g0 = g0, a.ng = ng, a.fe_batch = w[G_FE_BATCH], a.p_only = kind == 2, a.keys_only = (int)w[G_KEYS_ONLY];
  a.skip_hm = (int)w[G_SKIP_HM];
  launch_group_prep(a, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// gS: ng G2JEntry; bS: ceil(ng / k) G2JEntry, in/out
extern "C" int db_batch_sum(uint32_t ng, uint32_t k, const uint32_t* gS, uint32_t* bS, int guard) {
  if (ng < 1 || k < 1 || !gS || !bS || guard > 255) return DB_E_ARG;
  DbIo io;
  const G2JEntry* dgS;
  G2JEntry* dbS;
  const uint8_t* dg;
  DB_IN(io, dgS, gS, (size_t)ng * sizeof(G2JEntry));
  DB_IO(io, dbS, bS, (size_t)((ng + k - 1) / k) * sizeof(G2JEntry));
  if (const int rc = io.guard(&dg, guard)) return rc;
  launch_batch_sum(dgS, ng, k, dbS, 0, dg);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// launch_batch_verdict (k_first_batch first when `first` is given, as the launcher issues them).
// gst: ng bytes; bver: n_bver >= ceil(ng / fe_batch) bytes; gver: n_buf >= ng bytes, list: list_len >=
// ng words, count: one word (0 on entry), first: one word or null -- all in/out
extern "C" int db_batch_verdict(uint32_t ng, const uint8_t* gst, const uint8_t* bver, uint32_t n_bver, uint32_t fe_batch,
                                uint8_t* gver, uint32_t n_buf, uint32_t* list, uint32_t list_len, uint32_t* count,
                                int guard, uint32_t* first, uint32_t g0) {
  if (ng < 1 || !gst || !bver || !gver || ng > n_buf || !list || ng > list_len || !count || *count != 0 || guard > 255)
    return DB_E_ARG;
  const uint32_t fb = fe_batch ? fe_batch : FE_BATCH;
  if ((ng + fb - 1) / fb > n_bver || (uint64_t)g0 + ng > 0xffffffffull) return DB_E_ARG;
  DbIo io;
  const uint8_t *dgst, *dbver, *dg;
  uint8_t* dgver;
  uint32_t *dlist, *dcount, *dfirst;
  DB_IN(io, dgst, gst, ng);
  DB_IN(io, dbver, bver, n_bver);
  DB_IO(io, dgver, gver, n_buf);
  DB_IO(io, dlist, list, (size_t)list_len * 4);
  DB_IO(io, dcount, count, 4);
  DB_IO(io, dfirst, first, 4);
  if (const int rc = io.guard(&dg, guard)) return rc;
  launch_batch_verdict(dgst, dbver, ng, dgver, dlist, dcount, 0, dg, fe_batch, dfirst, g0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// launch_slot_verdict.  gst: ng bytes; sfail: two bytes, gver: n_buf >= ng bytes, in/out
extern "C" int db_slot_verdict(uint32_t ng, const uint8_t* gst, uint8_t* sfail, uint8_t* gver, uint32_t n_buf) {
  if (ng < 1 || !gst || !sfail || !gver || ng > n_buf) return DB_E_ARG;
  DbIo io;
  const uint8_t* dgst;
  uint8_t *dsfail, *dgver;
  DB_IN(io, dgst, gst, ng);
  DB_IO(io, dsfail, sfail, 2);
  DB_IO(io, dgver, gver, n_buf);
  launch_slot_verdict(dgst, dsfail, ng, dgver, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// launch_first_group / launch_first_item.  bytes: n of them; first: one word, in/out
static int db_first(bool item, const uint8_t* bytes, uint32_t n, uint32_t* first) {
  if (!bytes || n < 1 || !first) return DB_E_ARG;
  DbIo io;
  const uint8_t* db;
  uint32_t* dfirst;
  DB_IN(io, db, bytes, n);
  DB_IO(io, dfirst, first, 4);
  if (item) launch_first_item(db, n, dfirst, 0);
  else launch_first_group(db, n, dfirst, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}
extern "C" int db_first_group(const uint8_t* gver, uint32_t n_groups, uint32_t* first) { return db_first(false, gver, n_groups, first); }
extern "C" int db_first_item(const uint8_t* status, uint32_t n, uint32_t* first) { return db_first(true, status, n, first); }
