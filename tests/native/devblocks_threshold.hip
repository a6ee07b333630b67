// TEST-ONLY device block harness, the threshold aggregation: this unit compiles the product's
// charon_amd/csrc/threshold.hip itself (fp.h's default HB_ARG_LANES, as in the library) and is the
// whole of the "ta" harness (libhbls_devblocksta.so, an id of its own).  The terms are the vb
// harness's (devblocks_vbatch.hip): every index and offset array is checked on the host before any
// launch (DB_E_ARG if one points outside its buffer); each entry point drives exactly one product
// launcher, or one launcher sequence the product itself issues; in/out arrays are uploaded as the
// caller filled them (a sentinel pattern) and copied back IN FULL (DbIo), so that what a kernel must
// not write is visible to the test.  Workspace tables are sized by the product's own ta_table_bytes,
// ta_joint_table_bytes and ta_small_table_bytes.  k_group_sum is hipbls.hip's and is not compiled
// here: the test sums a group's output slots itself.
#include "../../charon_amd/csrc/threshold.hip"

#include "devblocks.h"

using namespace hb;

extern "C" const char* db_build_id() { return DB_BUILD_ID; }

static_assert(sizeof(TaDigits) == 32, "the digits are handed to the test as four 64-bit words");
static_assert(SEL_COUNTERS == 4, "the counters are handed to the test as four 64-bit words");

// record sizes in bytes, then the constants the test restates
extern "C" int db_ta_consts(uint32_t* o) {
  o[0] = sizeof(HmEntry), o[1] = sizeof(G2JEntry), o[2] = sizeof(TaDigits), o[3] = sizeof(TaSel);
  o[4] = (uint32_t)TA_SMALL_MAX, o[5] = (uint32_t)TA_JOINT_MAX, o[6] = (uint32_t)FR_SMALL_INV_N;
  o[7] = TASEL_KEYS, o[8] = TASEL_KEY_NONE, o[9] = TASEL_NONE;
  o[10] = M_OK, o[11] = M_BAD_SIG, o[12] = M_BAD_IDX;
  o[13] = TASEL_OK, o[14] = TASEL_FEW, o[15] = TASEL_MIXED, o[16] = TASEL_MODE_FIRST, o[17] = TASEL_MODE_MATCHING;
  o[18] = SEL_SEEN, o[19] = SEL_FEW, o[20] = SEL_SHIFTED, o[21] = SEL_SMALL, o[22] = SEL_COUNTERS;
  o[23] = ST_OK, o[24] = ST_BAD_INPUT, o[25] = ST_UNCHECKED, o[26] = ST_COMBINE_FAILED;
  return 27;
}

// offsets of ng groups: non-decreasing from 0, the last exactly n_items
static bool ta_off_ok(const uint32_t* off, uint32_t ng, uint32_t n_items) {
  if (!off || ng < 1 || off[0] != 0) return false;
  for (uint32_t g = 0; g < ng; g++)
    if (off[g] > off[g + 1]) return false;
  return off[ng] == n_items;
}
// the n member numbers src (null: the identity) each name one of n_pts points
static bool ta_src_ok(const uint32_t* src, uint32_t n, uint32_t n_pts) {
  if (!src) return n <= n_pts;
  for (uint32_t j = 0; j < n; j++)
    if (src[j] >= n_pts) return false;
  return true;
}
// a flag byte argument: 0 / 1 the byte's value, 2 no byte (a null pointer)
static int ta_flag(DbIo& io, const uint8_t** out, uint32_t f) { return io.guard(out, f == 2 ? -1 : (int)f); }

// launch_ta_layout.  grp_off: n_groups + 1 offsets; nonuni: one byte, in/out
extern "C" int db_ta_layout(const uint32_t* grp_off, uint32_t n_groups, uint32_t t_u, uint8_t* nonuni) {
  if (!nonuni || !ta_off_ok(grp_off, n_groups, grp_off ? grp_off[n_groups] : 0)) return DB_E_ARG;
  DbIo io;
  const uint32_t* doff;
  uint8_t* dn;
  DB_IN(io, doff, grp_off, (size_t)(n_groups + 1) * 4);
  DB_IO(io, dn, nonuni, 1);
  launch_ta_layout(doff, n_groups, t_u, dn, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// launch_ta_lambda.  idx: n_buf share indices; grp_off: n_groups + 1 offsets ending at n_partials;
// nonuni: one byte in/out or null; skip: n_groups bytes or null; dig: n_buf TaDigits, mstat: n_buf
// bytes, in/out
extern "C" int db_ta_lambda(const int64_t* idx, const uint32_t* grp_off, uint32_t n_groups, uint32_t n_partials,
                            uint32_t n_buf, int mode, uint32_t t_u, uint8_t* nonuni, const uint8_t* skip, uint64_t* dig,
                            uint8_t* mstat) {
  if (!idx || !dig || !mstat || n_partials < 1 || n_partials > n_buf || mode < 0 || mode > 1) return DB_E_ARG;
  if (!ta_off_ok(grp_off, n_groups, n_partials)) return DB_E_ARG;
  DbIo io;
  const int64_t* didx;
  const uint32_t* doff;
  const uint8_t* dskip;
  uint8_t *dn, *dm;
  TaDigits* dd;
  DB_IN(io, didx, idx, (size_t)n_buf * 8);
  DB_IN(io, doff, grp_off, (size_t)(n_groups + 1) * 4);
  DB_IN(io, dskip, skip, n_groups);
  DB_IO(io, dn, nonuni, 1);
  DB_IO(io, dd, dig, (size_t)n_buf * sizeof(TaDigits));
  DB_IO(io, dm, mstat, n_buf);
  launch_ta_lambda(didx, doff, n_groups, n_partials, mode, dd, dm, 0, t_u, dn, dskip);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// launch_ta_member_status.  sig_st: n_sig bytes; src: n_partials entries below n_sig; mstat: n_buf
// bytes, in/out
extern "C" int db_ta_member_status(const uint8_t* sig_st, uint32_t n_sig, const uint32_t* src, uint32_t n_partials,
                                   uint8_t* mstat, uint32_t n_buf) {
  if (!sig_st || n_sig < 1 || !src || !mstat || n_partials < 1 || n_partials > n_buf) return DB_E_ARG;
  if (!ta_src_ok(src, n_partials, n_sig)) return DB_E_ARG;
  DbIo io;
  const uint8_t* dst;
  const uint32_t* dsrc;
  uint8_t* dm;
  DB_IN(io, dst, sig_st, n_sig);
  DB_IN(io, dsrc, src, (size_t)n_partials * 4);
  DB_IO(io, dm, mstat, n_buf);
  launch_ta_member_status(dst, dsrc, n_partials, dm, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// launch_ta_straus.  pts: n_pts HmEntry; src: n_partials entries below n_pts, or null; dig:
// n_partials TaDigits; skip: n_groups bytes or null; guard: the guard byte, 2: none; out: n_buf
// G2JEntry, in/out
extern "C" int db_ta_straus(const uint32_t* pts, uint32_t n_pts, const uint32_t* src, const uint64_t* dig,
                            uint32_t n_partials, uint32_t n_groups, const uint8_t* skip, uint32_t guard, uint32_t* out,
                            uint32_t n_buf) {
  if (!pts || n_pts < 1 || !dig || !out || n_partials < 1 || n_partials > n_buf || n_groups < 1 || guard > 2)
    return DB_E_ARG;
  if (!ta_src_ok(src, n_partials, n_pts)) return DB_E_ARG;
  DbIo io;
  DbDev ws;
  const HmEntry* dpts;
  const uint32_t* dsrc;
  const TaDigits* dd;
  const uint8_t *dskip, *dg;
  G2JEntry* dout;
  void* tab;
  DB_IN(io, dpts, pts, (size_t)n_pts * sizeof(HmEntry));
  DB_IN(io, dsrc, src, (size_t)n_partials * 4);
  DB_IN(io, dd, dig, (size_t)n_partials * sizeof(TaDigits));
  DB_IN(io, dskip, skip, n_groups);
  DB_IO(io, dout, out, (size_t)n_buf * sizeof(G2JEntry));
  if (const int rc = ta_flag(io, &dg, guard)) return rc;
  DB_MAKE(ws, tab, nullptr, ta_table_bytes(n_partials));
  launch_ta_straus(dpts, dsrc, dd, n_partials, n_groups, tab, dout, 0, dskip, dg);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// launch_ta_joint: k_ta_jtab, k_ta_jladder, k_ta_jgeneral as the product issues them.  Members
// n_groups t; src as db_ta_straus; skip: n_groups bytes or null; nonuni: the byte, 2: none; out: n_buf
// G2JEntry, in/out
extern "C" int db_ta_joint(const uint32_t* pts, uint32_t n_pts, const uint32_t* src, const uint64_t* dig, uint32_t n_groups,
                           uint32_t t, uint32_t c, const uint8_t* skip, uint32_t nonuni, uint32_t* out, uint32_t n_buf) {
  if (!pts || n_pts < 1 || !dig || !out || n_groups < 1 || t < 1 || c < 1 || c > (uint32_t)TA_JOINT_MAX || nonuni > 2)
    return DB_E_ARG;
  const uint64_t n = (uint64_t)n_groups * t;
  if (n > n_buf || !ta_src_ok(src, (uint32_t)n, n_pts)) return DB_E_ARG;
  DbIo io;
  DbDev ws;
  const HmEntry* dpts;
  const uint32_t* dsrc;
  const TaDigits* dd;
  const uint8_t *dskip, *dn;
  G2JEntry* dout;
  void* tab;
  DB_IN(io, dpts, pts, (size_t)n_pts * sizeof(HmEntry));
  DB_IN(io, dsrc, src, (size_t)n * 4);
  DB_IN(io, dd, dig, (size_t)n * sizeof(TaDigits));
  DB_IN(io, dskip, skip, n_groups);
  DB_IO(io, dout, out, (size_t)n_buf * sizeof(G2JEntry));
  if (const int rc = ta_flag(io, &dn, nonuni)) return rc;
  DB_MAKE(ws, tab, nullptr, ta_joint_table_bytes(n_groups, t, c));
  launch_ta_joint(dpts, dsrc, dd, n_groups, t, c, tab, dout, 0, dskip, dn);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// k_ta_sprep, launched as launch_ta_small launches it: the split without the ladders.  idx: n_groups t
// share indices; nonuni: the byte, 2: none; csm: n_groups t, sdig: n_groups TaDigits, sok: n_groups
// bytes, in/out
extern "C" int db_ta_sprep(const int64_t* idx, uint32_t n_groups, uint32_t t, uint32_t nonuni, int64_t* csm, uint64_t* sdig,
                           uint8_t* sok) {
  if (!idx || n_groups < 1 || t < 1 || nonuni > 2 || !csm || !sdig || !sok) return DB_E_ARG;
  const size_t n = (size_t)n_groups * t;
  DbIo io;
  const int64_t* didx;
  const uint8_t* dn;
  int64_t* dc;
  TaDigits* dd;
  uint8_t* dk;
  DB_IN(io, didx, idx, n * 8);
  DB_IO(io, dc, csm, n * 8);
  DB_IO(io, dd, sdig, (size_t)n_groups * sizeof(TaDigits));
  DB_IO(io, dk, sok, n_groups);
  if (const int rc = ta_flag(io, &dn, nonuni)) return rc;
  hipLaunchKernelGGL(k_ta_sprep, dim3(blocks_of(n_groups, 64)), dim3(64), 0, 0, didx, n_groups, t, dc, dd, dk, dn);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// launch_ta_small.  pair: g_ta_pair_max is n_groups (the lane-pair ladder) or 0 (one lane per
// validator) for the call, and restored.  pts / src as db_ta_straus over n_groups t members; csm, sdig,
// sok as db_ta_sprep; done: n_groups bytes, out: n_buf G2JEntry, in/out
extern "C" int db_ta_small(const uint32_t* pts, uint32_t n_pts, const uint32_t* src, const int64_t* idx, uint32_t n_groups,
                           uint32_t t, uint32_t pair, uint32_t nonuni, int64_t* csm, uint64_t* sdig, uint8_t* sok,
                           uint8_t* done, uint32_t* out, uint32_t n_buf) {
  if (!pts || n_pts < 1 || !idx || n_groups < 1 || t < 1 || pair > 1 || nonuni > 2) return DB_E_ARG;
  if (!csm || !sdig || !sok || !done || !out) return DB_E_ARG;
  const uint64_t n = (uint64_t)n_groups * t;
  if (n > n_buf || !ta_src_ok(src, (uint32_t)n, n_pts)) return DB_E_ARG;
  DbIo io;
  DbDev ws;
  const HmEntry* dpts;
  const uint32_t* dsrc;
  const int64_t* didx;
  const uint8_t* dn;
  int64_t* dc;
  TaDigits* dd;
  uint8_t *dk, *ddone;
  G2JEntry* dout;
  void* tab;
  DB_IN(io, dpts, pts, (size_t)n_pts * sizeof(HmEntry));
  DB_IN(io, dsrc, src, (size_t)n * 4);
  DB_IN(io, didx, idx, (size_t)n * 8);
  DB_IO(io, dc, csm, (size_t)n * 8);
  DB_IO(io, dd, sdig, (size_t)n_groups * sizeof(TaDigits));
  DB_IO(io, dk, sok, n_groups);
  DB_IO(io, ddone, done, n_groups);
  DB_IO(io, dout, out, (size_t)n_buf * sizeof(G2JEntry));
  if (const int rc = ta_flag(io, &dn, nonuni)) return rc;
  DB_MAKE(ws, tab, nullptr, ta_small_table_bytes(n_groups));
  const size_t keep = g_ta_pair_max.load();
  g_ta_pair_max.store(pair ? (size_t)n_groups : 0);
  launch_ta_small(dpts, dsrc, didx, n_groups, t, dc, dd, dk, tab, ddone, dout, 0, dn);
  g_ta_pair_max.store(keep);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// The selection kernels over one TaSelectArgs.  Words:
enum {
  L_N,       // verified partials (vstatus, msg_idx)
  L_N_CAND,  // entries of src / idx
  L_N_GROUPS, L_T, L_MODE,
  L_COUNT_
};
enum {
  LA_VSTATUS, LA_MSG_IDX, LA_SRC, LA_IDX, LA_GRP_OFF,                   // db_ta_select's inputs
  LA_CHOSEN, LA_CIDX, LA_TA_COUNT, LA_KEY, LA_STATE, LA_GMSG, LA_HIST,  // its outputs (in/out); db_ta_sel_fill's inputs
  LA_OFF, LA_CUR, LA_PERM, LA_PMEM, LA_PGOFF, LA_PIDX,                  // off: TASEL_KEYS + 1 words; the rest in/out
  LA_CTR,                                                              // SEL_COUNTERS 64-bit words, in/out
  LA_COUNT_
};
extern "C" int db_ta_sel_words() { return L_COUNT_; }
extern "C" int db_ta_sel_ptrs() { return LA_COUNT_; }

// launch_ta_select.  Nothing to refuse among the candidates: offsets beyond n_cand are cut by the
// kernel and a candidate naming no partial (src >= n) counts as not verified
extern "C" int db_ta_select(const uint32_t* w, void* const* p) {
  if (!w || !p) return DB_E_ARG;
  const uint32_t n = w[L_N], nc = w[L_N_CAND], ng = w[L_N_GROUPS], t = w[L_T];
  if (n < 1 || nc < 1 || ng < 1 || t < 1 || t > TASEL_MAX || w[L_MODE] > TASEL_MODE_MATCHING) return DB_E_ARG;
  for (int i = LA_VSTATUS; i <= LA_HIST; i++)
    if (!p[i]) return DB_E_ARG;
  if (!p[LA_CTR]) return DB_E_ARG;
  DbIo io;
  TaSelectArgs a{};
  DB_IN(io, a.vstatus, p[LA_VSTATUS], n);
  DB_IN(io, a.msg_idx, p[LA_MSG_IDX], (size_t)n * 4);
  DB_IN(io, a.src, p[LA_SRC], (size_t)nc * 4);
  DB_IN(io, a.idx, p[LA_IDX], (size_t)nc * 8);
  DB_IN(io, a.grp_off, p[LA_GRP_OFF], (size_t)(ng + 1) * 4);
  DB_IO(io, a.chosen, p[LA_CHOSEN], (size_t)ng * t * 4);
  DB_IO(io, a.cidx, p[LA_CIDX], (size_t)ng * t * 8);
  DB_IO(io, a.ta_count, p[LA_TA_COUNT], (size_t)ng * 4);
  DB_IO(io, a.key, p[LA_KEY], (size_t)ng * 4);
  DB_IO(io, a.state, p[LA_STATE], ng);
  DB_IO(io, a.gmsg, p[LA_GMSG], (size_t)ng * 4);
  DB_IO(io, a.hist, p[LA_HIST], (size_t)TASEL_KEYS * 4);
  DB_IO(io, a.ctr, p[LA_CTR], SEL_COUNTERS * 8);
  a.n = n, a.n_groups = ng, a.t = t, a.n_cand = nc, a.mode = w[L_MODE];
  launch_ta_select(a, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// launch_ta_sel_fill.  key: n_groups entries below TASEL_KEYS; off: TASEL_KEYS + 1 words and cur:
// TASEL_KEYS words, such that every class has room below n_groups (off[k] + cur[k] + the groups of key
// k); chosen, cidx, state as db_ta_select left them
extern "C" int db_ta_sel_fill(const uint32_t* w, void* const* p) {
  if (!w || !p) return DB_E_ARG;
  const uint32_t ng = w[L_N_GROUPS], t = w[L_T];
  if (ng < 1 || t < 1 || t > TASEL_MAX) return DB_E_ARG;
  for (int i : {LA_CHOSEN, LA_CIDX, LA_KEY, LA_STATE, LA_OFF, LA_CUR, LA_PERM, LA_PMEM, LA_PGOFF, LA_PIDX})
    if (!p[i]) return DB_E_ARG;
  const uint32_t *key = (const uint32_t*)p[LA_KEY], *off = (const uint32_t*)p[LA_OFF], *cur = (const uint32_t*)p[LA_CUR];
  for (uint32_t g = 0; g < ng; g++)
    if (key[g] >= TASEL_KEYS) return DB_E_ARG;
  for (uint32_t g = 0; g < ng; g++) {  // the last place of key[g]'s class (quadratic: at most a few hundred groups)
    uint64_t cnt = 0;
    for (uint32_t h = 0; h < ng; h++) cnt += key[h] == key[g];
    if ((uint64_t)off[key[g]] + cur[key[g]] + cnt > ng) return DB_E_ARG;
  }
  DbIo io;
  TaSelectArgs a{};
  DB_IN(io, a.chosen, p[LA_CHOSEN], (size_t)ng * t * 4);
  DB_IN(io, a.cidx, p[LA_CIDX], (size_t)ng * t * 8);
  DB_IN(io, a.key, p[LA_KEY], (size_t)ng * 4);
  DB_IN(io, a.state, p[LA_STATE], ng);
  DB_IN(io, a.off, p[LA_OFF], (size_t)(TASEL_KEYS + 1) * 4);
  DB_IO(io, a.cur, p[LA_CUR], (size_t)TASEL_KEYS * 4);
  DB_IO(io, a.perm, p[LA_PERM], (size_t)ng * 4);
  DB_IO(io, a.pmem, p[LA_PMEM], (size_t)ng * t * 4);
  DB_IO(io, a.pgoff, p[LA_PGOFF], (size_t)(ng + 1) * 4);
  DB_IO(io, a.pidx, p[LA_PIDX], (size_t)ng * t * 8);
  a.n_groups = ng, a.t = t;
  launch_ta_sel_fill(a, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// launch_ta_sel_scatter.  perm: n_groups entries below n_groups, or null; state, pstatus: n_groups
// bytes; pout: 96 n_groups bytes; ppt: n_groups HmEntry; sdone: n_groups bytes or null; ta_out (96
// n_groups bytes), ta_status (n_groups), agg_pt (n_groups HmEntry or null), agg_st (n_groups or null),
// ctr (SEL_COUNTERS 64-bit words): in/out.  Device buffers are 16-byte aligned, so rows16 may be 1.
extern "C" int db_ta_sel_scatter(uint32_t n_groups, const uint32_t* perm, const uint8_t* state, const uint8_t* pout,
                                 const uint8_t* pstatus, const uint32_t* ppt, const uint8_t* sdone, int rows16,
                                 uint8_t* ta_out, uint8_t* ta_status, uint32_t* agg_pt, uint8_t* agg_st, uint64_t* ctr) {
  if (n_groups < 1 || !state || !pout || !pstatus || !ppt || !ta_out || !ta_status || !ctr || rows16 < 0 || rows16 > 1)
    return DB_E_ARG;
  if (perm)
    for (uint32_t g = 0; g < n_groups; g++)
      if (perm[g] >= n_groups) return DB_E_ARG;
  DbIo io;
  TaScatterArgs a{};
  DB_IN(io, a.perm, perm, (size_t)n_groups * 4);
  DB_IN(io, a.state, state, n_groups);
  DB_IN(io, a.pout, pout, (size_t)n_groups * 96);
  DB_IN(io, a.pstatus, pstatus, n_groups);
  DB_IN(io, a.ppt, ppt, (size_t)n_groups * sizeof(HmEntry));
  DB_IN(io, a.sdone, sdone, n_groups);
  DB_IO(io, a.ta_out, ta_out, (size_t)n_groups * 96);
  DB_IO(io, a.ta_status, ta_status, n_groups);
  DB_IO(io, a.agg_pt, agg_pt, (size_t)n_groups * sizeof(HmEntry));
  DB_IO(io, a.agg_st, agg_st, n_groups);
  DB_IO(io, a.ctr, ctr, SEL_COUNTERS * 8);
  a.n_groups = n_groups, a.rows16 = rows16;
  launch_ta_sel_scatter(a, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// launch_ta_sel_verdicts.  ta_status: n_groups bytes; agg_vstatus: n_buf bytes, in/out
extern "C" int db_ta_sel_verdicts(const uint8_t* ta_status, uint32_t n_groups, uint8_t* agg_vstatus, uint32_t n_buf) {
  if (!ta_status || n_groups < 1 || n_groups > n_buf || !agg_vstatus) return DB_E_ARG;
  DbIo io;
  const uint8_t* dst;
  uint8_t* dv;
  DB_IN(io, dst, ta_status, n_groups);
  DB_IO(io, dv, agg_vstatus, n_buf);
  launch_ta_sel_verdicts(dst, n_groups, dv, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}
