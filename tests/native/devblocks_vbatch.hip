// TEST-ONLY device block harness, the combination and verdict stage of the batched verification:
// this unit compiles the product's charon_amd/csrc/vbatch.hip itself (fp.h's default HB_ARG_LANES,
// as in the library) and is the whole of the "vb" harness (libhbls_devblocksvb.so, an id of its own).
// The terms are the pair harness's (devblocks_pair.hip): every index array is checked on the host
// before any launch (DB_E_ARG if one points outside its buffer); each entry point drives exactly one
// product launcher, or one launcher sequence the product itself issues; in/out arrays are uploaded
// as the caller filled them (a sentinel pattern) and copied back IN FULL (DbIo), so that what a
// kernel must not write is visible to the test.
#include "../../charon_amd/csrc/vbatch.hip"

#include "devblocks.h"

using namespace hb;

extern "C" const char* db_build_id() { return DB_BUILD_ID; }

static_assert(sizeof(KeyLearnCtr) == 64, "the counters are handed to the test as eight 64-bit words");

// record sizes in bytes, then the constants the test restates
extern "C" int db_vb_consts(uint32_t* o) {
  o[0] = sizeof(G1AEntry), o[1] = sizeof(HmEntry), o[2] = sizeof(G1JEntry), o[3] = sizeof(G2JEntry);
  o[4] = sizeof(MsgEntry), o[5] = sizeof(LineEntry), o[6] = (uint32_t)N_LINES, o[7] = KEY_WIDE_NONE;
  o[8] = (uint32_t)RLC_DIGITS, o[9] = RLC_CHUNK, o[10] = ST_OK, o[11] = ST_BAD_PUBKEY, o[12] = ST_BAD_SIGNATURE;
  o[13] = ST_NOT_VERIFIED, o[14] = ST_UNCHECKED, o[15] = GV_PASS, o[16] = GV_UNCHECKED, o[17] = GV_NOT_READY;
  o[18] = sizeof(KeyLearnCtr);
  return 19;
}

// offsets of ng groups: non-decreasing from 0, the last at most n_items
static bool vb_off_ok(const uint32_t* off, uint32_t ng, uint32_t n_items) {
  if (off[0] != 0) return false;
  for (uint32_t g = 0; g < ng; g++)
    if (off[g] > off[g + 1]) return false;
  return off[ng] <= n_items;
}

// the ladder tables of n_wide good, finite keys (ec28.h g1_wide_build per key, as k_pk_wide)
__global__ __launch_bounds__(64) void k_vb_tables(uint32_t n, const G1AEntry* __restrict__ pk, G1WidePt* __restrict__ wide) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const G1AEntry e = pk[i];
  g1_wide_build(G1A{e.x, e.y, false}, wide + (uint64_t)KEY_WIDE_PTS * i);
#endif
}

// KeyWideRef over the tables of wide_pk's n_wide keys (none flagged infinite: checked) and the entry
// numbers went (n of them, each below n_wide or KEY_WIDE_NONE); ctr: eight 64-bit words, in/out
static int vb_wide(DbIo& io, DbDev& ws, uint32_t n, uint32_t n_wide, const uint32_t* went, const uint32_t* wide_pk,
                   void* ctr, KeyWideRef& kw) {
  kw = KeyWideRef{};
  if (!went) return 0;
  if (!n_wide || !wide_pk || !ctr) return DB_E_ARG;
  for (uint32_t i = 0; i < n; i++)
    if (went[i] != KEY_WIDE_NONE && went[i] >= n_wide) return DB_E_ARG;
  for (uint32_t e = 0; e < n_wide; e++)
    if (wide_pk[(sizeof(G1AEntry) / 4) * e + 24] != 0) return DB_E_ARG;  // G1AEntry::inf
  const G1AEntry* dpk;
  G1WidePt* dwide;
  DB_IN(io, kw.ent, went, (size_t)n * 4);
  DB_IN(io, dpk, wide_pk, (size_t)n_wide * sizeof(G1AEntry));
  DB_IO(io, kw.ctr, ctr, sizeof(KeyLearnCtr));
  DB_MAKE(ws, dwide, nullptr, (size_t)n_wide * KEY_WIDE_PTS * sizeof(G1WidePt));
  hipLaunchKernelGGL(k_vb_tables, dim3((n_wide + 63) / 64), dim3(64), 0, 0, n_wide, dpk, dwide);
  if (const int rc = db_finish()) return rc;
  kw.wide = dwide;
  return 0;
}

// launch_item_group.  grp_off: n_groups + 1 offsets or null; item_grp: n_buf words, in/out
extern "C" int db_vb_item_group(const uint32_t* grp_off, uint32_t n_groups, uint32_t n, uint32_t* item_grp,
                                uint32_t n_buf) {
  if (n < 1 || !item_grp || n > n_buf) return DB_E_ARG;
  if (grp_off && (n_groups < 1 || !vb_off_ok(grp_off, n_groups, 0xffffffffu) || grp_off[n_groups] < n)) return DB_E_ARG;
  DbIo io;
  const uint32_t* doff;
  uint32_t* dig;
  DB_IN(io, doff, grp_off, (size_t)(n_groups + 1) * 4);
  DB_IO(io, dig, item_grp, (size_t)n_buf * 4);
  launch_item_group(doff, n_groups, n, dig, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// launch_rlc.  Words, then the 8 key words:
enum {
  R_SIDES, R_ALWAYS, R_N,
  R_N_BUF,     // entries of every per-item array (>= n)
  R_KEY_BASE,
  R_GUARD,     // the guard byte; 2: none
  R_N_GROUPS,  // grp_off has n_groups + 1 entries
  R_N_WIDE,    // keys of wide_pk
  R_KEY,
  R_COUNT_ = R_KEY + 8
};
enum {
  RA_PK, RA_PK_ST, RA_SIG, RA_SIG_ST,  // sig and sig_st: both or neither (sides 1)
  RA_ITEM_GRP, RA_GRP_OFF,             // both or neither
  RA_POUT, RA_SOUT, RA_COEF,           // in/out
  RA_WENT, RA_WIDE_PK, RA_CTR,         // all three or none: entry numbers, the keys of the tables, the counters (in/out)
  RA_COUNT_
};
extern "C" int db_vb_rlc_words() { return R_COUNT_; }
extern "C" int db_vb_rlc_ptrs() { return RA_COUNT_; }

extern "C" int db_vb_rlc(const uint32_t* w, void* const* p) {
  if (!w || !p) return DB_E_ARG;
  const uint32_t sides = w[R_SIDES], n = w[R_N], nb = w[R_N_BUF], ng = w[R_N_GROUPS];
  if (sides < 1 || sides > 3 || n < 1 || n > nb || w[R_GUARD] > 2) return DB_E_ARG;
  if (!p[RA_PK] || !p[RA_PK_ST] || !p[RA_SIG] != !p[RA_SIG_ST] || !p[RA_ITEM_GRP] != !p[RA_GRP_OFF]) return DB_E_ARG;
  if (!p[RA_SIG] && sides != 1) return DB_E_ARG;
  if (((sides & 1) && !p[RA_POUT]) || ((sides & 2) && !p[RA_SOUT]) || (sides == 2 && !p[RA_COEF])) return DB_E_ARG;
  if (p[RA_GRP_OFF]) {
    const uint32_t* ig = (const uint32_t*)p[RA_ITEM_GRP];
    if (ng < 1) return DB_E_ARG;
    for (uint32_t i = 0; i < n; i++)
      if (ig[i] >= ng) return DB_E_ARG;
  }
  DbIo io;
  DbDev ws;
  const G1AEntry* pk;
  const HmEntry* sig;
  const uint8_t *pk_st, *sig_st, *dg;
  const uint32_t *item_grp, *grp_off;
  G1JEntry* pout;
  G2JEntry* sout;
  uint2* coef;
  KeyWideRef kw;
  DB_IN(io, pk, p[RA_PK], (size_t)nb * sizeof(G1AEntry));
  DB_IN(io, pk_st, p[RA_PK_ST], nb);
  DB_IN(io, sig, p[RA_SIG], (size_t)nb * sizeof(HmEntry));
  DB_IN(io, sig_st, p[RA_SIG_ST], nb);
  DB_IN(io, item_grp, p[RA_ITEM_GRP], (size_t)nb * 4);
  DB_IN(io, grp_off, p[RA_GRP_OFF], (size_t)(ng + 1) * 4);
  DB_IO(io, pout, p[RA_POUT], (size_t)nb * sizeof(G1JEntry));
  DB_IO(io, sout, p[RA_SOUT], (size_t)nb * sizeof(G2JEntry));
  DB_IO(io, coef, p[RA_COEF], (size_t)nb * 8);
  if (const int rc = io.guard(&dg, w[R_GUARD] == 2 ? -1 : (int)w[R_GUARD])) return rc;
  if (const int rc = vb_wide(io, ws, n, w[R_N_WIDE], (const uint32_t*)p[RA_WENT], (const uint32_t*)p[RA_WIDE_PK], p[RA_CTR], kw))
    return rc;
  RlcKey key;
  for (int j = 0; j < 8; j++) key.w[j] = w[R_KEY + j];
  launch_rlc(pk, pk_st, sig, sig_st, item_grp, grp_off, (int)w[R_ALWAYS], n, w[R_KEY_BASE], key, pout, sout, 0, coef,
             (int)sides, dg, kw);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// launch_plan.  grp_off: ng + 1 offsets; cnt [ng], coff [ng + 1], cfirst / ccount [cap], in/out; cap
// at least the number of chunks
extern "C" int db_vb_plan(const uint32_t* grp_off, uint32_t ng, uint32_t cmax, uint32_t cap, uint32_t* cnt, uint32_t* coff,
                          uint32_t* cfirst, uint32_t* ccount) {
  if (!grp_off || ng < 1 || cmax < 1 || !cnt || !coff || !cfirst || !ccount) return DB_E_ARG;
  if (!vb_off_ok(grp_off, ng, 0x7fffffffu)) return DB_E_ARG;
  uint64_t total = 0;
  for (uint32_t g = 0; g < ng; g++) total += (grp_off[g + 1] - grp_off[g] + cmax - 1) / cmax;
  if (total > cap) return DB_E_ARG;
  DbIo io;
  const uint32_t* doff;
  uint32_t *dcnt, *dcoff, *dcf, *dcc;
  DB_IN(io, doff, grp_off, (size_t)(ng + 1) * 4);
  DB_IO(io, dcnt, cnt, (size_t)ng * 4);
  DB_IO(io, dcoff, coff, (size_t)(ng + 1) * 4);
  DB_IO(io, dcf, cfirst, (size_t)cap * 4);
  DB_IO(io, dcc, ccount, (size_t)cap * 4);
  launch_plan(doff, ng, cmax, dcnt, dcoff, dcf, dcc, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// launch_scan.  cnt: n words; off: n + 1 words, in/out
extern "C" int db_vb_scan(const uint32_t* cnt, uint32_t n, uint32_t* off) {
  if (!cnt || n < 1 || !off) return DB_E_ARG;
  DbIo io;
  const uint32_t* dcnt;
  uint32_t* doff;
  DB_IN(io, dcnt, cnt, (size_t)n * 4);
  DB_IO(io, doff, off, (size_t)(n + 1) * 4);
  launch_scan(dcnt, n, doff, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// What the product runs for a chunked combination: launch_plan, then launch_rlc_msm(args, n / cmax +
// n_groups) with n = grp_off[ng]; with M_THEN2 a second launch_rlc_msm of sides 2 over the coef the
// sides-1 launch left (the slot-wide check's second pass).  Words, then the 8 key words:
enum {
  M_SIDES, M_THEN2, M_SPARSE, M_ALWAYS,
  M_N_BUF,  // entries of every per-item array (>= grp_off[ng])
  M_NG, M_CMAX, M_KEY_BASE,
  M_GUARD,  // 2: none
  M_CAP,    // entries of cfirst / ccount (>= the number of chunks)
  M_N_WIDE,
  M_KEY,
  M_COUNT_ = M_KEY + 8
};
enum {
  MA_GRP_OFF, MA_PK, MA_PK_ST, MA_SIG, MA_SIG_ST,
  MA_POUT, MA_SOUT, MA_COEF, MA_COEF4,             // in/out, per item (coef4 when sparse)
  MA_CNT, MA_COFF, MA_CFIRST, MA_CCOUNT,           // in/out: the plan
  MA_WENT, MA_WIDE_PK, MA_CTR,                     // as db_vb_rlc
  MA_COUNT_
};
extern "C" int db_vb_rlc_msm_words() { return M_COUNT_; }
extern "C" int db_vb_rlc_msm_ptrs() { return MA_COUNT_; }

extern "C" int db_vb_rlc_msm(const uint32_t* w, void* const* p) {
  if (!w || !p) return DB_E_ARG;
  const uint32_t sides = w[M_SIDES], nb = w[M_N_BUF], ng = w[M_NG], cmax = w[M_CMAX], cap = w[M_CAP];
  if (sides < 1 || sides > 3 || ng < 1 || cmax < 1 || w[M_GUARD] > 2 || w[M_SPARSE] > 1) return DB_E_ARG;
  if (w[M_THEN2] && sides != 1) return DB_E_ARG;
  if (w[M_SPARSE] && (sides == 2 || w[M_THEN2] || !p[MA_COEF4])) return DB_E_ARG;
  for (int i = MA_GRP_OFF; i <= MA_COEF; i++)
    if (!p[i]) return DB_E_ARG;
  for (int i = MA_CNT; i <= MA_CCOUNT; i++)
    if (!p[i]) return DB_E_ARG;
  const uint32_t* off = (const uint32_t*)p[MA_GRP_OFF];
  if (!vb_off_ok(off, ng, nb)) return DB_E_ARG;
  const uint32_t n = off[ng];
  if (n < 1) return DB_E_ARG;
  uint64_t total = 0;
  for (uint32_t g = 0; g < ng; g++) total += (off[g + 1] - off[g] + cmax - 1) / cmax;
  if (total > cap) return DB_E_ARG;
  DbIo io;
  DbDev ws;
  RlcMsmArgs a{};
  const uint32_t* doff;
  uint32_t *dcnt, *dcoff, *dcf, *dcc;
  DB_IN(io, doff, p[MA_GRP_OFF], (size_t)(ng + 1) * 4);
  DB_IN(io, a.pk, p[MA_PK], (size_t)nb * sizeof(G1AEntry));
  DB_IN(io, a.pk_st, p[MA_PK_ST], nb);
  DB_IN(io, a.sig, p[MA_SIG], (size_t)nb * sizeof(HmEntry));
  DB_IN(io, a.sig_st, p[MA_SIG_ST], nb);
  DB_IO(io, a.pout, p[MA_POUT], (size_t)nb * sizeof(G1JEntry));
  DB_IO(io, a.sout, p[MA_SOUT], (size_t)nb * sizeof(G2JEntry));
  DB_IO(io, a.coef, p[MA_COEF], (size_t)nb * 8);
  DB_IO(io, a.coef4, p[MA_COEF4], (size_t)nb * 16);
  DB_IO(io, dcnt, p[MA_CNT], (size_t)ng * 4);
  DB_IO(io, dcoff, p[MA_COFF], (size_t)(ng + 1) * 4);
  DB_IO(io, dcf, p[MA_CFIRST], (size_t)cap * 4);
  DB_IO(io, dcc, p[MA_CCOUNT], (size_t)cap * 4);
  if (const int rc = io.guard(&a.guard, w[M_GUARD] == 2 ? -1 : (int)w[M_GUARD])) return rc;
  if (const int rc = vb_wide(io, ws, n, w[M_N_WIDE], (const uint32_t*)p[MA_WENT], (const uint32_t*)p[MA_WIDE_PK], p[MA_CTR], a.kw))
    return rc;
  DB_MAKE(ws, a.t1, nullptr, (size_t)nb * 4 * sizeof(G1J));
  DB_MAKE(ws, a.t2, nullptr, (size_t)nb * 4 * sizeof(G2J));
  a.cfirst = dcf, a.ccount = dcc, a.total = dcoff + ng;
  a.key_base = w[M_KEY_BASE];
  for (int j = 0; j < 8; j++) a.key.w[j] = w[M_KEY + j];
  a.sparse = (int)w[M_SPARSE], a.always = (int)w[M_ALWAYS], a.sides = (int)sides;
  launch_plan(doff, ng, cmax, dcnt, dcoff, dcf, dcc, 0);
  launch_rlc_msm(a, n / cmax + ng, 0);
  if (w[M_THEN2]) {
    a.sides = 2;
    launch_rlc_msm(a, n / cmax + ng, 0);
  }
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// launch_scatter over a whole ScatterArgs.  Words:
enum {
  S_N,
  S_N_BUF,     // entries of status (>= n)
  S_N_GROUPS,  // entries of gverdict; grp_off has n_groups + 1
  S_N_MSGS, S_N_AGG,
  S_AGG_BUF,   // entries of agg_status (>= n_agg)
  S_LIST_LEN,  // entries of list (>= n + n_agg)
  S_HAS_FIRST, S_FIRST,  // first_group: given, its value
  S_COUNT_
};
enum {
  SA_ITEM_GRP, SA_MSG_IDX, SA_HM, SA_PK, SA_PK_ST, SA_SIG, SA_SIG_ST, SA_GVERDICT,
  SA_GRP_OFF,  // nullable
  SA_TA_STATUS, SA_AGG_PK, SA_AGG_PK_ST, SA_AGG_SIG,  // n_agg entries each (n_agg > 0)
  SA_AGG_STATUS, SA_STATUS, SA_LIST, SA_COUNT,        // in/out
  SA_COUNT_
};
extern "C" int db_vb_scatter_words() { return S_COUNT_; }
extern "C" int db_vb_scatter_ptrs() { return SA_COUNT_; }

extern "C" int db_vb_scatter(const uint32_t* w, void* const* p) {
  if (!w || !p) return DB_E_ARG;
  const uint32_t n = w[S_N], nb = w[S_N_BUF], ng = w[S_N_GROUPS], nm = w[S_N_MSGS], na = w[S_N_AGG], ab = w[S_AGG_BUF];
  if (n < 1 || n > nb || ng < 1 || nm < 1 || na > ab || na > ng || (uint64_t)n + na > w[S_LIST_LEN]) return DB_E_ARG;
  for (int i = SA_ITEM_GRP; i <= SA_GVERDICT; i++)
    if (!p[i]) return DB_E_ARG;
  if (na)
    for (int i = SA_TA_STATUS; i <= SA_AGG_STATUS; i++)
      if (!p[i]) return DB_E_ARG;
  if (!p[SA_STATUS] || !p[SA_LIST] || !p[SA_COUNT]) return DB_E_ARG;
  const uint32_t *ig = (const uint32_t*)p[SA_ITEM_GRP], *mi = (const uint32_t*)p[SA_MSG_IDX];
  for (uint32_t i = 0; i < n; i++)
    if (ig[i] >= ng || mi[i] >= nm) return DB_E_ARG;
  if (*(const uint32_t*)p[SA_COUNT] != 0) return DB_E_ARG;  // the list is filled from its start
  DbIo io;
  ScatterArgs a{};
  DB_IN(io, a.item_grp, p[SA_ITEM_GRP], (size_t)n * 4);
  DB_IN(io, a.msg_idx, p[SA_MSG_IDX], (size_t)n * 4);
  DB_IN(io, a.hm, p[SA_HM], (size_t)nm * sizeof(MsgEntry));
  DB_IN(io, a.pk, p[SA_PK], (size_t)n * sizeof(G1AEntry));
  DB_IN(io, a.pk_st, p[SA_PK_ST], n);
  DB_IN(io, a.sig, p[SA_SIG], (size_t)n * sizeof(HmEntry));
  DB_IN(io, a.sig_st, p[SA_SIG_ST], n);
  DB_IN(io, a.gverdict, p[SA_GVERDICT], ng);
  DB_IN(io, a.grp_off, p[SA_GRP_OFF], (size_t)(ng + 1) * 4);
  if (na) {
    DB_IN(io, a.ta_status, p[SA_TA_STATUS], na);
    DB_IN(io, a.agg_pk, p[SA_AGG_PK], (size_t)na * sizeof(G1AEntry));
    DB_IN(io, a.agg_pk_st, p[SA_AGG_PK_ST], na);
    DB_IN(io, a.agg_sig, p[SA_AGG_SIG], (size_t)na * sizeof(HmEntry));
    DB_IO(io, a.agg_status, p[SA_AGG_STATUS], ab);
  }
  DB_IO(io, a.status, p[SA_STATUS], nb);
  DB_IO(io, a.list, p[SA_LIST], (size_t)w[S_LIST_LEN] * 4);
  DB_IO(io, a.count, p[SA_COUNT], 4);
  const uint32_t first = w[S_FIRST];
  DB_IN(io, a.first_group, w[S_HAS_FIRST] ? &first : nullptr, 4);
  a.n = n, a.n_agg = na;
  launch_scatter(a, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// launch_fb_lines.  list: list_len entries, each listed one (base + u < count, u < cap) below n_items
// + n_agg; sig: n_items HmEntry; agg_sig: n_agg HmEntry or null; lines: N_LINES cap LineEntry, in/out
extern "C" int db_vb_fb_lines(const uint32_t* list, uint32_t list_len, uint32_t count, uint32_t base, uint32_t cap,
                              const uint32_t* sig, uint32_t n_items, const uint32_t* agg_sig, uint32_t n_agg,
                              uint32_t* lines) {
  if (!list || cap < 1 || !sig || n_items < 1 || !lines || (n_agg && !agg_sig)) return DB_E_ARG;
  for (uint32_t u = 0; u < cap && (uint64_t)base + u < count; u++)
    if (base + u >= list_len || list[base + u] >= (uint64_t)n_items + n_agg) return DB_E_ARG;
  DbIo io;
  const uint32_t *dlist, *dcount;
  const HmEntry *dsig, *dagg;
  LineEntry* dlines;
  DB_IN(io, dlist, list, (size_t)list_len * 4);
  DB_IN(io, dcount, &count, 4);
  DB_IN(io, dsig, sig, (size_t)n_items * sizeof(HmEntry));
  DB_IN(io, dagg, n_agg ? agg_sig : nullptr, (size_t)n_agg * sizeof(HmEntry));
  DB_IO(io, dlines, lines, (size_t)N_LINES * cap * sizeof(LineEntry));
  launch_fb_lines(dlist, dcount, base, cap, dsig, dagg, n_items, dlines, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// launch_sig_lines.  sig: n HmEntry; lines: n_lines LineEntry, in/out (signature i's line j at j stride + i)
extern "C" int db_vb_sig_lines(const uint32_t* sig, uint32_t n, uint32_t* lines, uint32_t n_lines, uint32_t stride) {
  if (!sig || n < 1 || !lines || (uint64_t)(N_LINES - 1) * stride + n > n_lines) return DB_E_ARG;
  DbIo io;
  const HmEntry* dsig;
  LineEntry* dlines;
  DB_IN(io, dsig, sig, (size_t)n * sizeof(HmEntry));
  DB_IO(io, dlines, lines, (size_t)n_lines * sizeof(LineEntry));
  launch_sig_lines(dsig, n, dlines, stride, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// launch_seg_sum.  pts: n_pts G1AEntry (affine) or G1JEntry; st_in: n_pts bytes; seg_off: n_seg + 1
// offsets; out: n_out G1JEntry, st_out: n_out bytes, in/out
extern "C" int db_vb_seg_sum(int affine, const uint32_t* pts, const uint8_t* st_in, uint32_t n_pts, const uint32_t* seg_off,
                             uint32_t n_seg, uint32_t* out, uint8_t* st_out, uint32_t n_out) {
  if (!pts || !st_in || n_pts < 1 || !seg_off || n_seg < 1 || n_seg > n_out || !out || !st_out) return DB_E_ARG;
  if (!vb_off_ok(seg_off, n_seg, n_pts)) return DB_E_ARG;
  DbIo io;
  const void* dpts;
  const uint8_t* dst;
  const uint32_t* doff;
  G1JEntry* dout;
  uint8_t* dso;
  DB_IN(io, dpts, pts, (size_t)n_pts * (affine ? sizeof(G1AEntry) : sizeof(G1JEntry)));
  DB_IN(io, dst, st_in, n_pts);
  DB_IN(io, doff, seg_off, (size_t)(n_seg + 1) * 4);
  DB_IO(io, dout, out, (size_t)n_out * sizeof(G1JEntry));
  DB_IO(io, dso, st_out, n_out);
  launch_seg_sum(affine != 0, dpts, dst, doff, n_seg, dout, dso, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// launch_va_point.  sums: n_sums G1JEntry; sum_of_group: n_groups entries, each below n_sums or
// 0xffffffff; out: n_out G1AEntry, in/out
extern "C" int db_vb_va_point(const uint32_t* sums, uint32_t n_sums, const uint32_t* sum_of_group, uint32_t n_groups,
                              uint32_t* out, uint32_t n_out) {
  if (!sums || n_sums < 1 || !sum_of_group || n_groups < 1 || n_groups > n_out || !out) return DB_E_ARG;
  for (uint32_t g = 0; g < n_groups; g++)
    if (sum_of_group[g] != 0xffffffffu && sum_of_group[g] >= n_sums) return DB_E_ARG;
  DbIo io;
  const G1JEntry* dsums;
  const uint32_t* dsg;
  G1AEntry* dout;
  DB_IN(io, dsums, sums, (size_t)n_sums * sizeof(G1JEntry));
  DB_IN(io, dsg, sum_of_group, (size_t)n_groups * 4);
  DB_IO(io, dout, out, (size_t)n_out * sizeof(G1AEntry));
  launch_va_point(dsums, dsg, n_groups, dout, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// launch_va_status.  sig: n_groups HmEntry; sig_st, pv: n_groups bytes; key_bad: n_sums bytes;
// sum_of_group as db_vb_va_point; status: n_out bytes, in/out
extern "C" int db_vb_va_status(const uint32_t* sig, const uint8_t* sig_st, const uint8_t* key_bad, uint32_t n_sums,
                               const uint32_t* sum_of_group, const uint8_t* pv, uint32_t n_groups, uint8_t* status,
                               uint32_t n_out) {
  if (!sig || !sig_st || !key_bad || n_sums < 1 || !sum_of_group || !pv || n_groups < 1 || n_groups > n_out || !status)
    return DB_E_ARG;
  for (uint32_t g = 0; g < n_groups; g++)
    if (sum_of_group[g] != 0xffffffffu && sum_of_group[g] >= n_sums) return DB_E_ARG;
  DbIo io;
  const HmEntry* dsig;
  const uint8_t *dst, *dkb, *dpv;
  const uint32_t* dsg;
  uint8_t* dstatus;
  DB_IN(io, dsig, sig, (size_t)n_groups * sizeof(HmEntry));
  DB_IN(io, dst, sig_st, n_groups);
  DB_IN(io, dkb, key_bad, n_sums);
  DB_IN(io, dsg, sum_of_group, (size_t)n_groups * 4);
  DB_IN(io, dpv, pv, n_groups);
  DB_IO(io, dstatus, status, n_out);
  launch_va_status(dsig, dst, dkb, dsg, dpv, n_groups, dstatus, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}
