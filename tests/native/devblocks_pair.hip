// TEST-ONLY device block harness, the Miller-loop kernels: this unit compiles the product's
// charon_amd/csrc/pipeline.hip itself (its kernels and launchers as the library has them; the file
// sets its own HB_FAST_FPMUL and HB_ARG_LANES 128) and runs ONE launcher per entry point on explicit
// raw words.  With devblocks_vgroup.hip it is the pair harness (build.py DEVBLOCKS_PAIR: a library
// and an id of its own); tests/test_gpu_pairing.py compares what the kernels store with the oracle.
// The product library never loads this.
//
// Every entry point uploads the caller's arrays, launches on stream 0, synchronises once and copies
// every output array back in full.  Output arrays are in/out: they go up as the caller filled them
// (a sentinel pattern, never zero: zero is ST_OK / G_READY / GV_PASS), so that entries a kernel must
// not write are visible.  Every index a kernel will follow (units, list entries, message numbers,
// strides and offsets) is checked on the host against the array lengths first: DB_E_ARG before any
// launch, never a read or write outside a buffer.
//
// The unit is not split by launcher families (-DDB_PAIR=k, as devblocks_h2c.hip is): it includes
// pipeline.hip whole, so every part would compile every kernel again; its compile time is
// pipeline.hip's own in the library.
#include "../../charon_amd/csrc/pipeline.hip"

#include "devblocks.h"

using namespace hb;

extern "C" const char* db_build_id() { return DB_BUILD_ID; }

// N_LINES, GROUPS_PER_WAVE, MML_PAIRS, PROD_FAN, FE_BATCH, then the record sizes in bytes
extern "C" void db_pair_consts(uint32_t* o) {
  o[0] = (uint32_t)N_LINES, o[1] = (uint32_t)GROUPS_PER_WAVE, o[2] = MML_PAIRS, o[3] = PROD_FAN, o[4] = FE_BATCH;
  o[5] = sizeof(MsgEntry), o[6] = sizeof(LineEntry), o[7] = sizeof(Fp4Entry), o[8] = sizeof(G2JEntry);
  o[9] = sizeof(G1AEntry), o[10] = sizeof(HmEntry);
}

static constexpr size_t F12 = 3 * sizeof(Fp4Entry);  // one stored Fp12 value: the three roles

// hm: n_tab MsgEntry, in/out (the lines of the first n are written); guard < 0: none
extern "C" int db_lines_msg(uint32_t n, uint32_t n_tab, uint32_t* hm, int guard) {
  if (n < 1 || n > n_tab || !hm || guard > 255) return DB_E_ARG;
  DbIo io;
  MsgEntry* d;
  const uint8_t* dg;
  DB_IO(io, d, hm, (size_t)n_tab * sizeof(MsgEntry));
  if (const int rc = io.guard(&dg, guard)) return rc;
  launch_lines_msg(d, n, 0, dg);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// pk: n G1AEntry; pk_st: n bytes or null; msg_idx: n, each below n_msgs; hm: n_msgs MsgEntry;
// ev: N_LINES x n LineEntry, in/out.  at_p: k_lines_at_p (from hm[].h), else k_mml_eval (from hm[].lines)
static int eval_lines(bool at_p, uint32_t n, uint32_t n_msgs, const uint32_t* pk, const uint8_t* pk_st,
                      const uint32_t* msg_idx, const uint32_t* hm, uint32_t* ev) {
  if (n < 1 || n_msgs < 1 || !pk || !msg_idx || !hm || !ev) return DB_E_ARG;
  for (uint32_t i = 0; i < n; i++)
    if (msg_idx[i] >= n_msgs) return DB_E_ARG;
  DbIo io;
  Pair3Args a{};
  LineEntry* dev;
  DB_IN(io, a.pk, pk, (size_t)n * sizeof(G1AEntry));
  DB_IN(io, a.pk_st, pk_st, n);
  DB_IN(io, a.msg_idx, msg_idx, (size_t)n * 4);
  DB_IN(io, a.hm, hm, (size_t)n_msgs * sizeof(MsgEntry));
  DB_IO(io, dev, ev, (size_t)N_LINES * n * sizeof(LineEntry));
  a.f_n = n;
  if (at_p) launch_lines_at_p(a, dev, 0);
  else launch_mml_eval(a, dev, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}
extern "C" int db_lines_at_p(uint32_t n, uint32_t n_msgs, const uint32_t* pk, const uint8_t* pk_st,
                             const uint32_t* msg_idx, const uint32_t* hm, uint32_t* ev) {
  return eval_lines(true, n, n_msgs, pk, pk_st, msg_idx, hm, ev);
}
extern "C" int db_mml_eval(uint32_t n, uint32_t n_msgs, const uint32_t* pk, const uint8_t* pk_st,
                           const uint32_t* msg_idx, const uint32_t* hm, uint32_t* ev) {
  return eval_lines(false, n, n_msgs, pk, pk_st, msg_idx, hm, ev);
}

// k_pair3<mode> through its launcher.  Pair3Args as flat words and pointers:
enum {
  W_N, W_STRIDE, W_BASE, W_N_ITEMS, W_F_RANGE, W_F_N, W_F_OUT_STRIDE, W_F_OUT_OFF,
  W_COUNT,     // the value of *count (list mode)
  W_GUARD,     // the guard byte; 2: no guard
  W_N_ENT,     // entries of pk, pk_st, sig_st, sig_inf, msg_idx, status, f_bad
  W_N_MSGS,    // entries of hm
  W_N_AGG,     // entries of agg_pk, agg_msg, agg_status
  W_LIST_LEN,  // entries of list
  W_N_LINES,   // LineEntry records of sig_lines
  W_F_IN_LEN, W_F_OUT_LEN,  // stored values (three Fp4Entry each) of f_in, f_out
  W_COUNT_
};
enum {
  A_PK, A_PK_ST, A_SIG_ST, A_SIG_INF, A_MSG_IDX, A_HM, A_SIG_LINES, A_LIST, A_AGG_PK, A_AGG_MSG, A_F_IN,
  A_STATUS, A_AGG_STATUS, A_F_OUT, A_F_BAD,  // in/out
  A_COUNT_
};
extern "C" int db_pair3_words() { return W_COUNT_; }
extern "C" int db_pair3_ptrs() { return A_COUNT_; }

extern "C" int db_pair3(int mode, const uint32_t* w, void* const* p) {
  if (!w || !p || mode < P3_FULL || mode > P3_MLS || w[W_N] < 1 || w[W_GUARD] > 2) return DB_E_ARG;
  const uint32_t n = w[W_N], n_ent = w[W_N_ENT], n_msgs = w[W_N_MSGS], n_agg = w[W_N_AGG];
  const uint32_t* list = (const uint32_t*)p[A_LIST];
  const uint32_t *msg_idx = (const uint32_t*)p[A_MSG_IDX], *agg_msg = (const uint32_t*)p[A_AGG_MSG];
  // the units the kernel runs, as it computes them
  uint32_t avail = n;
  if (list) {
    avail = w[W_COUNT] > w[W_BASE] ? w[W_COUNT] - w[W_BASE] : 0;
    if (avail > n) avail = n;
    if ((uint64_t)w[W_BASE] + avail > w[W_LIST_LEN]) return DB_E_ARG;
  }
  const bool pair_side = mode == P3_FULL || mode == P3_ML;          // reads pk, msg_idx, hm
  const bool sig_side = mode == P3_FULL || mode == P3_MLS || (mode == P3_FIN && p[A_SIG_LINES]);
  const bool stores_f = mode == P3_ML || mode == P3_MLS || mode == P3_MML || mode == P3_PROD;
  const bool reads_f = mode == P3_FIN || mode == P3_PROD;
  if (pair_side && (!p[A_PK] || !msg_idx || !p[A_HM])) return DB_E_ARG;
  if ((sig_side || mode == P3_MML) && !p[A_SIG_LINES]) return DB_E_ARG;
  if (stores_f && !p[A_F_OUT]) return DB_E_ARG;
  if ((mode == P3_FULL || mode == P3_FIN) && !p[A_STATUS]) return DB_E_ARG;
  if (reads_f && (!p[A_F_IN] || w[W_F_IN_LEN] < (w[W_F_N] ? w[W_F_N] : 1u))) return DB_E_ARG;
  if (mode == P3_MML && (w[W_F_RANGE] < 1 || (uint64_t)N_LINES * w[W_F_N] > w[W_N_LINES])) return DB_E_ARG;
  if (sig_side && avail && (uint64_t)(N_LINES - 1) * w[W_STRIDE] + avail > w[W_N_LINES]) return DB_E_ARG;
  for (uint32_t u = 0; u < avail; u++) {
    const uint32_t e = list ? list[w[W_BASE] + u] : u;
    if (mode == P3_FULL && e >= w[W_N_ITEMS]) {  // a folded aggregate
      const uint32_t k = e - w[W_N_ITEMS];
      if (k >= n_agg || !p[A_AGG_PK] || !agg_msg || !p[A_AGG_STATUS] || agg_msg[k] >= n_msgs) return DB_E_ARG;
    } else if (pair_side || mode == P3_FIN) {
      if (e >= n_ent || (pair_side && msg_idx[e] >= n_msgs)) return DB_E_ARG;
    }
    if (mode == P3_MML && (uint64_t)e * w[W_F_RANGE] >= w[W_F_N]) return DB_E_ARG;  // the kernel prefetches ev[first]
    if (stores_f && (uint64_t)e * (w[W_F_OUT_STRIDE] ? w[W_F_OUT_STRIDE] : 1u) + w[W_F_OUT_OFF] >= w[W_F_OUT_LEN])
      return DB_E_ARG;
  }
  DbIo io;
  Pair3Args a{};
  DB_IN(io, a.pk, p[A_PK], (size_t)n_ent * sizeof(G1AEntry));
  DB_IN(io, a.pk_st, p[A_PK_ST], n_ent);
  DB_IN(io, a.sig_st, p[A_SIG_ST], n_ent);
  DB_IN(io, a.sig_inf, p[A_SIG_INF], n_ent);
  DB_IN(io, a.msg_idx, p[A_MSG_IDX], (size_t)n_ent * 4);
  DB_IN(io, a.hm, p[A_HM], (size_t)n_msgs * sizeof(MsgEntry));
  DB_IN(io, a.sig_lines, p[A_SIG_LINES], (size_t)w[W_N_LINES] * sizeof(LineEntry));
  DB_IN(io, a.list, p[A_LIST], (size_t)w[W_LIST_LEN] * 4);
  DB_IN(io, a.count, list ? &w[W_COUNT] : nullptr, 4);
  DB_IN(io, a.agg_pk, p[A_AGG_PK], (size_t)n_agg * sizeof(G1AEntry));
  DB_IN(io, a.agg_msg, p[A_AGG_MSG], (size_t)n_agg * 4);
  DB_IN(io, a.f_in, p[A_F_IN], (size_t)w[W_F_IN_LEN] * F12);
  DB_IO(io, a.status, p[A_STATUS], n_ent);
  DB_IO(io, a.agg_status, p[A_AGG_STATUS], n_agg);
  DB_IO(io, a.f_out, p[A_F_OUT], (size_t)w[W_F_OUT_LEN] * F12);
  DB_IO(io, a.f_bad, p[A_F_BAD], n_ent);
  if (const int rc = io.guard(&a.guard, w[W_GUARD] == 2 ? -1 : (int)w[W_GUARD])) return rc;
  a.stride = w[W_STRIDE], a.n = n, a.base = w[W_BASE], a.n_items = w[W_N_ITEMS];
  a.f_range = w[W_F_RANGE], a.f_n = w[W_F_N], a.f_out_stride = w[W_F_OUT_STRIDE], a.f_out_off = w[W_F_OUT_OFF];
  switch (mode) {
    case P3_FULL: launch_pair3(a, 0); break;
    case P3_ML: launch_pair3_ml(a, 0); break;
    case P3_FIN: launch_pair3_fin(a, 0); break;
    case P3_PROD: launch_pair3_prod(a, 0); break;
    case P3_MML: launch_pair3_mml(a, 0); break;
    default: launch_pair3_mls(a, 0); break;
  }
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// k_pair6_fin<per_wave> (3: eighteen lanes per unit, 10: six) through launch_pair6_fin, which
// chooses by g_fe18_max: set for the call and restored.  f_in: f_in_len stored values (>= f_n);
// pk_st: n bytes or null; status: n bytes, in/out
extern "C" int db_pair6_fin(int per_wave, uint32_t n, uint32_t f_range, uint32_t f_n, int guard, const uint32_t* f_in,
                            uint32_t f_in_len, const uint8_t* pk_st, uint8_t* status) {
  if ((per_wave != 3 && per_wave != 10) || n < 1 || guard > 255 || !f_in || !status || f_in_len < (f_n ? f_n : 1u))
    return DB_E_ARG;
  DbIo io;
  Pair3Args a{};
  DB_IN(io, a.f_in, f_in, (size_t)f_in_len * F12);
  DB_IN(io, a.pk_st, pk_st, n);
  DB_IO(io, a.status, status, n);
  if (const int rc = io.guard(&a.guard, guard)) return rc;
  a.n = n, a.f_range = f_range, a.f_n = f_n;
  const size_t before = g_fe18_max.load();
  g_fe18_max.store(per_wave == 3 ? ~(size_t)0 : 0);
  launch_pair6_fin(a, 0);
  g_fe18_max.store(before);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// k_lml<side>.  side 0: pts, n G2JEntry.  side 1: pk (n G1AEntry), pk_st (n bytes or null), msg_idx
// (n, each below n_msgs), hm (n_msgs MsgEntry).  f_out: f_out_len stored values, in/out; bad: n bytes
// or null, in/out
extern "C" int db_lml(int side, uint32_t n, uint32_t n_msgs, const uint32_t* pts, const uint32_t* pk, const uint8_t* pk_st,
                      const uint32_t* msg_idx, const uint32_t* hm, uint32_t* f_out, uint32_t f_out_len, uint32_t f_stride,
                      uint32_t f_off, uint8_t* bad, int guard) {
  if ((side != 0 && side != 1) || n < 1 || guard > 255 || !f_out) return DB_E_ARG;
  if ((uint64_t)(n - 1) * (f_stride ? f_stride : 1u) + f_off >= f_out_len) return DB_E_ARG;
  if (side == 0 && !pts) return DB_E_ARG;
  if (side == 1) {
    if (!pk || !msg_idx || !hm || n_msgs < 1) return DB_E_ARG;
    for (uint32_t i = 0; i < n; i++)
      if (msg_idx[i] >= n_msgs) return DB_E_ARG;
  }
  DbIo io;
  LmlArgs a{};
  if (side == 0) {
    DB_IN(io, a.pts, pts, (size_t)n * sizeof(G2JEntry));
  } else {
    DB_IN(io, a.pk, pk, (size_t)n * sizeof(G1AEntry));
    DB_IN(io, a.pk_st, pk_st, n);
    DB_IN(io, a.msg_idx, msg_idx, (size_t)n * 4);
    DB_IN(io, a.hm, hm, (size_t)n_msgs * sizeof(MsgEntry));
  }
  DB_IO(io, a.f_out, f_out, (size_t)f_out_len * F12);
  DB_IO(io, a.bad, bad, n);
  if (const int rc = io.guard(&a.guard, guard)) return rc;
  a.n = n, a.f_stride = f_stride, a.f_off = f_off;
  if (side == 0) launch_lml(a.pts, n, a.f_out, f_stride, f_off, a.bad, 0, a.guard);
  else launch_lml_p(a, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}
