// TEST-ONLY device harness of the segmented first-error verification's kernels
// (tests/test_gpu_duty_first_kernels.py): this unit compiles the product's charon_amd/csrc/dutyfirst.hip
// itself and runs its launchers, one at a time, on explicit bytes.  Every output array is uploaded as
// the caller filled it, `pad` sentinel entries behind its last element included, and copied back in
// full, so that what a kernel must not write is visible to the test.  Whatever a kernel indexes with is
// checked against the arrays' sizes here, before the launch.  The product library never loads this.  A
// library and an id of its own (build.py build_dutyfirstdev).
#include "../../charon_amd/csrc/dutyfirst.hip"

#include <string.h>

#include <vector>

#include "devblocks.h"

using namespace hb;

extern "C" const char* dfd_build_id() { return DFD_BUILD_ID; }

// k_seg_first_batch, then k_seg_batch_verdict, over one chunk of ng groups that starts at group g0:
// gst (ng), bver (ceil(ng / fb)), gseg (g0 + ng: every group up to the chunk's end), guard (< 0: none).
// In/out, preset by the caller: gver, list (ng + pad each), count (1 + pad), sfirst (2 n_seg + pad).
extern "C" int dfd_batch_verdict(int ng, const uint8_t* gst, const uint8_t* bver, int guard, int fb, int g0,
                                 const uint32_t* gseg, int n_seg, int pad, uint8_t* gver, uint32_t* list, uint32_t* count,
                                 uint32_t* sfirst) {
  if (ng < 1 || fb < 1 || g0 < 0 || n_seg < 0 || pad < 0 || !gst || !bver || !gseg || !gver || !list || !count || !sfirst)
    return DB_E_ARG;
  DbIo io;
  const uint8_t *dgst, *dbver, *dguard;
  const uint32_t* dgseg;
  uint8_t* dgver;
  uint32_t *dlist, *dcount, *dsf;
  DB_IN(io, dgst, gst, (size_t)ng);
  DB_IN(io, dbver, bver, (size_t)(ng + fb - 1) / fb);
  DB_IN(io, dgseg, gseg, ((size_t)g0 + ng) * 4);
  if (const int rc = io.guard(&dguard, guard)) return rc;
  DB_IO(io, dgver, gver, (size_t)ng + pad);
  DB_IO(io, dlist, list, ((size_t)ng + pad) * 4);
  DB_IO(io, dcount, count, ((size_t)1 + pad) * 4);
  DB_IO(io, dsf, sfirst, (2 * (size_t)n_seg + pad) * 4);
  launch_seg_batch_verdict(dgst, dbver, (uint32_t)ng, dgver, dlist, dcount, 0, dguard, (uint32_t)fb, (uint32_t)g0, dgseg,
                           (uint32_t)n_seg, dsf);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// k_seg_first_group over the call's n_groups verdicts; sfirst (2 n_seg + pad) preset by the caller
extern "C" int dfd_first_group(int n_groups, const uint8_t* gver, const uint32_t* gseg, int n_seg, int pad, uint32_t* sfirst) {
  if (n_groups < 1 || n_seg < 0 || pad < 0 || !gver || !gseg || !sfirst) return DB_E_ARG;
  DbIo io;
  const uint8_t* dgver;
  const uint32_t* dgseg;
  uint32_t* dsf;
  DB_IN(io, dgver, gver, (size_t)n_groups);
  DB_IN(io, dgseg, gseg, (size_t)n_groups * 4);
  DB_IO(io, dsf, sfirst, (2 * (size_t)n_seg + pad) * 4);
  launch_seg_first_group(dgver, (uint32_t)n_groups, dgseg, (uint32_t)n_seg, dsf, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// k_seg_scatter over n items: their groups (< n_groups), messages (< n_msgs), the infinity flags of
// their keys, signatures and hashed messages, their decoding statuses; the groups' verdicts, offsets
// (nullable) and segments; sfirst (2 n_seg, at least one pair).  In/out, preset: status, list (n + pad),
// count (1 + pad).
extern "C" int dfd_scatter(int n, const uint32_t* item_grp, const uint32_t* msg_idx, int n_msgs, const uint8_t* hm_inf,
                           const uint8_t* pk_inf, const uint8_t* pk_st, const uint8_t* sig_inf, const uint8_t* sig_st,
                           int n_groups, const uint8_t* gver, const uint32_t* grp_off, const uint32_t* gseg, int n_seg,
                           const uint32_t* sfirst, int pad, uint8_t* status, uint32_t* list, uint32_t* count) {
  if (n < 1 || n_msgs < 1 || n_groups < 1 || n_seg < 0 || pad < 0 || !item_grp || !msg_idx || !hm_inf || !pk_inf || !pk_st ||
      !sig_inf || !sig_st || !gver || !gseg || !sfirst || !status || !list || !count)
    return DB_E_ARG;
  for (int i = 0; i < n; i++)
    if (item_grp[i] >= (uint32_t)n_groups || msg_idx[i] >= (uint32_t)n_msgs) return DB_E_ARG;
  std::vector<G1AEntry> pk(n);
  std::vector<HmEntry> sig(n);
  std::vector<MsgEntry> hm(n_msgs);
  memset(pk.data(), 0, pk.size() * sizeof(G1AEntry));
  memset(sig.data(), 0, sig.size() * sizeof(HmEntry));
  memset(hm.data(), 0, hm.size() * sizeof(MsgEntry));
  for (int i = 0; i < n; i++) {
    pk[i].inf = pk_inf[i];
    sig[i].inf = sig_inf[i];
  }
  for (int j = 0; j < n_msgs; j++) hm[j].h.inf = hm_inf[j];
  DbIo io;
  ScatterArgs a{};
  const uint32_t *dgseg, *dsf;
  DB_IN(io, a.item_grp, item_grp, (size_t)n * 4);
  DB_IN(io, a.msg_idx, msg_idx, (size_t)n * 4);
  DB_IN(io, a.hm, hm.data(), hm.size() * sizeof(MsgEntry));
  DB_IN(io, a.pk, pk.data(), pk.size() * sizeof(G1AEntry));
  DB_IN(io, a.pk_st, pk_st, (size_t)n);
  DB_IN(io, a.sig, sig.data(), sig.size() * sizeof(HmEntry));
  DB_IN(io, a.sig_st, sig_st, (size_t)n);
  DB_IN(io, a.gverdict, gver, (size_t)n_groups);
  DB_IN(io, a.grp_off, grp_off, ((size_t)n_groups + 1) * 4);
  DB_IN(io, dgseg, gseg, (size_t)n_groups * 4);
  DB_IN(io, dsf, sfirst, 2 * (size_t)(n_seg ? n_seg : 1) * 4);
  DB_IO(io, a.status, status, (size_t)n + pad);
  DB_IO(io, a.list, list, ((size_t)n + pad) * 4);
  DB_IO(io, a.count, count, ((size_t)1 + pad) * 4);
  a.n = (uint32_t)n;
  launch_seg_scatter(a, dgseg, (uint32_t)n_seg, dsf, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// k_seg_first_item over n items; set_first (n_seg + pad) preset by the caller
extern "C" int dfd_first_item(int n, const uint8_t* status, const uint32_t* item_seg, const uint32_t* arrival, int n_seg,
                              int pad, uint32_t* set_first) {
  if (n < 1 || n_seg < 0 || pad < 0 || !status || !item_seg || !arrival || !set_first) return DB_E_ARG;
  DbIo io;
  const uint8_t* dst;
  const uint32_t *dseg, *darr;
  uint32_t* dsf;
  DB_IN(io, dst, status, (size_t)n);
  DB_IN(io, dseg, item_seg, (size_t)n * 4);
  DB_IN(io, darr, arrival, (size_t)n * 4);
  DB_IO(io, dsf, set_first, ((size_t)n_seg + pad) * 4);
  launch_seg_first_item(dst, dseg, darr, (uint32_t)n, dsf, (uint32_t)n_seg, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}
