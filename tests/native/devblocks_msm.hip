// TEST-ONLY device block harness, the slot-wide bucket MSM: this unit compiles the product's
// charon_amd/csrc/msm.hip itself (its kernels and launch_msm_* as the library has them) and runs
// launch_msm_count, an exclusive scan, launch_msm_fill, launch_msm_bucket, launch_msm_reduce and
// launch_msm_sum on explicit HmEntry points, statuses, group states and uint2 coefficients,
// returning total[0] -- the sum S that the product only ever compares inside a pairing product.
// The scan runs on the HOST here (counts copied back, offsets copied up): vbatch.hip's launch_scan
// is not linked.  tests/test_gpu_curve.py compares S with the oracle.  A unit of the curve harness
// (devblocks_curve.hip), built with fp.h's default HB_ARG_LANES as msm.hip in the library.
#include "../../charon_amd/csrc/msm.hip"

#include "devblocks.h"

#include <vector>

using namespace hb;

extern "C" int db_msm_keys() { return (int)MSM_KEYS; }
extern "C" int db_msm_chunk() { return (int)MSM_CHUNK; }

// sig: n HmEntry; agg_sig: n_agg HmEntry (group i - n); coef: n + n_agg pairs (a, b); igrp: n;
// gst: n_groups (>= n_agg, > every igrp); total: one G2JEntry (72 words)
extern "C" int db_msm(int n, int n_agg, int n_groups, const uint32_t* sig, const uint8_t* sig_st, const uint32_t* agg_sig,
                      const uint8_t* agg_st, const uint32_t* coef, const uint32_t* igrp, const uint8_t* gst,
                      uint32_t* total) {
  static_assert(sizeof(HmEntry) == 52 * 4 && sizeof(G2JEntry) == 72 * 4, "raw-word layouts of layout.h");
  if (n < 0 || n_agg < 0 || n + n_agg < 1 || n_groups < 1 || n_agg > n_groups || !sig || !sig_st || !agg_sig || !agg_st ||
      !coef || !igrp || !gst || !total)
    return DB_E_ARG;
  for (int i = 0; i < n; i++)
    if (igrp[i] >= (uint32_t)n_groups) return DB_E_ARG;
  const size_t items = (size_t)n + n_agg;
  DbDev in, ws;  // eight buffers each
  G2MsmArgs a{};
  HmEntry *dsig, *dagg;
  uint8_t *dsst, *dast, *dgst;
  uint2* dcoef;
  uint32_t* digrp;
  DB_MAKE(in, dsig, sig, (size_t)n * sizeof(HmEntry));
  DB_MAKE(in, dsst, sig_st, (size_t)n);
  DB_MAKE(in, dagg, agg_sig, (size_t)n_agg * sizeof(HmEntry));
  DB_MAKE(in, dast, agg_st, (size_t)n_agg);
  DB_MAKE(in, dcoef, coef, items * sizeof(uint2));
  DB_MAKE(in, digrp, igrp, (size_t)n * 4);
  DB_MAKE(in, dgst, gst, (size_t)n_groups);
  a.sig = dsig, a.sig_st = dsst, a.agg_sig = dagg, a.agg_st = dast, a.coef = dcoef, a.igrp = digrp, a.gst = dgst;
  a.n = (uint32_t)n, a.n_agg = (uint32_t)n_agg;
  DB_MAKE(ws, a.cnt, nullptr, MSM_KEYS * 4);
  DB_MAKE(ws, a.off, nullptr, (MSM_KEYS + 1) * 4);
  DB_MAKE(ws, a.cur, nullptr, MSM_KEYS * 4);
  DB_MAKE(ws, a.ent, nullptr, 2 * MSM_WINDOWS * items * 4);
  DB_MAKE(ws, a.order, nullptr, MSM_KEYS * 4);
  DB_MAKE(ws, a.bucket, nullptr, MSM_KEYS * sizeof(G2JEntry));
  DB_MAKE(ws, a.part, nullptr, MSM_PARTS * sizeof(G2JEntry));
  DB_MAKE(in, a.part2, nullptr, (MSM_PARTS / 128 + 1) * sizeof(G2JEntry));  // part2 [MSM_PARTS / 128], then total
  a.total = a.part2 + MSM_PARTS / 128;
  launch_msm_count(a, 0);
  if (const int rc = db_finish()) return rc;
  std::vector<uint32_t> cnt(MSM_KEYS), off(MSM_KEYS + 1);
  if (const int rc = db_fetch(cnt.data(), a.cnt, MSM_KEYS * 4)) return rc;
  uint64_t run = 0;
  for (uint32_t k = 0; k < MSM_KEYS; k++) {
    off[k] = (uint32_t)run;
    run += cnt[k];
  }
  off[MSM_KEYS] = (uint32_t)run;
  if (run > 2 * MSM_WINDOWS * items) return DB_E_ARG;  // more entries than `ent` holds: never written
  if (hipMemcpy(a.off, off.data(), (MSM_KEYS + 1) * 4, hipMemcpyHostToDevice) != hipSuccess) return DB_E_UPLOAD;
  launch_msm_fill(a, 0);
  if (const int rc = db_finish()) return rc;
  launch_msm_bucket(a, 0);
  if (const int rc = db_finish()) return rc;
  launch_msm_reduce(a, 0);
  if (const int rc = db_finish()) return rc;
  launch_msm_sum(a, 0);
  if (const int rc = db_finish()) return rc;
  return db_fetch(total, a.total, sizeof(G2JEntry));
}
