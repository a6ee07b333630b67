// TEST-ONLY device harness of hbls_duty_add_sets' kernels (tests/test_gpu_duty_sets_kernels.py): this
// unit compiles the product's charon_amd/csrc/duty.hip itself and runs launch_duty_set_first,
// launch_duty_gate and, behind the gate, launch_duty_store on explicit words.  Every output array is
// uploaded as the caller filled it, `pad` sentinel entries behind its last element included, and
// copied back in full, so that what a kernel must not write is visible to the test.  The product
// library never loads this.  A library and an id of its own (build.py build_dutysetdev).
#include "../../charon_amd/csrc/duty.hip"

#include <vector>

#include "devblocks.h"

using namespace hb;

extern "C" const char* dsd_build_id() { return DSD_BUILD_ID; }

// set_first: n_sets + pad words, preset by the caller (0xffffffff, then its sentinels)
extern "C" int dsd_set_first(int n, const uint8_t* vstatus, const uint32_t* set_id, const uint32_t* arrival, int n_sets,
                             int pad, uint32_t* set_first) {
  if (n < 1 || n_sets < 0 || pad < 0 || !vstatus || !set_id || !arrival || !set_first) return DB_E_ARG;
  DbIo io;
  const uint8_t* dv;
  const uint32_t *dsid, *darr;
  uint32_t* dsf;
  DB_IN(io, dv, vstatus, (size_t)n);
  DB_IN(io, dsid, set_id, (size_t)n * 4);
  DB_IN(io, darr, arrival, (size_t)n * 4);
  DB_IO(io, dsf, set_first, ((size_t)n_sets + pad) * 4);
  launch_duty_set_first(dv, dsid, darr, (uint32_t)n, dsf, (uint32_t)n_sets, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// set_first: n_sets words (at least one); admit: n + pad bytes, preset by the caller
extern "C" int dsd_gate(int n, const uint8_t* vstatus, const uint32_t* set_id, const uint32_t* set_first, int n_sets, int pad,
                        uint8_t* admit) {
  if (n < 1 || n_sets < 0 || pad < 0 || !vstatus || !set_id || !set_first || !admit) return DB_E_ARG;
  DbIo io;
  const uint8_t* dv;
  const uint32_t *dsid, *dsf;
  uint8_t* dad;
  DB_IN(io, dv, vstatus, (size_t)n);
  DB_IN(io, dsid, set_id, (size_t)n * 4);
  DB_IN(io, dsf, set_first, (size_t)(n_sets ? n_sets : 1) * 4);
  DB_IO(io, dad, admit, (size_t)n + pad);
  launch_duty_gate(dv, dsid, (uint32_t)n, dsf, (uint32_t)n_sets, dad, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}

// k_duty_store behind the gate: the n items' verdicts, set ids, message ids and serials; the sets'
// verdicts; the n_touched groups' CSR over n_pos partials; the shard's records (n_groups x max_stored,
// count and fired per group), updated in place.  Out, each with `pad` sentinel entries behind it:
// admit, stored, slot (n), mserial (n_touched x t), copies (n pairs), fired_u (n_touched), ctr
// (DUTY_CTRS).  mslot / midx / fmsg / fkey are scratch here.
extern "C" int dsd_store(int n, const uint8_t* vstatus, const uint32_t* set_id, const uint32_t* set_first, int n_sets,
                         const uint32_t* msg_idx, const uint32_t* serial, int n_touched, int n_pos, const uint32_t* tgroup,
                         const uint32_t* toff, const uint32_t* tpos, const int64_t* tidx, int n_groups, int max_stored, int t,
                         int64_t* rec_idx, uint32_t* rec_msg, uint32_t* rec_serial, uint32_t* count, uint8_t* fired, int pad,
                         uint8_t* admit, uint8_t* stored, uint32_t* slot, uint32_t* mserial, uint32_t* copies,
                         uint32_t* fired_u, uint32_t* ctr) {
  if (n < 1 || n_sets < 0 || n_touched < 1 || n_pos < 1 || n_groups < 1 || pad < 0) return DB_E_ARG;
  if (max_stored < 1 || max_stored > (int)DUTY_MAX_STORED || t < 1 || t > (int)DUTY_MAX_T) return DB_E_ARG;
  if (!vstatus || !set_id || !set_first || !msg_idx || !serial || !tgroup || !toff || !tpos || !tidx || !rec_idx || !rec_msg ||
      !rec_serial || !count || !fired || !admit || !stored || !slot || !mserial || !copies || !fired_u || !ctr)
    return DB_E_ARG;
  DbIo io;
  DutyStoreArgs a{};
  const uint8_t* dv;
  const uint32_t *dsid, *dsf;
  uint8_t* dad;
  const size_t slots = (size_t)n_groups * max_stored, mt = (size_t)n_touched * t;
  std::vector<uint32_t> z32(mt, 0);
  std::vector<int64_t> z64(mt, 0);
  DB_IN(io, dv, vstatus, (size_t)n);
  DB_IN(io, dsid, set_id, (size_t)n * 4);
  DB_IN(io, dsf, set_first, (size_t)(n_sets ? n_sets : 1) * 4);
  DB_IN(io, a.msg_idx, msg_idx, (size_t)n * 4);
  DB_IN(io, a.serial, serial, (size_t)n * 4);
  DB_IN(io, a.tgroup, tgroup, (size_t)n_touched * 4);
  DB_IN(io, a.toff, toff, ((size_t)n_touched + 1) * 4);
  DB_IN(io, a.tpos, tpos, (size_t)n_pos * 4);
  DB_IN(io, a.tidx, tidx, (size_t)n_pos * 8);
  DB_IN(io, a.mslot, z32.data(), mt * 4);
  DB_IN(io, a.midx, z64.data(), mt * 8);
  DB_IN(io, a.fmsg, z32.data(), (size_t)n_touched * 4);
  DB_IN(io, a.fkey, z32.data(), (size_t)n_touched * 4);
  DB_IO(io, a.rec_idx, rec_idx, (slots + pad) * 8);
  DB_IO(io, a.rec_msg, rec_msg, (slots + pad) * 4);
  DB_IO(io, a.rec_serial, rec_serial, (slots + pad) * 4);
  DB_IO(io, a.count, count, ((size_t)n_groups + pad) * 4);
  DB_IO(io, a.fired, fired, (size_t)n_groups + pad);
  DB_IO(io, dad, admit, (size_t)n + pad);
  DB_IO(io, a.stored, stored, (size_t)n + pad);
  DB_IO(io, a.slot, slot, ((size_t)n + pad) * 4);
  DB_IO(io, a.mserial, mserial, (mt + pad) * 4);
  DB_IO(io, a.copies, copies, ((size_t)n + pad) * 8);
  DB_IO(io, a.fired_u, fired_u, ((size_t)n_touched + pad) * 4);
  DB_IO(io, a.ctr, ctr, ((size_t)DUTY_CTRS + pad) * 4);
  a.n_groups = (uint32_t)n_groups;
  a.max_stored = (uint32_t)max_stored;
  a.t = (uint32_t)t;
  a.vstatus = dad;
  a.n = (uint32_t)n;
  a.n_touched = (uint32_t)n_touched;
  a.n_pos = (uint32_t)n_pos;
  launch_duty_gate(dv, dsid, (uint32_t)n, dsf, (uint32_t)n_sets, dad, 0);
  if (const int rc = db_finish()) return rc;
  launch_duty_store(a, 0);
  if (const int rc = db_finish()) return rc;
  return io.fetch();
}
