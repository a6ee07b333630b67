// TEST-ONLY: what the two translation units of the device block harness share (devblocks_leaf.hip,
// devblocks_grp.hip): the product headers included exactly as the product's fast translation units
// include them, and the checked allocate / copy / launch / synchronise / copy-back helpers.
//
// The harness is built twice (charon_amd/build.py build_devblocks): with fp.h's default
// HB_ARG_LANES (64: vbatch.hip, threshold.hip, msm.hip, hashsplit.hip) and with -DHB_ARG_LANES=128
// (pipeline.hip).  In the 128 build the leaf kernels run 128-thread workgroups, so wave 1 uses the
// LDS argument slots 64..127 (pipeline.hip k_lml's consumer wave).
//
// A unit that defines DB_STD_CONVENTION first (devblocks_h2c_std.hip) gets the product headers as
// hash.hip includes them instead: no HB_FAST_FPMUL, the building blocks separate functions.
#pragma once
#if defined(DB_STD_CONVENTION)
#include "../../charon_amd/csrc/layout.h"
#else
#define HB_FAST_FPMUL 1
#include "../../charon_amd/csrc/lines.h"
#include "../../charon_amd/csrc/pair3.h"
#include "../../charon_amd/csrc/pair6.h"
#endif

// threads per workgroup of the leaf kernels: the build's HB_ARG_LANES (fp.h defines its default in
// the device pass only, so the default is named here for the host pass and compared below)
#if defined(HB_ARG_LANES)
#define DB_BLOCK HB_ARG_LANES
#else
#define DB_BLOCK 64
#endif
#if defined(__HIP_DEVICE_COMPILE__)
static_assert(DB_BLOCK == HB_ARG_LANES, "one LDS argument slot per thread of a workgroup");
#endif

// Return codes of every entry point: 0, or the first failing step
enum {
  DB_E_ARG = -1,     // n < 1, a null pointer
  DB_E_ALLOC = -2,   // hipMalloc
  DB_E_UPLOAD = -3,  // hipMemcpy host -> device
  DB_E_CLEAR = -4,   // hipMemset of the output
  DB_E_LAUNCH = -5,  // the launch itself (hipGetLastError)
  DB_E_SYNC = -6,    // hipDeviceSynchronize: the kernel's own error
  DB_E_DOWNLOAD = -7,  // hipMemcpy device -> host
  DB_E_OP = -10,     // no such operation (for this lane group)
};

struct DbDev {  // device buffers of one call, freed when it returns
  void* p[8] = {};
  int n = 0;
  ~DbDev() {
    for (int i = 0; i < n; i++) (void)hipFree(p[i]);
  }
  // a device copy of `bytes` bytes of src (src == nullptr: zero-filled)
  int make(void** out, const void* src, size_t bytes) {
    if (n >= 8) return DB_E_ARG;
    if (hipMalloc(out, bytes ? bytes : 4) != hipSuccess) return DB_E_ALLOC;
    p[n++] = *out;
    if (src) {
      if (bytes && hipMemcpy(*out, src, bytes, hipMemcpyHostToDevice) != hipSuccess) return DB_E_UPLOAD;
    } else if (bytes && hipMemset(*out, 0, bytes) != hipSuccess) {
      return DB_E_CLEAR;
    }
    return 0;
  }
};
#define DB_MAKE(dev, ptr, src, bytes)                                   \
  do {                                                                  \
    const int db_rc_ = (dev).make((void**)&(ptr), (src), (bytes));      \
    if (db_rc_) return db_rc_;                                          \
  } while (0)

// The buffers of a call that has more than eight (the pair harness: a whole argument struct of the
// product): device copies of host arrays -- a null array stays a null device pointer -- and the
// in/out ones, uploaded as the caller filled them (a sentinel pattern) and copied back IN FULL by
// fetch(), so that what a kernel must not write is visible to the caller.
struct DbIo {
  DbDev dev[4];
  struct Out {
    void *host, *devp;
    size_t bytes;
  } outs[12];
  int n = 0, n_out = 0;
  int in(void** out, const void* src, size_t bytes) {
    *out = nullptr;
    if (!src) return 0;
    if (n >= 32) return DB_E_ARG;
    return dev[n++ / 8].make(out, src, bytes);
  }
  int io(void** out, void* host, size_t bytes) {
    if (host && n_out >= 12) return DB_E_ARG;
    const int rc = in(out, host, bytes);
    if (!rc && host) outs[n_out++] = {host, *out, bytes};
    return rc;
  }
  // guard < 0: no guard byte (null); else a device byte of that value
  int guard(const uint8_t** out, int g) {
    const uint8_t b = (uint8_t)g;
    return in((void**)out, g < 0 ? nullptr : &b, 1);
  }
  int fetch() {
    for (int i = 0; i < n_out; i++)
      if (outs[i].bytes && hipMemcpy(outs[i].host, outs[i].devp, outs[i].bytes, hipMemcpyDeviceToHost) != hipSuccess)
        return DB_E_DOWNLOAD;
    return 0;
  }
};
#define DB_IN(io_, ptr, src, bytes)                                     \
  do {                                                                  \
    const int db_rc_ = (io_).in((void**)&(ptr), (src), (bytes));        \
    if (db_rc_) return db_rc_;                                          \
  } while (0)
#define DB_IO(io_, ptr, host, bytes)                                    \
  do {                                                                  \
    const int db_rc_ = (io_).io((void**)&(ptr), (host), (bytes));       \
    if (db_rc_) return db_rc_;                                          \
  } while (0)

// every message i = (off[i], len[i]) inside an uploaded buffer of msgs_bytes bytes
static inline bool db_ranges_ok(int n, size_t msgs_bytes, const uint64_t* off, const uint32_t* len) {
  for (int i = 0; i < n; i++)
    if (off[i] > msgs_bytes || (uint64_t)len[i] > msgs_bytes - off[i]) return false;
  return true;
}

static inline int db_finish() {  // after the launch
  if (hipGetLastError() != hipSuccess) return DB_E_LAUNCH;
  if (hipDeviceSynchronize() != hipSuccess) return DB_E_SYNC;
  return 0;
}
static inline int db_fetch(void* dst, const void* src, size_t bytes) {
  return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : DB_E_DOWNLOAD;
}
