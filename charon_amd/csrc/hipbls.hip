// libhipbls.so: gfx950 kernels + C ABI (include/hipbls.h) for charon's BLS hot path.
//
// Reference interface replaced: tbls.Implementation (/root/reference/tbls/tbls.go:27-69) as
// implemented by tbls.Herumi (/root/reference/tbls/herumi.go).  This file holds the one-lane
// kernels of the cold entry points (Sign, SecretToPublicKey, split/recover, group sums) and the
// host runtime: per-device contexts (one process may drive every GPU in its device mask),
// workspace sets ordered by events, the batched verification pipeline, a coalescing queue for
// concurrent callers (charon calls tbls.Verify from one goroutine per libp2p stream,
// p2p/receive.go:52) and the RCCL exchange of slot results between processes.
#include "layout.h"
#include "../../include/hipbls.h"
#include "cluster.h"
#include "clustersel.h"
#include "coalesce.h"
#include "dutysel.h"
#include "hduty.h"
#include "hgroup.h"
#include "hslot.h"
#include "msgtable.h"
#include "vplan.h"

#include <rccl/rccl.h>
#include <sys/random.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <string.h>
#include <thread>
#include <unordered_map>
#include <vector>

using namespace hb;

#define KERNEL_BOUNDS __launch_bounds__(64)
constexpr int BLOCK = 64;

// ---------------------------------------------------------------------------------------
// One-lane kernels (standard calling convention product: code size over speed)
// ---------------------------------------------------------------------------------------

// One lane per group: sum the member points, compress (herumi Sign.Recover / Sign.Aggregate +
// Serialize).  Status precedence follows herumi: any undecodable partial -> BAD_SIGNATURE
// (deserialisation happens first, herumi.go:255-264), then combine failure.  agg_pt (nullable):
// the affine result, for the folded post-aggregate verification of the slot entry point.
//
// Invariant the slot path relies on: a group with a member whose status is M_BAD_SIG never uses
// its ladders' outputs (pts) -- it is zeroed here whatever they hold.  In hbls_slot_device the
// aggregation ladders start once the partials are decoded (ev_dec) and only the Lagrange digits
// wait for the subgroup statuses (mst_ready), so k_g2_subgroup may overwrite a failing member's
// point with infinity while a ladder reads it; such a member's status is M_BAD_SIG by the time
// this kernel runs (it is ordered after mst_ready), so the raced values are never published.
__global__ KERNEL_BOUNDS void k_group_sum(const uint32_t* __restrict__ grp_off, uint32_t n_groups, int mode,
                                          const G2JEntry* __restrict__ pts, const uint8_t* __restrict__ mstat,
                                          uint8_t* __restrict__ out, uint8_t* __restrict__ status,
                                          HmEntry* __restrict__ agg_pt) {
  uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_groups) return;
  uint32_t b = grp_off[g], e = grp_off[g + 1];
  uint8_t st = ST_OK;
  if (e == b && mode == 0) st = ST_COMBINE_FAILED;  // Recover of an empty set fails
  for (uint32_t m = b; m < e; m++) {
    if (mstat[m] == M_BAD_SIG) st = ST_BAD_SIGNATURE;
  }
  if (st == ST_OK) {
    for (uint32_t m = b; m < e; m++)
      if (mstat[m] == M_BAD_IDX) st = ST_COMBINE_FAILED;
  }
  uint8_t* o = out + 96ull * g;
  if (st != ST_OK) {
    for (int k = 0; k < 96; k++) o[k] = 0;
    status[g] = st;
    if (agg_pt) agg_pt[g].inf = 1;
    return;
  }
  G2J acc = jac_infinity<Fp2>();
  for (uint32_t m = b; m < e; m++) {
    G2JEntry q = pts[m];
    acc = jac_add(acc, G2J{q.X, q.Y, q.Z});
  }
  const G2A a = jac_to_aff(acc);
  uint8_t buf[96];
  g2_compress(buf, a);
  for (int k = 0; k < 96; k++) o[k] = buf[k];
  status[g] = ST_OK;
  if (agg_pt) {
    HmEntry h;
    h.x = a.x;
    h.y = a.y;
    h.inf = a.inf ? 1u : 0u;
    h.pad[0] = h.pad[1] = h.pad[2] = 0;
    agg_pt[g] = h;
  }
}

// Sign: one lane per (sk, message): sigma = sk * H(m)   (herumi.go:306-316)
__global__ KERNEL_BOUNDS void k_sign(const uint8_t* __restrict__ sks, const uint32_t* __restrict__ msg_idx,
                                     const MsgEntry* __restrict__ hm, uint32_t n, uint8_t* __restrict__ sigs,
                                     uint8_t* __restrict__ status) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint8_t skb[32];
  for (int k = 0; k < 32; k++) skb[k] = sks[32ull * i + k];
  Fr s;
  uint8_t buf[96];
  if (!fr_from_be(s, skb)) {
    status[i] = ST_BAD_SECRET;
    for (int k = 0; k < 96; k++) sigs[96ull * i + k] = 0;
    return;
  }
  G2J sg = jac_mul_aff(hm_load(hm[msg_idx[i]].h), s.v, 255);
  g2_compress(buf, jac_to_aff<Fp2, true>(sg));  // secret-dependent: fixed-trip inversion
  for (int k = 0; k < 96; k++) sigs[96ull * i + k] = buf[k];
  status[i] = ST_OK;
}

// SecretToPublicKey: pk = sk * g1 (herumi.go:66-79; GetSafePublicKey rejects sk = 0)
__global__ KERNEL_BOUNDS void k_sk_to_pk(const uint8_t* __restrict__ sks, uint32_t n, uint8_t* __restrict__ pks,
                                         uint8_t* __restrict__ status) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint8_t skb[32];
  for (int k = 0; k < 32; k++) skb[k] = sks[32ull * i + k];
  Fr s;
  uint8_t buf[48];
  if (!fr_from_be(s, skb) || fr_is_zero(s)) {
    status[i] = ST_BAD_SECRET;
    for (int k = 0; k < 48; k++) pks[48ull * i + k] = 0;
    return;
  }
  G1J p = jac_mul_aff(g1_generator(), s.v, 255);
  g1_compress(buf, jac_to_aff<Fp, true>(p));  // secret-dependent: fixed-trip inversion
  for (int k = 0; k < 48; k++) pks[48ull * i + k] = buf[k];
  status[i] = ST_OK;
}

// ThresholdSplit core: share i = f(i), f(z) = secret + sum coeffs[k-1] z^k over Fr.
__global__ KERNEL_BOUNDS void k_split(const uint8_t* __restrict__ poly, uint32_t threshold, uint32_t total,
                                      uint8_t* __restrict__ shares, uint8_t* __restrict__ status) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  Fr x = fr_from_i64((int64_t)i + 1);
  Fr acc = fr_zero();
  for (int k = (int)threshold - 1; k >= 0; k--) {
    Fr c;
    if (!fr_from_be(c, poly + 32ull * k)) {
      status[i] = ST_BAD_SECRET;
      return;
    }
    acc = fr_add(fr_mul(acc, x), fr_to_mont(c));
  }
  fr_to_be(shares + 32ull * i, fr_from_mont(acc));
  status[i] = ST_OK;
}

// RecoverSecret: single lane (k small), Lagrange at 0 over Fr.
__global__ void k_recover(const uint8_t* __restrict__ shares, const int64_t* __restrict__ idx, uint32_t k,
                          uint8_t* __restrict__ out, uint8_t* __restrict__ status) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  Fr acc = fr_zero();
  for (uint32_t i = 0; i < k; i++) {
    Fr si;
    if (!fr_from_be(si, shares + 32ull * i)) {
      status[0] = ST_BAD_SECRET;
      return;
    }
    Fr lam = fr_one();
    if (k > 1) {
      Fr xi = fr_from_i64(idx[i]);
      Fr num = fr_one(), den = fr_one();
      for (uint32_t m = 0; m < k; m++) {
        if (m == i) continue;
        Fr xm = fr_from_i64(idx[m]);
        num = fr_mul(num, xm);
        den = fr_mul(den, fr_sub(xm, xi));
      }
      if (fr_is_zero(num) || fr_is_zero(den)) {
        status[0] = ST_COMBINE_FAILED;
        return;
      }
      lam = fr_mul(num, fr_inv(den));
    }
    acc = fr_add(acc, fr_mul(lam, fr_to_mont(si)));
  }
  if (k == 0) {
    status[0] = ST_COMBINE_FAILED;
    return;
  }
  fr_to_be(out, fr_from_mont(acc));
  status[0] = ST_OK;
}

// ---------------------------------------------------------------------------------------
// Host runtime
// ---------------------------------------------------------------------------------------
namespace {

thread_local std::string g_err;

int set_err(const std::string& what) {
  g_err = what;
  return -1;
}
int set_err(const char* what, hipError_t e) { return set_err(std::string(what) + ": " + hipGetErrorString(e)); }

#define HCHK(expr)                                         \
  do {                                                     \
    hipError_t _e = (expr);                                \
    if (_e != hipSuccess) return set_err(#expr, _e);       \
  } while (0)

inline unsigned blocks_for(size_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

// Host-buffer Verify on one device: the caller's keys and signatures go up as they are, and the
// device puts them in group order (one lane per item: 48 + 96 bytes as 16-byte words) and the
// statuses back in the caller's order -- no host-side copy of the 144 bytes per item.
__global__ KERNEL_BOUNDS void k_gather_items(const uint4* __restrict__ pk_in, const uint4* __restrict__ sig_in,
                                             const uint32_t* __restrict__ order, uint32_t n, uint4* __restrict__ pk_out,
                                             uint4* __restrict__ sig_out) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const uint32_t i = order[k];
  HB_UNROLL for (int w = 0; w < 3; w++) pk_out[3ull * k + w] = pk_in[3ull * i + w];
  HB_UNROLL for (int w = 0; w < 6; w++) sig_out[6ull * k + w] = sig_in[6ull * i + w];
}
__global__ KERNEL_BOUNDS void k_scatter_status(const uint8_t* __restrict__ st_in, const uint32_t* __restrict__ order,
                                               uint32_t n, uint8_t* __restrict__ st_out) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) st_out[order[k]] = st_in[k];
}

// the verify bitmap of a slot (bit i of byte i / 8, least significant first: status[i] == OK): one
// ballot per wave, eight bytes per wave -- what the ranks all-gather
__global__ KERNEL_BOUNDS void k_status_bitmap(const uint8_t* __restrict__ st, uint32_t n, uint8_t* __restrict__ bits) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t m = __ballot(i < n && st[i] == ST_OK);
  const uint32_t lane = threadIdx.x & 63u, first = i - lane;  // the wave's first item (a multiple of 64)
  if (lane < 8 && first + 8 * lane < n) bits[first / 8 + lane] = (uint8_t)(m >> (8 * lane));
}

#define LAUNCH(kern, n, stream, ...)                                                              \
  do {                                                                                            \
    if ((n) > 0) {                                                                                \
      hipLaunchKernelGGL(kern, dim3(blocks_for(n)), dim3(BLOCK), 0, (stream), __VA_ARGS__);       \
      HCHK(hipGetLastError());                                                                    \
    }                                                                                             \
  } while (0)

size_t env_size(const char* name, size_t dflt) {
  const char* v = getenv(name);
  if (!v || !*v) return dflt;
  char* end = nullptr;
  unsigned long long x = strtoull(v, &end, 0);
  return (end && *end == 0) ? (size_t)x : dflt;
}

// Verification groups are chunked for the line buffers: GCAP groups per pairing launch, FB_CAP
// fallback items per pass (HBLS_GROUP_CHUNK / HBLS_FALLBACK_CHUNK).  Host-buffer calls build
// groups of at most GMAX items over one message (HBLS_GROUP_MAX).
std::atomic<size_t> g_gcap{131072}, g_fbcap{65536}, g_gmax{16};
std::atomic<size_t> g_rlc_lanes{65536};   // HBLS_RLC_LANES: lanes the chunk size aims to keep busy
// public-key cache: compressed key -> entry index (the same on every device).  Lock order: an
// adder (or clear) takes g_kc_add_mu, then one Dev::mu at a time to fill that device's table, then
// g_kc_mu to publish; verifications hold their Dev::mu and take g_kc_mu for the lookup.  g_kc_mu is
// always the innermost lock, so adds and verifications never wait on each other in a cycle.  A
// lookup made under a Dev::mu stays valid for everything enqueued while it is held: entries are
// only written under it, and kc_fill first waits for every launch already enqueued on the device
// (which covers indices reused after hbls_pubkey_cache_clear).
std::mutex g_kc_add_mu;
std::mutex g_kc_mu;
std::unordered_map<std::string, uint32_t> g_kc_map;
size_t g_kc_n = 0;             // published entries (g_kc_mu; written under g_kc_add_mu too)
std::vector<uint8_t> g_kc_keys;  // their compressed bytes, 48 B each (g_kc_add_mu): fills new devices
// HBLS_TA_JOINT: members per lane of the joint aggregation ladders (k_ta_jtab, k_ta_jladder, k_ta_jgeneral) when every group has
// the same size t; 0 = auto (about TA_JOINT_LANES lanes, at most t and 8), 1 = one ladder per member
// (k_ta_straus)
std::atomic<size_t> g_ta_joint{0};
constexpr size_t TA_JOINT_LANES = 98304;
// HBLS_FE_BATCH: verifications of at least this many groups check FE_BATCH groups per final
// exponentiation (vgroup.hip; 0 = one final exponentiation per group)
std::atomic<size_t> g_fe_batch_min{2 * FE_BATCH};
// HBLS_SLOT_MSM: batched verifications of at least this many items (partials + folded aggregates,
// one chunk of groups) check every group at once -- the signature side as one multi-scalar
// multiplication (msm.hip), one final exponentiation for the call -- and fall back to the
// per-batch check when that fails (0 = never).  32 768: at C2 (40 k partials + 10 k folded
// aggregates) the slot-wide check beats the per-batch one since the multi-Miller loops and the
// six-lane final exponentiation (14.4 vs 15.3 ms per slot, profiles/r03s_ab_summary.txt)
std::atomic<size_t> g_slot_msm_min{32768};
// HBLS_ADAPTIVE=0: always try the slot-wide check.  Default: after a call whose slot-wide check
// failed (invalid partials or aggregates that only a pairing catches), the next calls go straight
// to the per-batch check -- a failing slot-wide check is work thrown away -- until a call passes
// every batch; under a sustained attack (C5: 1 % of the partials invalid in every slot) that
// saves the signature-side MSM, its lines and Miller loop, the product tree and one final
// exponentiation per slot.  Verdicts are the same either way.
std::atomic<bool> g_adaptive{true};
// HBLS_SUBGROUP_BATCH / hbls_subgroup_batch: device-buffer verifications of at least this many
// items that decompress all their signatures check them for G2 membership with one batched test
// (msm.hip k_subg_*: five bucket entries per signature and 20 tested sums instead of a 63-doubling
// ladder each) and run the per-item ladders only if it fails (0 = never).  2^19: above every call
// with a pinned launch trace (the largest runs chunks of 265 000 items), and far above the
// break-even.  With HBLS_ADAPTIVE, after a call whose batched test failed the
// next calls go straight to the ladders until one of them finds every signature in G2.
std::atomic<size_t> g_subg_batch_min{size_t(1) << 19};
// HBLS_SINGLE_MAX / hbls_single_max: host Verify batches of fewer items check every item alone
// (hgroup.h SINGLE_MAX_DEFAULT: the batched final exponentiation's threshold, g_fe_batch_min)
std::atomic<size_t> g_single_max{SINGLE_MAX_DEFAULT};

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
};

// hipMalloc'ed buffers that go when this does.  Like every hipMalloc and hipFree of the handle layer it
// lives under the device lock, with the device current: declare it behind the lock guard.
struct DevBufs {
  std::vector<void*> p;
  DevBufs(std::initializer_list<void*> own = {}) : p(own) {}  // own: takes over what was allocated elsewhere
  DevBufs(const DevBufs&) = delete;
  ~DevBufs() {
    for (void* q : p)
      if (q) (void)hipFree(q);
  }
  template <class T>
  int alloc(T** out, size_t bytes) {
    HCHK(hipMalloc((void**)out, bytes));
    p.push_back(*out);
    return 0;
  }
};

// workspace buffers of one set
enum WsId {
  W_VPK, W_VPKST, W_VSIG, W_VSIGST, W_IGRP, W_PR, W_SR, W_GP, W_GST, W_GMSG, W_GVER, W_GLINES, W_LIST, W_COUNT,
  W_FBLINES,
  W_APK, W_APKST, W_ASIG, W_APR, W_ASR,          // folded aggregates (post-aggregate verification)
  W_TAPTS, W_TADST, W_TAMST, W_TADIG, W_TATAB, W_TAJ, W_TAHIT,  // ThresholdAggregate / Aggregate
  W_TACSM, W_TASDIG, W_TASOK, W_TASDONE, W_TASTAB, W_TANONUNI,  // its small-scalar path
  W_SEGA, W_SEGB, W_SEGSTA, W_SEGSTB, W_VAPT, W_VAPV, W_PLAN,  // VerifyAggregate key reduction
  W_PCNT, W_PCOFF, W_PCFIRST, W_PCCOUNT, W_COEF, W_COEF4, W_RT1, W_RT2,  // chunk plan + multi-scalar RLC
  W_FBUF, W_GS, W_BS, W_BLINES, W_BBAD, W_BVER, W_GLIST, W_GCOUNT,  // batched final exponentiation
  W_MCNT, W_MOFF, W_MCUR, W_MORDER, W_MENT, W_MBUCKET, W_MPART, W_MPART2, W_MTOT, W_PBUF1, W_PBUF2, W_PBUF3, W_SFAIL,  // slot-wide check
  W_MLEV,                                                                          // its evaluated Miller lines
  W_SGDIG, W_SGCNT, W_SGOFF, W_SGCUR, W_SGORDER, W_SGENT, W_SGBUCKET, W_SGCLS, W_SGSUMS, W_SGREC,  // batched subgroup test
  W_PFIN, W_TBUF, W_F1, W_F1BAD, W_F1S, W_FIRST,                                                                  // final exponentiations' factors
  W_KLMISS, W_KLCNT,  // learned key cache: the call's missing keys (partials' keys, then DV keys) and their two counts
  W_KLENT, W_KLMENT,  // its ladder tables: every key's entry number (lookup), every miss's (learn -> k_pk_wide)
  // verified-member selection (hbls_slot_select_device): per group in the caller's order, the counting
  // sort, the tables and the aggregation's outputs in class order, the aggregates to verify
  W_SELCIDX, W_SELKEY, W_SELSTATE, W_SELGMSG, W_SELHIST, W_SELOFF, W_SELPERM, W_SELPMEM, W_SELPIDX, W_SELPGOFF,
  W_SELPOUT, W_SELPST, W_SELPPT, W_SELAPT, W_SELAST,
  W_SEGFIRST,  // segmented first-error mode (VerifyCall::gseg): two words per segment
  W_COUNT_
};

// A workspace set: grow-only device buffers plus the event recorded after the last kernel that
// used them.  Every user waits on `free_ev` in each stream it launches on before touching the
// set, so two calls never share a set concurrently, whatever streams they run on.
//
// Each set also owns the side streams its calls fork onto (decompression, hashing, aggregation)
// and their fork/join events, so two calls in flight on different user streams -- consecutive
// slots, say -- overlap instead of queueing behind each other on shared side streams.
constexpr int N_SIDE = 4;
struct Ws {
  DevBuf b[W_COUNT_];
  hipEvent_t free_ev = nullptr;
  bool used = false;
  hipStream_t side[N_SIDE] = {};
  hipEvent_t ev_fork = nullptr, ev_side[N_SIDE] = {}, ev_ta = nullptr, ev_msm = nullptr;
  hipEvent_t ev_pk = nullptr;  // the partials' keys decompressed (side 0, before the DV keys)
  hipEvent_t ev_dec = nullptr;  // the partials' signatures decompressed (side 1, before their subgroup checks)
  hipEvent_t ev_h = nullptr;  // host calls: the hashing done (before the messages' lines)
  hipEvent_t ev_dflt = nullptr;  // hbls_slot_device: the device's default stream when the call was made
};

// host-call staging buffers (inputs and outputs of the host-buffer entry points)
enum IoId {
  I_PK, I_SIG, I_MSG, I_OFF, I_LEN, I_MIDX, I_HM, I_STAT, I_IDX, I_GOFF, I_OUT, I_SK, I_VGOFF, I_HM2,
  // hbls_slot_select_batch: the candidates, their share indices and offsets, the DV keys; the members, their counts,
  // the aggregates and the two statuses per group
  I_CAND, I_CIDX, I_SGOFF, I_DVPK, I_CHOSEN, I_TACNT, I_TAOUT, I_TAST, I_AGGST,
  // hbls_duty_add: the items' serials, the touched groups (CSR), the per-item and per-touched-group outputs of
  // k_duty_store, its two lists and counters, the sorted fired rows and their group ids
  I_DSERIAL, I_DTGRP, I_DTOFF, I_DTPOS, I_DTIDX, I_DSTORED, I_DSLOT, I_DMSLOT, I_DMSER, I_DMIDX, I_DFMSG, I_DFKEY,
  I_DCOPY, I_DFIRED, I_DCTR, I_DFROW, I_DFGRP,
  // hbls_duty_add_sets: the items' set ids and arrival indices, the sets' first failures, the status bytes
  // k_duty_store reads, and (several shards) the decompressed signatures kept from phase one for phase two
  I_DSETID, I_DARR, I_DSETFIRST, I_DADMIT, I_DVSIG,
  I_DGSEG,  // hbls_duty_add_sets_first: the verification groups' set ids
  I_DCGRP, I_DCSHARE,  // a cluster duty's add: the items' groups and share indices (k_cluster_keys)
  I_COUNT
};

constexpr int N_WS_MAX = 8;  // workspace sets per device: HBLS_WS_SETS (default 3)
int g_ws_sets = 3;

struct Timed {
  const char* name;
  hipEvent_t a, b;
};

// Host-call contexts: a blocking host-buffer call (Verify / ThresholdAggregate / VerifyAggregate
// batches: what the Go shim calls from its goroutines) owns one from its first upload to its last
// download -- its own stream and staging buffers -- and holds the device lock only while it
// enqueues.  Several calls from different threads therefore overlap on the device (one workspace
// set each), as consecutive slots do on the device-buffer path.  g_ws_sets contexts per device; a
// caller beyond them waits for one to finish.
struct Hc {
  hipStream_t s = nullptr;
  DevBuf io[I_COUNT];
  bool busy = false;
  hipEvent_t ev = nullptr;  // a chunked call's hand-overs between contexts (verify_large)
  // pinned staging for uploads queued behind the call's own kernels: a pageable hipMemcpyAsync is
  // staged by the runtime and returns only once staged, so one queued behind the decompression
  // held the calling thread until that finished (verify_large's grouping: 20 ms measured; on a
  // stream of its own beside the kernels the pageable copies took over a second)
  uint8_t* pin = nullptr;
  size_t pin_cap = 0;
  // a signature-cache put (on the device's cache stream, after the call returned) still reading
  // this context's staging buffers: the context's next call waits for it before it uploads into
  // them (hc_acquire)
  hipEvent_t put_ev = nullptr;
  bool put_pending = false;
  hipStream_t put_s = nullptr;  // its signature-cache puts (sc_put_release)
};

// host arrays packed into a context's pinned staging, then one asynchronous copy each
struct PinnedUploads {
  struct Item {
    IoId id;
    const void* src;
    size_t bytes;
    void** dst;
  };
  std::vector<Item> items;
  template <class T>
  void add(IoId id, const T* src, size_t count, T** dst) {
    items.push_back({id, src, count * sizeof(T), (void**)dst});
  }
};

// one record per call that could take the slot-wide check: did it fail (or, skipped, did any batch
// fail the per-batch check)
struct SlotRes {
  uint8_t sfail, skipped, pad[2];
  uint32_t gcount;
};
constexpr unsigned N_RES = 16;
struct SubgRes {
  uint32_t rec[2];
  uint32_t skipped, pad;
};

struct Dev {
  int ord = -1;
  int n_cu = 256;  // compute units (4 SIMDs each)
  hipStream_t stream = nullptr;  // the library stream of host-buffer calls
  Ws ws[N_WS_MAX];
  unsigned next_ws = 0;
  DevBuf io[I_COUNT];
  std::mutex mu;  // one call at a time enqueues on this device
  Hc hc[N_WS_MAX];
  std::mutex hc_mu;  // hc[].busy
  std::condition_variable hc_cv;
  // public-key cache (hbls_pubkey_cache_add): decompressed entries + statuses, every device holds
  // all g_kc_n of them
  DevBuf kc_tab, kc_st;
  // its compressed keys and their open-addressing index (vbatch.hip k_kc_index / k_pk_cached):
  // kc_n entries indexed, kc_tcap slots (a power of two >= 2 kc_n)
  DevBuf kc_keys, kc_hidx;
  size_t kc_n = 0, kc_tcap = 0;
  // learned key cache (vbatch.hip k_pk_lookup / k_pk_learn; kl_table, kl_keys below): what the device
  // entry points have decompressed, found again by the keys' bytes.  kl_cap entries allocated and
  // emptied (0: not yet, or dropped by a reset); kl_ctr stays for the device's lifetime.
  DevBuf kl_keys, kl_ent, kl_st, kl_idx, kl_ctr;
  size_t kl_cap = 0, kl_tcap = 0;
  // the ladder tables of its first kl_wcap entries (ec28.h G1WidePt, 15 per entry; HBLS_KEY_WIDE),
  // written by k_pk_wide behind k_pk_learn and read by the combinations of later calls -- which
  // run behind their own lookup, so the ordering chain below covers them
  DevBuf kl_wide;
  size_t kl_wcap = 0;
  // ORDERING INVARIANT of the learned key cache.  Every kernel that touches the table runs on the
  // side stream 0 of some workspace set, enqueued under `mu`, in the order
  //     wait(kl_ev); k_pk_lookup ...; k_pk_learn ...; record(kl_ev)
  // so the table's reads and writes are totally ordered across calls, whatever streams and
  // workspace sets the calls use: lookup 1, learn 1, lookup 2, learn 2, ...  Visibility comes from
  // kernel boundaries alone; no kernel ever runs beside a writer of what it reads, and no
  // cross-kernel memory-ordering argument is needed.  (Slots enqueued back to back from cold
  // therefore decompress each key once.)  Anything that rewrites the table from the host side
  // (kl_reset) first drains the library's streams under `mu`.  Keep every new reader or writer
  // inside this chain.
  hipEvent_t kl_ev = nullptr;  // after the last call's k_pk_learn
  bool kl_ev_set = false;
  // decompressed-signature cache (vbatch.hip k_sc_write / k_sc_index / k_sc_get): filled by host-buffer Verify
  // batches, read by host-buffer ThresholdAggregate batches; enqueued under `mu` like everything
  // else.  A put runs on its host-call context's own put stream, off the Verify call's critical
  // path and beside other contexts' puts: it waits for its call's pipeline (`pipe`), for every get
  // enqueued before it (a put rewrites ring entries a get may read) and for any put still in flight
  // whose ring range overlaps its own, and records `done`.  A get waits only for puts whose
  // pipeline has already completed (a short kernel pair); the ring entries of puts still behind
  // their pipeline are passed to it as a range of misses.  Ring positions are also counted without
  // the wrap (`pos`), so the span of the in-flight puts is exact.
  DevBuf sc_key, sc_ent, sc_st, sc_tab;
  size_t sc_cap = 0, sc_cursor = 0, sc_filled = 0;
  uint64_t sc_pos = 0;
  struct ScPut {
    size_t start, m;
    uint64_t pos;
    hipEvent_t pipe, done;
  };
  std::deque<ScPut> sc_inflight;       // enqueue (= ring) order
  std::vector<hipEvent_t> sc_gets;     // gets not yet known complete
  std::vector<hipEvent_t> sc_ev_pool;  // spare events
  // adaptive slot-wide check (HBLS_ADAPTIVE): outcomes of recent checked calls, copied to pinned host
  // memory asynchronously and read once their event has completed -- never a synchronisation
  SlotRes* res_host = nullptr;
  hipEvent_t res_ev[N_RES] = {};
  unsigned res_head = 0, res_tail = 0;  // records [tail, head) not yet read
  bool attack = false;                  // the last known call had invalid items a pairing caught
  // batched subgroup test: its cumulative counters on the device (hbls_subgroup_batch_stats) and
  // its own adaptive history, kept like the slot-wide check's -- the record of each call that ran
  // or skipped the test ([0] the test failed, [1] points its ladders found off G2)
  DevBuf sg_ctr;
  SubgRes* sres_host = nullptr;
  hipEvent_t sres_ev[N_RES] = {};
  unsigned sres_head = 0, sres_tail = 0;
  bool subg_failed = false;  // the last known call had signatures off G2
  // verified-member selection: its cumulative counters (layout.h SEL_*; hbls_slot_select_stats)
  DevBuf sel_ctr;
  // timing (hbls_timing)
  bool timing = false;
  bool serial = false;  // timing mode 2: every timed launch completes before the next is enqueued
  std::vector<Timed> tev;
  size_t tev_used = 0;
};

// HBLS_SIG_CACHE / hbls_sig_cache: entries of each device's decompressed-signature cache (a power
// of two; 0 = off).  2^21 (two C3 slots of partials): 2 M x 305 B = 640 MB per device.
std::atomic<size_t> g_sc_cap{size_t(1) << 21};
uint64_t g_sc_k0 = 0x243f6a8885a308d3ull, g_sc_k1 = 0x13198a2e03707344ull;  // keyed hash (getrandom at init)
// HBLS_KEY_LEARN / hbls_tune: entries of each device's learned key cache (0 = off).  2^21: the
// smallest power of two above the largest per-GPU key set of BASELINE.json (C3: 1.0 M pubshares +
// 0.1 M DV keys); 2 M x 149 B = 312 MB plus a 16 MB index per device, allocated by the first call
// that uses it.
std::atomic<size_t> g_key_learn{size_t(1) << 21};
constexpr size_t KEY_LEARN_MAX = size_t(1) << 30;
// HBLS_KEY_WIDE / hbls_tune: how many of those entries also get a ladder table (15 affine points,
// 1440 B; at most the cache's capacity, the default; 0 = none): 2 M x 1440 B = 3.0 GB per device,
// allocated with the cache.  A new value empties the cache.
std::atomic<size_t> g_key_wide{KEY_LEARN_MAX};

std::mutex g_init_mu;
std::vector<Dev*> g_devs;  // in device-mask order (hbls_debug_split: each ordinal repeated); g_devs_mu
std::mutex g_devs_mu;      // hbls_debug_split swaps g_devs while calls may be in flight
// a snapshot of g_devs: Dev objects are never freed (split contexts are pooled), so the pointers
// stay valid after the lock is released
std::vector<Dev*> devs() {
  std::lock_guard<std::mutex> l(g_devs_mu);
  return g_devs;
}
std::vector<Dev*> g_base_devs;   // one per device of the mask
std::vector<std::vector<Dev*>> g_split_pool;  // per base device: extra contexts of hbls_debug_split (reused)
uint32_t g_mask = 0;
std::atomic<bool> g_ready{false};

int ensure_buf(DevBuf& b, size_t bytes, void** out) {
  if (bytes == 0) bytes = 16;
  if (b.cap < bytes) {
    if (b.p) HCHK(hipFree(b.p));
    b.p = nullptr;
    size_t cap = bytes + bytes / 4;
    HCHK(hipMalloc(&b.p, cap));
    b.cap = cap;
  }
  *out = b.p;
  return 0;
}

template <class T>
int wsbuf(Ws& w, WsId id, size_t count, T** out) {
  // growing a buffer frees the old one: its last user (on any stream) must be done with it
  if (w.used && w.b[id].cap < std::max<size_t>(count * sizeof(T), 16)) HCHK(hipEventSynchronize(w.free_ev));
  void* p;
  if (ensure_buf(w.b[id], count * sizeof(T), &p)) return -1;
  *out = (T*)p;
  return 0;
}

// Acquire a workspace set for a call whose kernels run on `s` and the set's side streams.
Ws& ws_acquire(Dev& d, hipStream_t s) {
  Ws& w = d.ws[d.next_ws++ % (unsigned)g_ws_sets];
  if (w.used) {
    (void)hipStreamWaitEvent(s, w.free_ev, 0);
    for (hipStream_t x : w.side) (void)hipStreamWaitEvent(x, w.free_ev, 0);
  }
  return w;
}
int ws_release(Ws& w, hipStream_t last) {
  HCHK(hipEventRecord(w.free_ev, last));
  w.used = true;
  return 0;
}

// --- timing of kernel launches (hbls_timing): event pairs on the launch's stream -------------
int timed_begin(Dev& d, const char* name, hipStream_t s, Timed** t) {
  *t = nullptr;
  if (!d.timing) return 0;
  if (d.tev_used == d.tev.size()) {
    Timed x{name, nullptr, nullptr};
    HCHK(hipEventCreate(&x.a));
    HCHK(hipEventCreate(&x.b));
    d.tev.push_back(x);
  }
  Timed& x = d.tev[d.tev_used++];
  x.name = name;
  HCHK(hipEventRecord(x.a, s));
  *t = &x;
  return 0;
}
int timed_end(Dev& d, Timed* t, hipStream_t s) {
  if (t) {
    HCHK(hipEventRecord(t->b, s));
    if (d.serial) HCHK(hipEventSynchronize(t->b));  // the kernel ran alone on the device
  }
  return 0;
}
#define TIMED(dev, name, s, call)                  \
  do {                                             \
    Timed* _t;                                     \
    if (timed_begin((dev), (name), (s), &_t)) return -1; \
    call;                                          \
    HCHK(hipGetLastError());                       \
    if (timed_end((dev), _t, (s))) return -1;      \
  } while (0)

int dev_create(int ord, Dev** out) {
  HCHK(hipSetDevice(ord));
  hipDeviceProp_t prop;
  HCHK(hipGetDeviceProperties(&prop, ord));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return set_err(std::string("libhipbls is built for gfx950, device ") + std::to_string(ord) + " is " +
                   prop.gcnArchName);
  Dev* d = new Dev();
  d->ord = ord;
  d->n_cu = std::max(1, prop.multiProcessorCount);
  // the verification's side streams (decompression, hashing) get the highest priority: they
  // gate the pairing kernel; the library stream is the lowest
  int prio_lo = 0, prio_hi = 0;
  HCHK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
  HCHK(hipStreamCreateWithPriority(&d->stream, hipStreamNonBlocking, prio_lo));
  for (int k_ws = 0; k_ws < g_ws_sets; k_ws++) {
    Ws& w = d->ws[k_ws];
    HCHK(hipEventCreateWithFlags(&w.free_ev, hipEventDisableTiming));
    for (int k = 0; k < N_SIDE; k++) {
      // side 3 (the slot's ThresholdAggregate) at high priority like the others (the lowest measured
      // 135.7-135.9 against 134.2-134.9 ms per C3 slot, three slots in flight)
      HCHK(hipStreamCreateWithPriority(&w.side[k], hipStreamNonBlocking, prio_hi));
      HCHK(hipEventCreateWithFlags(&w.ev_side[k], hipEventDisableTiming));
    }
    HCHK(hipEventCreateWithFlags(&w.ev_fork, hipEventDisableTiming));
    HCHK(hipEventCreateWithFlags(&w.ev_ta, hipEventDisableTiming));
    HCHK(hipEventCreateWithFlags(&w.ev_msm, hipEventDisableTiming));
    HCHK(hipEventCreateWithFlags(&w.ev_h, hipEventDisableTiming));
    HCHK(hipEventCreateWithFlags(&w.ev_pk, hipEventDisableTiming));
    HCHK(hipEventCreateWithFlags(&w.ev_dec, hipEventDisableTiming));
    HCHK(hipEventCreateWithFlags(&w.ev_dflt, hipEventDisableTiming));
    HCHK(hipStreamCreateWithPriority(&d->hc[k_ws].s, hipStreamNonBlocking, prio_lo));
    HCHK(hipEventCreateWithFlags(&d->hc[k_ws].ev, hipEventDisableTiming));
  }
  HCHK(hipEventCreateWithFlags(&d->kl_ev, hipEventDisableTiming));
  HCHK(hipHostMalloc((void**)&d->res_host, N_RES * sizeof(SlotRes), hipHostMallocDefault));
  for (unsigned k = 0; k < N_RES; k++) HCHK(hipEventCreateWithFlags(&d->res_ev[k], hipEventDisableTiming));
  HCHK(hipHostMalloc((void**)&d->sres_host, N_RES * sizeof(SubgRes), hipHostMallocDefault));
  for (unsigned k = 0; k < N_RES; k++) HCHK(hipEventCreateWithFlags(&d->sres_ev[k], hipEventDisableTiming));
  {
    void* p;
    if (ensure_buf(d->sg_ctr, sizeof(SubgCtr), &p)) return -1;
    HCHK(hipMemset(p, 0, sizeof(SubgCtr)));
    HCHK(hipStreamSynchronize(nullptr));
  }
  *out = d;
  return 0;
}

// hbls_init: mask 0 = HBLS_DEVICE_MASK from the environment, else device 0; 0xffffffff = every
// visible device.  Idempotent for the same mask; a different mask afterwards is an error.
int init_mask(uint32_t mask) {
  if (g_ready.load()) {
    if (mask != 0 && mask != g_mask && !(mask == 0xffffffffu && g_mask == ((1u << g_base_devs.size()) - 1)))
      return set_err("hipbls already initialised with device mask " + std::to_string(g_mask));
    return 0;
  }
  std::lock_guard<std::mutex> lk(g_init_mu);
  if (g_ready.load()) return init_mask(mask);
  int n = 0;
  HCHK(hipGetDeviceCount(&n));
  if (n <= 0) return set_err("no HIP device");
  if (mask == 0) mask = (uint32_t)env_size("HBLS_DEVICE_MASK", 1);
  const uint32_t visible = n >= 32 ? 0xffffffffu : ((1u << n) - 1);
  if (mask == 0xffffffffu) mask = visible;
  if ((mask & visible) != mask || mask == 0)
    return set_err("device mask " + std::to_string(mask) + " names devices that are not visible (" +
                   std::to_string(n) + " devices)");
  g_gcap = std::max<size_t>(1, env_size("HBLS_GROUP_CHUNK", g_gcap.load()));
  g_fbcap = std::max<size_t>(1, env_size("HBLS_FALLBACK_CHUNK", g_fbcap.load()));
  g_gmax = std::max<size_t>(1, env_size("HBLS_GROUP_MAX", g_gmax.load()));
  g_rlc_lanes = std::max<size_t>(1, env_size("HBLS_RLC_LANES", g_rlc_lanes.load()));
  g_ta_joint = std::min<size_t>(8, env_size("HBLS_TA_JOINT", g_ta_joint.load()));
  g_fe_batch_min = env_size("HBLS_FE_BATCH", g_fe_batch_min.load());
  g_slot_msm_min = env_size("HBLS_SLOT_MSM", g_slot_msm_min.load());
  g_adaptive = env_size("HBLS_ADAPTIVE", 1) != 0;
  g_subg_batch_min = env_size("HBLS_SUBGROUP_BATCH", g_subg_batch_min.load());
  g_single_max = env_size("HBLS_SINGLE_MAX", SINGLE_MAX_DEFAULT);
  g_dec_pair_max = env_size("HBLS_DEC_PAIR_MAX", 0);
  g_ta_pair_max = env_size("HBLS_TA_PAIR_MAX", g_ta_pair_max.load());
  g_hash_pair_max = env_size("HBLS_HASH_PAIR_MAX", g_hash_pair_max.load());
  g_hash_one_lane = env_size("HBLS_HASH_ONE_LANE", g_hash_one_lane.load());
  g_hash_split = env_size("HBLS_HASH_SPLIT", 1) != 0;
  g_fe18_max = env_size("HBLS_FE18_MAX", g_fe18_max.load());
  g_key_learn = std::min(env_size("HBLS_KEY_LEARN", g_key_learn.load()), KEY_LEARN_MAX);
  g_key_wide = std::min(env_size("HBLS_KEY_WIDE", g_key_wide.load()), KEY_LEARN_MAX);
  g_ws_sets = (int)std::min<size_t>(N_WS_MAX, std::max<size_t>(1, env_size("HBLS_WS_SETS", 3)));
  {
    size_t sc = env_size("HBLS_SIG_CACHE", g_sc_cap.load());
    while (sc & (sc - 1)) sc &= sc - 1;  // a power of two
    g_sc_cap = std::min<size_t>(sc, size_t(1) << 30);
    uint64_t k[2];
    if (getrandom(k, sizeof(k), 0) == (ssize_t)sizeof(k)) {  // otherwise the fixed key (a miss costs time only)
      g_sc_k0 = k[0];
      g_sc_k1 = k[1] | 1;
    }
  }
  std::vector<Dev*> devs;
  for (int k = 0; k < 32; k++)
    if (mask & (1u << k)) {
      Dev* d;
      if (dev_create(k, &d)) return -1;
      devs.push_back(d);
    }
  {
    std::lock_guard<std::mutex> l(g_devs_mu);
    g_devs = devs;
  }
  g_base_devs = devs;
  g_mask = mask;
  g_ready.store(true);
  return 0;
}

int ensure_init() { return g_ready.load() ? 0 : init_mask(0); }

// the device of a caller's stream (device entry points); stream 0: the first device
int dev_of_stream(hipStream_t s, Dev** out) {
  if (ensure_init()) return -1;
  const std::vector<Dev*> ds = devs();
  int ord = ds[0]->ord;
  if (s) {
    hipDevice_t dv;
    HCHK(hipStreamGetDevice(s, &dv));
    ord = (int)dv;
  }
  for (Dev* d : ds)
    if (d->ord == ord) {
      HCHK(hipSetDevice(ord));
      *out = d;
      return 0;
    }
  return set_err("stream belongs to device " + std::to_string(ord) + ", outside the library's device mask");
}

// a host call's stream and staging buffers: its context's, or the device's own (h == nullptr: the
// small entry points, which hold the device lock throughout)
inline hipStream_t call_stream(Dev& d, Hc* h) { return h ? h->s : d.stream; }
inline DevBuf* call_io(Dev& d, Hc* h) { return h ? h->io : d.io; }

template <class T>
int upload(Dev& d, IoId id, const T* src, size_t count, T** dst, Hc* h = nullptr) {
  void* p;
  if (ensure_buf(call_io(d, h)[id], count * sizeof(T), &p)) return -1;
  if (count) HCHK(hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, call_stream(d, h)));
  *dst = (T*)p;
  return 0;
}

// the uploads through h's pinned staging, on h's stream (never blocks the calling thread; the
// staging is reused by the context's next call only, after this one's stream synchronisation)
int upload_pinned(Dev& d, Hc& h, const PinnedUploads& u) {
  auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
  size_t total = 0;
  for (const auto& it : u.items) total += al(it.bytes);
  if (total > h.pin_cap) {
    if (h.pin) HCHK(hipHostFree(h.pin));
    h.pin = nullptr;
    h.pin_cap = 0;
    const size_t cap = std::max(total + total / 4, size_t(1) << 20);
    HCHK(hipHostMalloc((void**)&h.pin, cap, hipHostMallocDefault));
    h.pin_cap = cap;
  }
  size_t o = 0;
  for (const auto& it : u.items) {
    void* p;
    if (ensure_buf(h.io[it.id], it.bytes, &p)) return -1;
    if (it.bytes) {
      memcpy(h.pin + o, it.src, it.bytes);
      HCHK(hipMemcpyAsync(p, h.pin + o, it.bytes, hipMemcpyHostToDevice, h.s));
    }
    *it.dst = p;
    o += al(it.bytes);
  }
  return 0;
}

// a context's staging buffers are free once the signature-cache put of its previous call has read
// them (a short kernel pair that started when that call's pipeline ended)
void hc_ready(Hc& h) {
  if (h.put_pending) {
    (void)hipEventSynchronize(h.put_ev);
    h.put_pending = false;
  }
}
Hc& hc_acquire(Dev& d) {
  Hc* got = nullptr;
  {
    std::unique_lock<std::mutex> lk(d.hc_mu);
    while (!got) {
      for (int k = 0; k < g_ws_sets && !got; k++)
        if (!d.hc[k].busy) {
          d.hc[k].busy = true;
          got = &d.hc[k];
        }
      if (!got) d.hc_cv.wait(lk);
    }
  }
  hc_ready(*got);
  return *got;
}
void hc_release(Dev& d, Hc& h) {
  {
    std::lock_guard<std::mutex> lk(d.hc_mu);
    h.busy = false;
  }
  d.hc_cv.notify_one();
}
// a free context or nullptr (never waits: a chunked call takes only what is idle)
Hc* hc_try_acquire(Dev& d) {
  Hc* got = nullptr;
  {
    std::lock_guard<std::mutex> lk(d.hc_mu);
    for (int k = 0; k < g_ws_sets && !got; k++)
      if (!d.hc[k].busy) {
        d.hc[k].busy = true;
        got = &d.hc[k];
      }
  }
  if (got) hc_ready(*got);
  return got;
}

// per-call random linear combination key (OS CSPRNG)
int rlc_key(RlcKey& k) {
  uint8_t* p = reinterpret_cast<uint8_t*>(k.w);
  size_t got = 0;
  while (got < sizeof(k.w)) {
    ssize_t r = getrandom(p + got, sizeof(k.w) - got, 0);
    if (r <= 0) return set_err("getrandom failed");
    got += (size_t)r;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------
// Batched verification of n partials already in device memory (vbatch.hip):
//   side 0: k_dec_pk            side 1: k_dec_sig_pt
//   s:      k_item_group, k_rlc, then per chunk of groups k_group_prep -> k_pair3,
//           k_scatter, then the fallback passes (k_fb_lines -> k_pair3 over the listed items)
// Optional fold of the slot's ThresholdAggregate (reusing the decompressed partials) and of the
// post-aggregate verification under the DV keys (sigagg.go:117) into the same groups.
// ---------------------------------------------------------------------------------------
// verification statistics (HBLS_STATS=1): items, groups, items re-checked alone
std::atomic<uint64_t> g_stats[8];
bool stats_on() {
  const char* v = getenv("HBLS_STATS");
  return v && v[0] == '1';
}

struct TaFold {
  // aggregation members: verified partial src[j] (src == nullptr: decompress sigs instead)
  const uint8_t* ta_sigs;
  const uint32_t* ta_src;
  const int64_t* ta_idx;
  const uint32_t* grp_off;
  size_t n_groups, n_partials;
  uint8_t* ta_out;
  uint8_t* ta_status;
  // post-aggregate verification (nullable): DV public key per group, verdict per group
  const uint8_t* dv_pks;
  uint8_t* agg_status;
  // decompressed-key tables (hbls_decompress_pubkeys_device; nullable): used instead of
  // decompressing pks / dv_pks in this call
  const G1AEntry* pk_table;
  const uint8_t* pk_table_st;
  const G1AEntry* dv_pk_table;
  const uint8_t* dv_pk_table_st;
};


// ThresholdAggregate (mode 0) / Aggregate (mode 1) of groups whose members are already
// decompressed (pts, mst) into ta_out / ta_status; agg_pt (nullable) gets the affine results.
int ta_tail(Dev& d, Ws& w, const HmEntry* pts, const uint32_t* src, const uint8_t* mst_in, const int64_t* didx,
            const uint32_t* dgoff, size_t n_groups, size_t np, int mode, uint8_t* out, uint8_t* status,
            HmEntry* agg_pt, hipStream_t s, hipEvent_t mst_ready = nullptr, hipEvent_t pts_ready = nullptr,
            const uint8_t** sdone_out = nullptr) {
  if (sdone_out) *sdone_out = nullptr;  // the groups the small-scalar path took, when it ran
  uint8_t* mst;
  TaDigits* dig;
  void* tab;
  G2JEntry* pj;
  if (wsbuf(w, W_TAMST, np, &mst) || wsbuf(w, W_TADIG, np, &dig) || wsbuf(w, W_TAJ, np, &pj)) return -1;
  // joint ladders over chunks of a validator's members (k_ta_jtab, k_ta_jladder, k_ta_jgeneral) when every group has t members
  const size_t t_u = (n_groups && np % n_groups == 0) ? np / n_groups : 0;
  size_t jc = 0;
  if (mode == 0 && t_u > 1) {
    const size_t knob = g_ta_joint.load();
    jc = knob ? knob : np / TA_JOINT_LANES;
    jc = std::min<size_t>(std::min<size_t>(jc, t_u), 8);
    if (jc <= 1) jc = 0;
  }
  // (the joint path's guarded per-member fallback reads the same buffer: the larger of the two)
  const size_t tab_bytes = jc ? std::max(ta_joint_table_bytes((uint32_t)n_groups, (uint32_t)t_u, (uint32_t)jc),
                                         ta_table_bytes((uint32_t)np))
                              : ta_table_bytes((uint32_t)np);
  if (wsbuf(w, W_TATAB, tab_bytes, (uint8_t**)&tab)) return -1;
  if (np) {
    // t_u > 1: the joint and small-scalar paths assume groups of exactly t_u members; k_ta_layout
    // flags any other layout in nonuni (the per-member ladders then run instead)
    uint8_t* nonuni = nullptr;
    if (mode == 0 && t_u > 1) {
      if (wsbuf(w, W_TANONUNI, 1, &nonuni)) return -1;
      HCHK(hipMemsetAsync(nonuni, 0, 1, s));
      TIMED(d, "k_ta_lambda", s, launch_ta_layout(dgoff, (uint32_t)n_groups, (uint32_t)t_u, nonuni, s));
    }
    // small-scalar path first (groups of exactly t members, wave-uniform index sets); the Lagrange
    // digits and the per-member ladders below skip the groups it aggregated
    uint8_t* sdone = nullptr;
    if (mode == 0 && t_u >= 2 && t_u <= (size_t)TA_SMALL_MAX) {
      int64_t* csm;
      TaDigits* sdig;
      uint8_t *sok, *stab;
      if (wsbuf(w, W_TACSM, np, &csm) || wsbuf(w, W_TASDIG, n_groups, &sdig) || wsbuf(w, W_TASOK, n_groups, &sok) ||
          wsbuf(w, W_TASDONE, n_groups, &sdone) || wsbuf(w, W_TASTAB, ta_small_table_bytes((uint32_t)n_groups), &stab))
        return -1;
      TIMED(d, "k_ta_small", s,
            launch_ta_small(pts, src, didx, (uint32_t)n_groups, (uint32_t)t_u, csm, sdig, sok, stab, sdone, pj, s,
                            nonuni, pts_ready));
      pts_ready = nullptr;  // waited for inside, after the index-only split
      if (sdone_out) *sdone_out = sdone;
    }
    if (pts_ready) HCHK(hipStreamWaitEvent(s, pts_ready, 0));
    // the members' statuses are first read by the Lagrange digits: the small-scalar ladders above
    // run on the decompressed points while their subgroup checks (mst_ready) finish; a member that
    // fails them makes its group's status and output below whatever the ladders computed
    if (mst_ready) HCHK(hipStreamWaitEvent(s, mst_ready, 0));
    if (src) launch_ta_member_status(mst_in, src, (uint32_t)np, mst, s);
    else HCHK(hipMemcpyAsync(mst, mst_in, np, hipMemcpyDeviceToDevice, s));
    HCHK(hipGetLastError());
    TIMED(d, "k_ta_lambda", s,
          launch_ta_lambda(didx, dgoff, (uint32_t)n_groups, (uint32_t)np, mode, dig, mst, s, (uint32_t)t_u, nonuni,
                           sdone));
    if (jc) {
      TIMED(d, "k_ta_straus", s,
            launch_ta_joint(pts, src, dig, (uint32_t)n_groups, (uint32_t)t_u, (uint32_t)jc, tab, pj, s, sdone, nonuni));
      // groups not all of t_u members: the per-member ladders instead (nothing unless nonuni)
      TIMED(d, "k_ta_straus", s,
            launch_ta_straus(pts, src, dig, (uint32_t)np, (uint32_t)n_groups, tab, pj, s, nullptr, nonuni));
    } else {
      TIMED(d, "k_ta_straus", s, launch_ta_straus(pts, src, dig, (uint32_t)np, (uint32_t)n_groups, tab, pj, s, sdone));
    }
  }
  TIMED(d, "k_group_sum", s,
        LAUNCH(k_group_sum, n_groups, s, dgoff, (uint32_t)n_groups, mode, (const G2JEntry*)pj, (const uint8_t*)mst,
               out, status, agg_pt));
  return 0;
}

// Every launch the library enqueued on its own streams (the library stream, the host-call
// contexts' and the workspaces' side streams) has completed -- not the whole device: caller, torch
// and RCCL streams keep running.  Caller holds d.mu, so nothing new is enqueued meanwhile.
int drain_lib_streams(Dev& d) {
  HCHK(hipStreamSynchronize(d.stream));
  for (int k = 0; k < N_WS_MAX; k++) {
    if (d.hc[k].s) HCHK(hipStreamSynchronize(d.hc[k].s));
    for (int j = 0; j < N_SIDE; j++)
      if (d.ws[k].side[j]) HCHK(hipStreamSynchronize(d.ws[k].side[j]));
  }
  return 0;
}

// ---- learned key cache (Dev::kl_*; kernels in vbatch.hip).  All under d.mu.
// Empty the table (hbls_pubkey_cache_clear, a new HBLS_KEY_LEARN): its readers and writers all
// run on workspace side streams, drained first; the next call that uses the cache allocates and
// zeroes it again.  The hit and miss counters keep counting.
int kl_reset(Dev& d, bool release) {
  if (!d.kl_cap && !release) return 0;
  HCHK(hipSetDevice(d.ord));
  if (drain_lib_streams(d)) return -1;
  d.kl_cap = d.kl_tcap = d.kl_wcap = 0;
  d.kl_ev_set = false;
  if (release)
    for (DevBuf* b : {&d.kl_keys, &d.kl_ent, &d.kl_st, &d.kl_idx, &d.kl_wide}) {
      if (b->p) HCHK(hipFree(b->p));
      *b = DevBuf{};
    }
  return 0;
}
// The table at the current capacity, allocated and emptied on stream ss (a side stream 0, inside
// the ordering chain of Dev::kl_ev) when there is none; t->cap == 0: the cache is off.
int kl_table(Dev& d, hipStream_t ss, KeyLearnTab* t) {
  *t = KeyLearnTab{};
  const size_t cap = g_key_learn.load();
  if (!cap) return 0;
  if (d.kl_cap != cap) {
    if (kl_reset(d, false)) return -1;
    size_t tcap = 2;  // a power of two >= 2 cap: load <= 1/2
    while (tcap < 2 * cap) tcap *= 2;
    void* p;
    const bool first = d.kl_ctr.p == nullptr;
    const size_t wcap = std::min(g_key_wide.load(), cap);
    const size_t wbytes = wcap * KEY_WIDE_PTS * sizeof(G1WidePt);  // (exact: ensure_buf's slack would be 0.75 GB)
    if (d.kl_wide.cap < wbytes) {
      if (d.kl_wide.p) HCHK(hipFree(d.kl_wide.p));
      d.kl_wide = DevBuf{};
      HCHK(hipMalloc(&d.kl_wide.p, wbytes));
      d.kl_wide.cap = wbytes;
    }
    if (ensure_buf(d.kl_keys, 48 * cap, &p) || ensure_buf(d.kl_ent, cap * sizeof(G1AEntry), &p) ||
        ensure_buf(d.kl_st, cap, &p) || ensure_buf(d.kl_idx, tcap * sizeof(uint32_t), &p) ||
        ensure_buf(d.kl_ctr, sizeof(KeyLearnCtr), &p))
      return -1;
    if (first) HCHK(hipMemsetAsync(d.kl_ctr.p, 0, sizeof(KeyLearnCtr), ss));
    HCHK(hipMemsetAsync(d.kl_idx.p, 0, tcap * sizeof(uint32_t), ss));
    HCHK(hipMemsetAsync(&((KeyLearnCtr*)d.kl_ctr.p)->size, 0, sizeof(uint32_t), ss));
    d.kl_cap = cap;
    d.kl_tcap = tcap;
    d.kl_wcap = wcap;
  }
  t->keys = (uint8_t*)d.kl_keys.p;
  t->ent = (G1AEntry*)d.kl_ent.p;
  t->st = (uint8_t*)d.kl_st.p;
  t->idx = (uint32_t*)d.kl_idx.p;
  t->ctr = (KeyLearnCtr*)d.kl_ctr.p;
  t->cap = (uint32_t)d.kl_cap;
  t->tcap = (uint32_t)d.kl_tcap;
  t->wide = (G1WidePt*)d.kl_wide.p;
  t->wcap = (uint32_t)d.kl_wcap;
  return 0;
}
// The keys of one array through the cache on ss: hits copied, the misses listed at miss[0 ..
// *mcount) and decompressed there (labelled k_pk_miss, not k_dec_pk: with every key cached these
// launches are empty, and a per-key rate computed from them would mean nothing)
int kl_keys(Dev& d, const KeyLearnTab& t, const uint8_t* pks, size_t n, G1AEntry* out, uint8_t* st, uint32_t* miss,
            uint32_t* mcount, uint32_t* went, hipStream_t ss) {
  TIMED(d, "k_pk_lookup", ss, launch_pk_lookup(t, pks, (uint32_t)n, g_sc_k0, g_sc_k1, out, st, miss, mcount, went, ss));
  TIMED(d, "k_pk_miss", ss, launch_pk_miss(pks, (uint32_t)n, miss, mcount, out, st, ss));
  return 0;
}

static_assert(VP_GROUPS_PER_WAVE == GROUPS_PER_WAVE && VP_PROD_FAN == PROD_FAN && VP_RLC_CHUNK == RLC_CHUNK,
              "vplan.h restates layout.h");

// One verification (verify_pipeline): the call's inputs by name, and what it hands back.
struct VerifyCall {
  const uint8_t *pks = nullptr, *sigs = nullptr;  // compressed, n of each
  const uint32_t* msg_idx = nullptr;              // each item's message in hm
  const MsgEntry* hm = nullptr;
  size_t n = 0;
  const uint32_t* grp_off = nullptr;  // the verification groups' offsets (null: every item its own group)
  size_t n_groups = 0;
  uint8_t* status = nullptr;  // out: one per item
  hipStream_t s = nullptr;
  hipEvent_t hm_ready = nullptr;  // the hashed messages and their lines (null: already ordered before s)
  hipEvent_t h_ready = nullptr;   // host calls: the hashing alone, before the messages' lines
  const TaFold* fold = nullptr;   // the slot's ThresholdAggregate and folded aggregates, key tables
  bool key_cache = false;         // host-buffer call: the keys through the public-key cache
  bool device_entry = false;      // a device-buffer entry point (the batched subgroup test, vplan.h own_sigs)
  // defer_hm / defer_msgs: the caller hashed the defer_msgs messages at defer_hm (the call's messages
  // or a contiguous range of them) without their Miller lines (callers whose messages have about one
  // verification group each, batched final exponentiation sizes): the slot-wide check evaluates each
  // group's chain at P directly (k_lines_at_p) and the unevaluated lines are computed only behind a
  // failed check; any other path computes them first.
  MsgEntry* defer_hm = nullptr;
  size_t defer_msgs = 0;
  // first-error mode (vplan.h): the first item whose status is decided and not OK (0xffffffff: none)
  uint32_t* first_out = nullptr;
  // segmented first-error mode (dutyfirst.h; hbls_duty_add_sets_first): the call's groups are cut into
  // n_seg ordered segments, gseg[g] the segment of group g, and each segment gets its own first failure
  // where the plan's first_only applies (exact statuses where it does not).  Per segment the pipeline
  // keeps two words (batch and group, VerifyBufs::wseg) and writes seg_first_out[k]: the smallest
  // item_arrival[i] over the items i of segment item_seg[i] == k whose status is decided and not OK
  // (0xffffffff: none).  Takes no folded aggregates, and not first_out beside it.
  const uint32_t* gseg = nullptr;
  uint32_t n_seg = 0;
  const uint32_t *item_seg = nullptr, *item_arrival = nullptr;
  uint32_t* seg_first_out = nullptr;
  // the items' signatures already decompressed and in G2, with their statuses (sigs is then unused):
  // hbls_slot_select_device's aggregates, sums of partials it decompressed and subgroup-checked
  const HmEntry* pre_sig = nullptr;
  const uint8_t* pre_sigst = nullptr;
  // keys by cluster (a cluster duty's adds and its fired groups' aggregates; pks is then unused): the
  // shard's resident keys and each item's group and share index (null: the groups' DV keys), resolved by
  // k_cluster_keys where the lookup runs otherwise.  The out fields are the pipeline's.  Such a call
  // neither reads nor writes the learned key cache and is outside the chain of Dev::kl_ev.
  const ClusterKeysArgs* cluster = nullptr;
  const G1WidePt* cluster_wide = nullptr;  // the cluster's ladder tables (null: none)
  // handed back: the decompressed signatures and their statuses (the host calls' signature-cache put)
  HmEntry* vsig = nullptr;
  uint8_t* vsigst = nullptr;
};

// The call's workspace buffers (verify_bufs; value-initialised, so null where the plan has no use
// for one), its coefficient key, and what a phase leaves for a later one.
struct VerifyBufs {
  // the decompressed keys and signatures with their statuses (vpk / vpkst and apk / apkst: the
  // caller's key tables when it gave them), the items' groups and sides, the groups' sums, states,
  // messages, verdicts and lines, the fallback's list
  G1AEntry* vpk;
  HmEntry* vsig;
  uint8_t *vpkst, *vsigst, *gst, *gver;
  uint32_t *igrp, *gmsg, *list, *count;
  G1JEntry* pr;
  G2JEntry* sr;
  G1AEntry* gP;
  LineEntry *glines, *fbl;
  // folded aggregates (n_agg)
  G1AEntry* apk;
  uint8_t* apkst;
  HmEntry* asig;
  G1JEntry* apr;
  G2JEntry* asr;
  uint32_t* wfirst;  // first_only
  uint32_t* wseg;    // first_only with VerifyCall::gseg: two words per segment (taken by verify_pipeline)
  // batched final exponentiation (bfe)
  Fp4Entry* fbuf;
  G2JEntry *gS, *bS;
  LineEntry* blines;
  uint8_t *bbad, *bver;
  uint32_t *glist, *gcount;
  // the two factors of each final exponentiation side by side (product tree root, signature-side
  // loop), and the product tree's intermediate level
  Fp4Entry *pfin, *tbuf;
  // slot-wide check (smsm).  pbuf1: the multi-Miller loops (kept: behind a failed slot-wide check
  // they are the per-batch check's public-key sides); pbuf2 / pbuf3: the product tree's levels
  G2MsmArgs ma;
  Fp4Entry *pbuf1, *pbuf2, *pbuf3;
  uint8_t* sfail;
  LineEntry* mlev;
  // the items' coefficients (folded aggregates' behind them at coef + n): written by the first
  // combination for the slot-wide check's MSM and its guarded second pass (smsm), or the chunked
  // combination's own
  uint2* coef;
  // chunked combination (rlc_chunked)
  uint32_t *pcnt, *pcoff, *pcf, *pcc;
  uint4* coef4;
  G1J* t1;
  G2J* t2;
  // small calls (no bfe)
  Fp4Entry* f1;
  uint8_t* f1bad;
  G2JEntry* f1S;
  RlcKey key;
  bool learned;  // decompress recorded Dev::kl_ev for this call (resolve joins it)
  // the learned keys' ladder tables for the key sides of the combinations: the partials' keys and
  // the DV keys (ent null unless this call's keys came through the learned cache's lookup)
  KeyWideRef kw, akw;
  // batched subgroup test (subg_batch; subg_skip: its record alone)
  SubgArgs sg;
};

// chunks of the chunked combination (an upper bound: a group's last chunk may be short)
uint32_t rlc_chunk_count(const VerifyPlan& p) { return (uint32_t)(p.n / p.rlc_cmax + p.n_groups); }

// Same buffers, sizes and conditions whatever the phases do with them: wsbuf synchronises when a
// buffer grows, so none is taken that the plan does not use.
int verify_bufs(Ws& w, const VerifyPlan& p, VerifyBufs& b) {
  const size_t n = p.n, n_agg = p.n_agg, n_groups = p.n_groups, gcap = p.gcap, nbcap = p.nbcap;
  if (wsbuf(w, W_VPK, n, &b.vpk) || wsbuf(w, W_VPKST, n, &b.vpkst) || wsbuf(w, W_VSIG, n, &b.vsig) ||
      wsbuf(w, W_VSIGST, n, &b.vsigst) || wsbuf(w, W_IGRP, n, &b.igrp) || wsbuf(w, W_PR, n, &b.pr) ||
      wsbuf(w, W_SR, n, &b.sr) || wsbuf(w, W_GP, gcap, &b.gP) || wsbuf(w, W_GST, gcap, &b.gst) ||
      wsbuf(w, W_GMSG, n_groups, &b.gmsg) || wsbuf(w, W_GVER, n_groups, &b.gver) ||
      wsbuf(w, W_GLINES, gcap * N_LINES, &b.glines) || wsbuf(w, W_LIST, n + n_agg, &b.list) ||
      wsbuf(w, W_COUNT, 1, &b.count) || wsbuf(w, W_FBLINES, p.fbcap * N_LINES, &b.fbl))
    return -1;
  if (n_agg && (wsbuf(w, W_APK, n_agg, &b.apk) || wsbuf(w, W_APKST, n_agg, &b.apkst) ||
                wsbuf(w, W_ASIG, n_agg, &b.asig) || wsbuf(w, W_APR, n_agg, &b.apr) || wsbuf(w, W_ASR, n_agg, &b.asr)))
    return -1;
  if (p.first_only && wsbuf(w, W_FIRST, 2, &b.wfirst)) return -1;
  if (p.bfe && (wsbuf(w, W_FBUF, 3 * gcap, &b.fbuf) || wsbuf(w, W_GS, gcap, &b.gS) || wsbuf(w, W_BS, nbcap, &b.bS) ||
                wsbuf(w, W_BLINES, nbcap * N_LINES, &b.blines) || wsbuf(w, W_BBAD, nbcap, &b.bbad) ||
                wsbuf(w, W_BVER, nbcap, &b.bver) || wsbuf(w, W_GLIST, gcap, &b.glist) ||
                wsbuf(w, W_GCOUNT, 1, &b.gcount) || wsbuf(w, W_PFIN, 3 * 2 * std::max<size_t>(nbcap, 1), &b.pfin) ||
                wsbuf(w, W_TBUF, 3 * nbcap, &b.tbuf)))
    return -1;
  G2MsmArgs& ma = b.ma;
  if (p.smsm && (wsbuf(w, W_MCNT, MSM_KEYS, &ma.cnt) || wsbuf(w, W_MOFF, MSM_KEYS + 1, &ma.off) ||
                 wsbuf(w, W_MCUR, MSM_KEYS, &ma.cur) || wsbuf(w, W_MORDER, MSM_KEYS, &ma.order) ||
                 wsbuf(w, W_MENT, 2 * MSM_WINDOWS * (n + n_agg), &ma.ent) ||
                 wsbuf(w, W_MBUCKET, MSM_KEYS, &ma.bucket) || wsbuf(w, W_MPART, MSM_PARTS, &ma.part) ||
                 wsbuf(w, W_MPART2, MSM_PARTS / 128, &ma.part2) || wsbuf(w, W_MTOT, 1, &ma.total) ||
                 wsbuf(w, W_PBUF1, 3 * p.nb1, &b.pbuf1) || wsbuf(w, W_PBUF2, 3 * p.nb2, &b.pbuf2) ||
                 wsbuf(w, W_PBUF3, 3 * p.nb2, &b.pbuf3) || wsbuf(w, W_SFAIL, 2, &b.sfail) ||
                 wsbuf(w, W_MLEV, N_LINES * gcap, &b.mlev)))
    return -1;
  SubgArgs& sg = b.sg;
  if (p.subg_batch && (wsbuf(w, W_SGDIG, SG_WINDOWS * n, &sg.dig) || wsbuf(w, W_SGCNT, SG_KEYS, &sg.cnt) ||
                       wsbuf(w, W_SGOFF, SG_KEYS + 1, &sg.off) || wsbuf(w, W_SGCUR, SG_KEYS, &sg.cur) ||
                       wsbuf(w, W_SGORDER, SG_KEYS, &sg.order) || wsbuf(w, W_SGENT, SG_WINDOWS * n, &sg.ent) ||
                       wsbuf(w, W_SGBUCKET, SG_KEYS, &sg.bucket) || wsbuf(w, W_SGCLS, SG_CLASSES, &sg.cls) ||
                       wsbuf(w, W_SGSUMS, SG_SUMS, &sg.sums)))
    return -1;
  if ((p.subg_batch || p.subg_skip) && wsbuf(w, W_SGREC, 2, &sg.rec)) return -1;
  if ((p.rlc_chunked || p.smsm) && wsbuf(w, W_COEF, n + n_agg, &b.coef)) return -1;
  const size_t max_chunks = rlc_chunk_count(p);
  if (p.rlc_chunked &&
      (wsbuf(w, W_PCNT, n_groups, &b.pcnt) || wsbuf(w, W_PCOFF, n_groups + 1, &b.pcoff) ||
       wsbuf(w, W_PCFIRST, max_chunks, &b.pcf) || wsbuf(w, W_PCCOUNT, max_chunks, &b.pcc) ||
       wsbuf(w, W_RT1, 4 * n, &b.t1) || wsbuf(w, W_RT2, 4 * n, &b.t2) || (p.sparse && wsbuf(w, W_COEF4, n, &b.coef4))))
    return -1;
  if (!p.bfe && (wsbuf(w, W_F1, 3 * 2 * gcap, &b.f1) || wsbuf(w, W_F1BAD, gcap, &b.f1bad) || wsbuf(w, W_F1S, gcap, &b.f1S)))
    return -1;
  return rlc_key(b.key) ? -1 : 0;
}

// The signatures of a large call (plan subg_batch / subg_skip), on side 1: the square roots as ever
// (ev_dec behind them: the aggregation's ladders start there), then the batched subgroup test --
// digits, counting sort, bucket sums, class sums, the 20 weighted sums and their verdict -- and the
// per-item ladders behind its flag: launched always, they return at once when every sum was in G2
// and run exactly as without the test when one was not, so the host never waits and every status
// and zeroed point is the ladders' own.  subg_skip (the adaptive history expects a failure): the
// ladders alone, counting what they find.  Either way the call's record goes to the history.
int verify_subgroup_batch(Dev& d, Ws& w, const VerifyCall& c, const VerifyPlan& p, VerifyBufs& b) {
  hipStream_t s1 = w.side[1];
  const uint32_t n = (uint32_t)p.n;
  SubgArgs& sg = b.sg;
  SubgCtr* ctr = (SubgCtr*)d.sg_ctr.p;
  HCHK(hipMemsetAsync(sg.rec, 0, 2 * sizeof(uint32_t), s1));
  if (p.subg_skip) {
    TIMED(d, "k_dec_sig_pt", s1, launch_dec_sig_pt(c.sigs, n, b.vsig, b.vsigst, s1, nullptr, w.ev_dec, ctr, sg.rec + 1));
    TIMED(d, "k_subg_skipped", s1, launch_subg_skipped(ctr, s1));
  } else {
    HCHK(hipMemsetAsync(sg.cnt, 0, SG_KEYS * sizeof(uint32_t), s1));
    HCHK(hipMemsetAsync(sg.cur, 0, SG_KEYS * sizeof(uint32_t), s1));
    TIMED(d, "k_dec_sig_pt", s1, launch_dec_sig_sqrt(c.sigs, n, b.vsig, b.vsigst, s1, nullptr));
    HCHK(hipEventRecord(w.ev_dec, s1));
    sg.sig = b.vsig;
    sg.sig_st = b.vsigst;
    sg.n = n;
    sg.key = b.key;
    sg.ctr = ctr;
    TIMED(d, "k_subg_digits", s1, launch_subg_digits(sg, s1));
    TIMED(d, "k_subg_count", s1, launch_subg_count(sg, s1));
    TIMED(d, "k_subg_scan", s1, launch_scan(sg.cnt, SG_KEYS, sg.off, s1));
    TIMED(d, "k_subg_fill", s1, launch_subg_fill(sg, s1));
    TIMED(d, "k_subg_bucket", s1, launch_subg_bucket(sg, s1));
    TIMED(d, "k_subg_class", s1, launch_subg_class(sg.bucket, sg.cls, s1));
    TIMED(d, "k_subg_weigh", s1, launch_subg_weigh(sg.cls, sg.sums, s1));
    TIMED(d, "k_subg_verdict", s1, launch_subg_verdict(sg.sums, sg.rec, ctr, s1));
    TIMED(d, "k_g2_subgroup", s1, launch_g2_subgroup(n, b.vsig, b.vsigst, s1, nullptr, sg.rec, ctr, sg.rec + 1));
  }
  // the call's outcome for the next calls' choice (read when its event has completed)
  if (p.adaptive && d.sres_head - d.sres_tail < N_RES) {
    const unsigned k = d.sres_head % N_RES;
    d.sres_host[k].skipped = p.subg_skip ? 1 : 0;
    HCHK(hipMemcpyAsync(d.sres_host[k].rec, sg.rec, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s1));
    HCHK(hipEventRecord(d.sres_ev[k], s1));
    d.sres_head++;
  }
  return 0;
}

// Decompress: the fork onto the side streams, the public keys from one of four sources, the
// signatures, and the learned key cache's chain (Dev::kl_ev)
int verify_decompress(Dev& d, Ws& w, const VerifyCall& c, const VerifyPlan& p, VerifyBufs& b) {
  const TaFold* fold = c.fold;
  const size_t n = p.n, n_agg = p.n_agg;
  // fork: decompression on the side streams (after the previous verification's decompression)
  HCHK(hipEventRecord(w.ev_fork, c.s));
  for (int k = 0; k < 2; k++) HCHK(hipStreamWaitEvent(w.side[k], w.ev_fork, 0));
  // public keys: from the caller's decompressed-key tables when given (static per cluster lock:
  // decompressed and subgroup-checked once); device calls without tables through the learned key
  // cache (hits copied, misses decompressed and, behind the key side, learned); else decompressed
  // here
  // (the lookup loads a key as three 16-byte words: a caller's array that is not 16-byte aligned
  // takes the plain decompression)
  const auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
  const bool learn_pk = !c.cluster && !c.key_cache && !(fold && fold->pk_table) && n && al16(c.pks);
  const bool learn_dv = !c.cluster && !c.key_cache && n_agg && !fold->dv_pk_table && al16(fold->dv_pks);
  KeyLearnTab kl{};
  uint32_t *kmiss = nullptr, *kcnt = nullptr;  // taken here: whether there is a table is only known now
  uint32_t *kent = nullptr, *kment = nullptr;
  if (learn_pk || learn_dv) {
    // the ordering chain of Dev::kl_ev: behind the last call's k_pk_learn
    if (d.kl_ev_set) HCHK(hipStreamWaitEvent(w.side[0], d.kl_ev, 0));
    if (kl_table(d, w.side[0], &kl)) return -1;
    if (kl.cap) {
      if (wsbuf(w, W_KLMISS, n + n_agg, &kmiss) || wsbuf(w, W_KLCNT, 2, &kcnt) ||
          wsbuf(w, W_KLENT, n + n_agg, &kent) || wsbuf(w, W_KLMENT, n + n_agg, &kment))
        return -1;
      HCHK(hipMemsetAsync(kcnt, 0, 2 * sizeof(uint32_t), w.side[0]));
      b.kw.ctr = b.akw.ctr = kl.ctr;
      b.kw.wide = b.akw.wide = kl.wide;
    }
  }
  if (c.cluster) {  // the cluster's own keys by (group, share index): no lookup, no miss, nothing learned
    ClusterKeysArgs ck = *c.cluster;
    ck.n = (uint32_t)n;
    ck.vpk = b.vpk;
    ck.vpkst = b.vpkst;
    ck.went = nullptr;
    ck.tables = c.cluster_wide ? 1u : 0u;
    if (c.cluster_wide) {
      if (wsbuf(w, W_KLENT, n, &kent)) return -1;
      ck.went = kent;
      b.kw.ent = kent;
      b.kw.wide = c.cluster_wide;  // (b.kw.ctr stays null: the counters are the learned cache's)
    }
    TIMED(d, "k_cluster_keys", w.side[0], launch_cluster_keys(ck, w.side[0]));
  } else if (fold && fold->pk_table) {
    b.vpk = const_cast<G1AEntry*>(fold->pk_table);
    b.vpkst = const_cast<uint8_t*>(fold->pk_table_st);
  } else if (c.key_cache && d.kc_n) {  // host-buffer call with the key cache: cached entries, the rest decompressed
    TIMED(d, "k_dec_pk", w.side[0],
          launch_pk_cached(c.pks, (uint32_t)n, (const uint8_t*)d.kc_keys.p, (const G1AEntry*)d.kc_tab.p,
                           (const uint8_t*)d.kc_st.p, (const uint32_t*)d.kc_hidx.p, (uint32_t)d.kc_tcap, g_sc_k0,
                           g_sc_k1, b.vpk, b.vpkst, w.side[0]));
  } else if (learn_pk && kl.cap) {
    if (kl_keys(d, kl, c.pks, n, b.vpk, b.vpkst, kmiss, kcnt, kent, w.side[0])) return -1;
    if (kl.wcap) b.kw.ent = kent;
  } else {
    TIMED(d, "k_dec_pk", w.side[0], launch_dec_pk(c.pks, (uint32_t)n, b.vpk, b.vpkst, w.side[0]));
  }
  HCHK(hipEventRecord(w.ev_pk, w.side[0]));
  if (n_agg && fold->dv_pk_table) {
    b.apk = const_cast<G1AEntry*>(fold->dv_pk_table);
    b.apkst = const_cast<uint8_t*>(fold->dv_pk_table_st);
  } else if (learn_dv && kl.cap) {
    if (kl_keys(d, kl, fold->dv_pks, n_agg, b.apk, b.apkst, kmiss + n, kcnt + 1, kent + n, w.side[0])) return -1;
    if (kl.wcap) b.akw.ent = kent + n;
  } else if (n_agg) {
    TIMED(d, "k_dec_pk", w.side[0], launch_dec_pk(fold->dv_pks, (uint32_t)n_agg, b.apk, b.apkst, w.side[0]));
  }
  if (c.pre_sig) {
    b.vsig = const_cast<HmEntry*>(c.pre_sig);
    b.vsigst = const_cast<uint8_t*>(c.pre_sigst);
    HCHK(hipEventRecord(w.ev_dec, w.side[1]));
  } else if (p.subg_batch || p.subg_skip) {
    if (verify_subgroup_batch(d, w, c, p, b)) return -1;
  } else {
    TIMED(d, "k_dec_sig_pt", w.side[1],
          launch_dec_sig_pt(c.sigs, (uint32_t)n, b.vsig, b.vsigst, w.side[1], nullptr, w.ev_dec));
  }
  HCHK(hipEventRecord(w.ev_side[0], w.side[0]));
  HCHK(hipEventRecord(w.ev_side[1], w.side[1]));
  // the misses into the table, behind everything that waits for the keys; the next call's lookup
  // (on any workspace set) waits for kl_ev, and so does the end of this call: k_pk_learn reads the
  // caller's key bytes and this set's buffers
  b.learned = kl.cap != 0;
  if (b.learned) {
    if (learn_pk)
      TIMED(d, "k_pk_learn", w.side[0],
            launch_pk_learn(kl, c.pks, (uint32_t)n, kmiss, kcnt, g_sc_k0, g_sc_k1, b.vpk, b.vpkst, kment, w.side[0]));
    if (learn_dv)
      TIMED(d, "k_pk_learn", w.side[0],
            launch_pk_learn(kl, fold->dv_pks, (uint32_t)n_agg, kmiss + n, kcnt + 1, g_sc_k0, g_sc_k1, b.apk, b.apkst,
                            kment + n, w.side[0]));
    HCHK(hipEventRecord(d.kl_ev, w.side[0]));
    d.kl_ev_set = true;
  }
  return 0;
}

// Fold: the slot's ThresholdAggregate on side 3 (needs the decompressed partials when it reuses them)
int verify_fold(Dev& d, Ws& w, const VerifyCall& c, VerifyBufs& b) {
  const TaFold* fold = c.fold;
  if (!(fold && fold->n_groups)) return 0;
  hipStream_t st = w.side[3];
  HCHK(hipStreamWaitEvent(st, w.ev_fork, 0));
  const HmEntry* pts = b.vsig;
  const uint8_t* mst_in = b.vsigst;
  hipEvent_t mst_ready = nullptr, pts_ready = nullptr;
  if (fold->ta_src) {  // the points once decompressed; their subgroup statuses before the digits
    pts_ready = w.ev_dec;
    mst_ready = w.ev_side[1];
  } else {  // the aggregation members come as their own bytes: decompress them here
    HmEntry* tpts;
    uint8_t* tdst;
    if (wsbuf(w, W_TAPTS, fold->n_partials, &tpts) || wsbuf(w, W_TADST, fold->n_partials, &tdst)) return -1;
    TIMED(d, "k_dec_sig_pt", st, launch_dec_sig_pt(fold->ta_sigs, (uint32_t)fold->n_partials, tpts, tdst, st));
    pts = tpts;
    mst_in = tdst;
  }
  if (ta_tail(d, w, pts, fold->ta_src, mst_in, fold->ta_idx, fold->grp_off, fold->n_groups, fold->n_partials, 0,
              fold->ta_out, fold->ta_status, b.asig, st, mst_ready, pts_ready))
    return -1;
  HCHK(hipEventRecord(w.ev_ta, st));
  return 0;
}

// the chunked combination's launch (the first pass; the slot-wide check's guarded second pass
// changes its sides and guard)
RlcMsmArgs rlc_chunk_args(const VerifyPlan& p, const VerifyBufs& b) {
  RlcMsmArgs ra{};
  ra.pk = b.vpk;
  ra.pk_st = b.vpkst;
  ra.sig = b.vsig;
  ra.sig_st = b.vsigst;
  ra.cfirst = b.pcf;
  ra.ccount = b.pcc;
  ra.total = b.pcoff + p.n_groups;
  ra.key_base = 0;
  ra.key = b.key;
  ra.coef = b.coef;
  ra.coef4 = b.coef4;
  ra.sparse = p.sparse ? 1 : 0;
  ra.t1 = b.t1;
  ra.t2 = b.t2;
  ra.pout = b.pr;
  ra.sout = b.sr;
  ra.always = p.item_always;
  ra.sides = p.sides1;
  ra.kw = b.kw;
  return ra;
}

// Combine: random linear combinations per item, then per group (the partials' keys only: the DV
// keys' decompression behind them on side 0 is waited for by the aggregates' combination below)
int verify_combine(Dev& d, Ws& w, const VerifyCall& c, const VerifyPlan& p, VerifyBufs& b) {
  hipStream_t s = c.s;
  const size_t n = p.n, n_agg = p.n_agg;
  HCHK(hipStreamWaitEvent(s, w.ev_pk, 0));
  if (!p.keys_only) HCHK(hipStreamWaitEvent(s, w.ev_side[1], 0));  // (vplan.h keys_only)
  TIMED(d, "k_item_group", s, launch_item_group(c.grp_off, (uint32_t)p.n_groups, (uint32_t)n, b.igrp, s));
  if (p.rlc_chunked) {
    TIMED(d, "k_plan", s, launch_plan(c.grp_off, (uint32_t)p.n_groups, p.rlc_cmax, b.pcnt, b.pcoff, b.pcf, b.pcc, s));
    TIMED(d, "k_rlc", s, launch_rlc_msm(rlc_chunk_args(p, b), rlc_chunk_count(p), s));
  } else {
    TIMED(d, "k_rlc", s,
          launch_rlc(b.vpk, b.vpkst, p.keys_only ? nullptr : b.vsig, p.keys_only ? nullptr : b.vsigst, b.igrp,
                     c.grp_off, p.item_always, (uint32_t)n, 0, b.key, b.pr, b.sr, s, b.coef, p.sides1, nullptr, b.kw));
    HCHK(hipStreamWaitEvent(s, w.ev_side[1], 0));  // the groups' states below read the signatures
  }
  if (n_agg) {
    // without the batched final exponentiation the folded aggregate keeps r = 1: one coefficient
    // per combination may be fixed without losing soundness (an invalid aggregate alone fails the
    // combined check exactly; with an invalid partial j beside it the check passes for one value
    // of the random r_j only) -- the group's items all take random coefficients (item_always)
    //
    // Key side only (sides1 1, the slot-wide check's MSM takes the signature side): the DV keys
    // are all it reads, so it runs beside the slot's ThresholdAggregate; the aggregates' statuses
    // and points are applied where the signature side is read (group_scan's with_agg, msm_take)
    const bool key_side = p.sides1 == 1;
    if (!key_side) HCHK(hipStreamWaitEvent(s, w.ev_ta, 0));
    HCHK(hipStreamWaitEvent(s, w.ev_side[0], 0));
    TIMED(d, "k_rlc", s,
          launch_rlc(b.apk, b.apkst, key_side ? nullptr : b.asig, key_side ? nullptr : c.fold->ta_status, nullptr,
                     nullptr, p.bfe ? 1 : 0, (uint32_t)n_agg, (uint32_t)n, b.key, b.apr, b.asr, s,
                     p.try_msm ? b.coef + n : nullptr, p.sides1, nullptr, b.akw));
    HCHK(hipStreamWaitEvent(s, w.ev_ta, 0));  // the groups' states below read the aggregates
  }
  // small calls (no batched final exponentiation): the groups' sums and signature lines do not
  // need the hashed messages, so they overlap the hashing; the wait comes before the pairing
  if (c.hm_ready && p.bfe) HCHK(hipStreamWaitEvent(s, c.hm_ready, 0));
  if (c.defer_msgs && !p.lines_at_p)  // the per-batch check reads the unevaluated lines
    TIMED(d, "k_lines_msg", s, launch_lines_msg(c.defer_hm, (uint32_t)c.defer_msgs, s));
  return 0;
}

// the groups [g0, g0 + ng) of one chunk: their sums, states and signature lines
GroupPrepArgs group_prep_args(const VerifyCall& c, const VerifyPlan& p, const VerifyBufs& b, size_t g0, uint32_t ng) {
  GroupPrepArgs ga{};
  ga.keys_only = p.keys_only ? 1 : 0;
  ga.grp_off = c.grp_off;
  ga.g0 = (uint32_t)g0;
  ga.ng = ng;
  ga.msg_idx = c.msg_idx;
  ga.hm = c.hm;
  ga.pk = b.vpk;
  ga.pk_st = b.vpkst;
  ga.sig = b.vsig;
  ga.sig_st = b.vsigst;
  ga.pr = b.pr;
  ga.sr = b.sr;
  if (p.n_agg) {
    ga.agg_pk = b.apk;
    ga.agg_pk_st = b.apkst;
    ga.agg_sig = b.asig;
    ga.agg_st = c.fold->ta_status;
    ga.agg_pr = b.apr;
    ga.agg_sr = b.asr;
  }
  ga.gP = b.gP;
  ga.gmsg = b.gmsg;
  ga.gst = b.gst;
  ga.glines = b.glines;
  return ga;
}
// the chunk's (P_g, H(m_g)) Miller loops, stored unexponentiated in fbuf
Pair3Args group_loops_args(const VerifyCall& c, const VerifyBufs& b, size_t g0, uint32_t ng) {
  Pair3Args pm{};
  pm.pk = b.gP;
  pm.pk_st = b.gst;
  pm.msg_idx = b.gmsg + g0;
  pm.hm = c.hm;
  pm.sig_lines = b.glines;
  pm.stride = ng;
  pm.n = ng;
  pm.f_out = b.fbuf;
  return pm;
}
// behind a batched check (slot-wide or per-batch): the groups of a failing batch (glist) one by
// one, their stored loop times their own S lines' loop
int group_recheck(Dev& d, const VerifyCall& c, const VerifyBufs& b, size_t g0, uint32_t ng) {
  hipStream_t s = c.s;
  TIMED(d, "k_slines", s, launch_slines(b.gS, b.glist, b.gcount, ng, b.glines, ng, nullptr, s));
  Pair3Args pg{};
  pg.sig_lines = b.glines;
  pg.stride = ng;
  pg.n = ng;
  pg.list = b.glist;
  pg.count = b.gcount;
  pg.f_in = b.fbuf;
  pg.f_range = 1;
  pg.f_n = ng;
  pg.status = b.gver + g0;
  TIMED(d, "k_pair3_fin", s, launch_pair3_fin(pg, s));
  return 0;
}

// Group check, slot-wide (plan smsm; one chunk holds every group), with its guarded per-batch fallback
int check_slot_wide(Dev& d, Ws& w, const VerifyCall& c, const VerifyPlan& p, VerifyBufs& b, size_t g0, uint32_t ng) {
  hipStream_t s = c.s;
  const size_t n = p.n, n_agg = p.n_agg, mmlk = p.mmlk;
  const bool skip_msm = p.skip_msm;
  uint8_t* sfail = b.sfail;
  GroupPrepArgs ga = group_prep_args(c, p, b, g0, ng);
  Pair3Args pm = group_loops_args(c, b, g0, ng);
  // the groups' public-key sides and states; then beside each other: the (P_g, H(m_g))
  // Miller loops and their product tree (s), the MSM of the signature side and its lines (side 0)
  ga.fe_batch = FE_BATCH;
  ga.p_only = 1;
  TIMED(d, "k_group_prep", s, launch_group_prep(ga, s));
  if (skip_msm) HCHK(hipMemsetAsync(sfail, 1, 1, s));  // the per-batch check runs unconditionally
  HCHK(hipEventRecord(w.ev_msm, s));
  hipStream_t sm = w.side[0];
  if (!skip_msm) {
    G2MsmArgs& ma = b.ma;
    // the bucket counters zeroed before the wait (side 0 is idle since the keys' decompression;
    // under three slots these fills wait for free CUs: ~1 ms on the check's chain otherwise)
    HCHK(hipMemsetAsync(ma.cnt, 0, MSM_KEYS * sizeof(uint32_t), sm));
    HCHK(hipMemsetAsync(ma.cur, 0, MSM_KEYS * sizeof(uint32_t), sm));
    HCHK(hipStreamWaitEvent(sm, w.ev_msm, 0));
    ma.sig = b.vsig;
    ma.sig_st = b.vsigst;
    ma.agg_sig = b.asig;
    ma.agg_st = n_agg ? c.fold->ta_status : nullptr;
    ma.coef = b.coef;
    ma.igrp = b.igrp;
    ma.gst = b.gst;
    ma.n = (uint32_t)n;
    ma.n_agg = (uint32_t)n_agg;
    TIMED(d, "k_msm_count", sm, launch_msm_count(ma, sm));
    TIMED(d, "k_msm_scan", sm, launch_scan(ma.cnt, MSM_KEYS, ma.off, sm));
    TIMED(d, "k_msm_fill", sm, launch_msm_fill(ma, sm));
    TIMED(d, "k_msm_bucket", sm, launch_msm_bucket(ma, sm));
    TIMED(d, "k_msm_reduce", sm, launch_msm_reduce(ma, sm));
    TIMED(d, "k_msm_sum", sm, launch_msm_sum(ma, sm));
    // the signature side's Miller loop, beside the multi-Miller loops and their product tree:
    // the final exponentiation's second factor, pfin[1] (lines and loop in one kernel, k_lml)
    TIMED(d, "k_pair3_mls", sm, launch_lml(ma.total, 1, b.pfin, 1, 1, b.bbad, sm));
  }
  HCHK(hipEventRecord(w.ev_side[0], sm));
  // multi-Miller loops over mmlk groups (shared squarings), then a product tree of fan-in
  // PROD_FAN down to ONE value, pfin[0] (ping-pong between pbuf1 and pbuf2): eight products
  // per level in each lane group instead of a chain of 64
  Pair3Args pp{};
  pp.pk = b.gP;
  pp.pk_st = b.gst;
  pp.msg_idx = b.gmsg + g0;
  pp.hm = c.hm;
  pp.n = (uint32_t)((ng + mmlk - 1) / mmlk);
  pp.f_range = (uint32_t)mmlk;
  pp.f_n = ng;
  pp.f_out = b.pbuf1;
  pp.sig_lines = b.mlev;
  if (p.lines_at_p) TIMED(d, "k_lines_at_p", s, launch_lines_at_p(pp, b.mlev, s));
  else TIMED(d, "k_mml_eval", s, launch_mml_eval(pp, b.mlev, s));
  TIMED(d, "k_pair3_mml", s, launch_pair3_mml(pp, s));
  Fp4Entry* cur = b.pbuf1;
  uint32_t cur_n = pp.n;
  if (!skip_msm) do {
    Pair3Args pt{};
    pt.n = (cur_n + PROD_FAN - 1) / PROD_FAN;
    pt.f_in = cur;
    pt.f_range = PROD_FAN;
    pt.f_n = cur_n;
    pt.f_out = pt.n == 1 ? b.pfin : (cur == b.pbuf2 ? b.pbuf3 : b.pbuf2);
    TIMED(d, "k_pair3_prod", s, launch_pair3_prod(pt, s));
    cur = pt.f_out;
    cur_n = pt.n;
  } while (cur_n > 1);
  HCHK(hipStreamWaitEvent(s, w.ev_side[0], 0));
  if (!skip_msm) {
    Pair3Args pf{};
    pf.pk_st = b.bbad;
    pf.n = 1;
    pf.f_in = b.pfin;
    pf.f_range = 2;
    pf.f_n = 2;
    pf.status = sfail;
    TIMED(d, "k_pair3_fin", s, launch_pair6_fin(pf, s));
    HCHK(hipMemsetAsync(sfail + 1, 0, 1, s));
    TIMED(d, "k_slot_verdict", s, launch_slot_verdict(b.gst, sfail, ng, b.gver + g0, s));
    // deferred lines: read by the per-batch check behind a failed slot-wide check and by
    // the per-item fallback of any group that was not READY (k_slot_verdict sets sfail[1])
    if (p.lines_at_p)
      TIMED(d, "k_lines_msg", s, launch_lines_msg(c.defer_hm, (uint32_t)c.defer_msgs, s, sfail + 1));
    // the slot-wide check failed: the per-batch check (signature sides per item and group;
    // computed in the first pass when the check was skipped)
    if (p.rlc_chunked) {
      RlcMsmArgs ra = rlc_chunk_args(p, b);
      ra.sides = 2;
      ra.guard = sfail;
      TIMED(d, "k_rlc", s, launch_rlc_msm(ra, rlc_chunk_count(p), s));
    } else {
      TIMED(d, "k_rlc", s,
            launch_rlc(b.vpk, b.vpkst, b.vsig, b.vsigst, b.igrp, c.grp_off, 1, (uint32_t)n, 0, b.key, b.pr, b.sr, s,
                       b.coef, 2, sfail));
    }
    if (n_agg)
      TIMED(d, "k_rlc", s,
            launch_rlc(b.apk, b.apkst, b.asig, c.fold->ta_status, nullptr, nullptr, 1, (uint32_t)n_agg, (uint32_t)n,
                       b.key, b.apr, b.asr, s, b.coef + n, 2, sfail));
  }
  ga.p_only = 0;
  ga.guard = sfail;
  pm.guard = sfail;
  // the per-batch check over the multi-Miller loops' chunks (mmlk consecutive groups): their
  // stored loops (pbuf1) are the batches' public-key sides, so no group's (P_g, H(m_g)) loop
  // is recomputed unless its batch fails.  Per batch: the signature sides S_g summed, the
  // lines of the sum, its loop times the stored one, one final exponentiation (3 lanes: one
  // round of waves for the chip-sized batch count, where six lanes would take two)
  const uint32_t nbm = (uint32_t)((ng + mmlk - 1) / mmlk);
  ga.gS = b.gS;
  ga.bS = nullptr;
  ga.fe_batch = 1;
  TIMED(d, "k_group_prep", s, launch_group_prep(ga, s));
  TIMED(d, "k_group_prep", s, launch_batch_sum(b.gS, ng, (uint32_t)mmlk, b.bS, s, sfail));
  TIMED(d, "k_slines", s, launch_slines(b.bS, nullptr, nullptr, nbm, b.blines, nbm, b.bbad, s, sfail));
  Pair3Args pb{};
  pb.sig_lines = b.blines;
  pb.stride = nbm;
  pb.n = nbm;
  pb.f_in = b.pbuf1;
  pb.f_range = 1;
  pb.f_n = nbm;
  pb.pk_st = b.bbad;
  pb.status = b.bver;
  pb.guard = sfail;
  TIMED(d, "k_pair3_fin", s, launch_pair3_fin(pb, s));
  HCHK(hipMemsetAsync(b.gcount, 0, sizeof(uint32_t), s));
  if (b.wseg)
    TIMED(d, "k_seg_batch_verdict", s,
          launch_seg_batch_verdict(b.gst, b.bver, ng, b.gver + g0, b.glist, b.gcount, s, sfail, (uint32_t)mmlk,
                                   (uint32_t)g0, c.gseg, c.n_seg, b.wseg));
  else
    TIMED(d, "k_batch_verdict", s,
          launch_batch_verdict(b.gst, b.bver, ng, b.gver + g0, b.glist, b.gcount, s, sfail, (uint32_t)mmlk, b.wfirst,
                               (uint32_t)g0));
  // groups of a failing batch: their own (P_g, H(m_g)) loops, then each group alone below
  pm.list = b.glist;
  pm.count = b.gcount;
  TIMED(d, "k_pair3_ml", s, launch_pair3_ml(pm, s));
  // the call's outcome for the next calls' choice (read when its event has completed)
  if (p.adaptive && d.res_head - d.res_tail < N_RES) {
    const unsigned k = d.res_head % N_RES;
    d.res_host[k].skipped = skip_msm ? 1 : 0;
    HCHK(hipMemcpyAsync(&d.res_host[k].sfail, sfail, 1, hipMemcpyDeviceToHost, s));
    HCHK(hipMemcpyAsync(&d.res_host[k].gcount, b.gcount, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HCHK(hipEventRecord(d.res_ev[k], s));
    d.res_head++;
  }
  return group_recheck(d, c, b, g0, ng);
}

// Group check, per batch of FE_BATCH groups (plan bfe, below the slot-wide check's size)
int check_per_batch(Dev& d, const VerifyCall& c, const VerifyPlan& p, VerifyBufs& b, size_t g0, uint32_t ng) {
  hipStream_t s = c.s;
  const uint32_t fb = FE_BATCH;
  const uint32_t nb = (ng + fb - 1) / fb;
  GroupPrepArgs ga = group_prep_args(c, p, b, g0, ng);
  ga.fe_batch = fb;
  ga.gS = b.gS;
  ga.bS = b.bS;
  TIMED(d, "k_group_prep", s, launch_group_prep(ga, s));
  // the (P_g, H(m_g)) Miller loops, stored unexponentiated
  TIMED(d, "k_pair3_ml", s, launch_pair3_ml(group_loops_args(c, b, g0, ng), s));
  // per batch: the lines of sum_g S_g, one Miller loop times the batch's stored loops, one
  // final exponentiation
  const uint8_t* guard = nullptr;
  TIMED(d, "k_slines", s, launch_slines(b.bS, nullptr, nullptr, nb, b.blines, nb, b.bbad, s, guard));
  // the batches' signature-side loops (pfin[2b + 1]), the product trees of their stored loops
  // (fan-in PROD_FAN, the last level into pfin[2b]), then each batch's final exponentiation
  // multiplies just the two.  All on s: with several slots in flight a side stream here would
  // share a hardware queue with another slot's long kernels (C2 24.4 vs 19.1 ms per slot)
  Pair3Args ps{};
  ps.sig_lines = b.blines;
  ps.stride = nb;
  ps.n = nb;
  ps.f_out = b.pfin;
  ps.f_out_stride = 2;
  ps.f_out_off = 1;
  ps.guard = guard;
  TIMED(d, "k_pair3_mls", s, launch_pair3_mls(ps, s));
  const Fp4Entry* cur = b.fbuf;
  uint32_t cur_n = ng, span = 1;
  while (span < fb) {
    const uint32_t fan = std::min<uint32_t>(PROD_FAN, fb / span);
    Pair3Args pt{};
    pt.n = (cur_n + fan - 1) / fan;
    pt.f_in = cur;
    pt.f_range = fan;
    pt.f_n = cur_n;
    pt.guard = guard;
    span *= fan;
    if (span == fb) {
      pt.f_out = b.pfin;
      pt.f_out_stride = 2;
    } else {
      pt.f_out = b.tbuf;
    }
    TIMED(d, "k_pair3_prod", s, launch_pair3_prod(pt, s));
    cur = pt.f_out;
    cur_n = pt.n;
  }
  Pair3Args pf{};
  pf.pk_st = b.bbad;
  pf.n = nb;
  pf.f_in = b.pfin;
  pf.f_range = 2;
  pf.f_n = 2 * nb;
  pf.status = b.bver;
  pf.guard = guard;
  TIMED(d, "k_pair3_fin", s, launch_pair6_fin(pf, s));
  // groups of a failing batch: checked one by one (their stored loop, their own S lines)
  HCHK(hipMemsetAsync(b.gcount, 0, sizeof(uint32_t), s));
  if (b.wseg)
    TIMED(d, "k_seg_batch_verdict", s,
          launch_seg_batch_verdict(b.gst, b.bver, ng, b.gver + g0, b.glist, b.gcount, s, guard, fb, (uint32_t)g0, c.gseg,
                                   c.n_seg, b.wseg));
  else
    TIMED(d, "k_batch_verdict", s,
          launch_batch_verdict(b.gst, b.bver, ng, b.gver + g0, b.glist, b.gcount, s, guard, fb, b.wfirst, (uint32_t)g0));
  return group_recheck(d, c, b, g0, ng);
}

// Group check of small calls (no batched final exponentiation): every group on its own.
// These calls are single Verifies and small batches, latency-bound: each group's sums (S kept
// Jacobian, no lines), then its signature side's Miller loop -- lines produced and consumed in
// one kernel (k_lml) -- on side stream 0 while the messages still hash; after the hashing (not
// its lines) the (P, H(m)) loop the same way on s, beside it; then ONE six-lane final
// exponentiation of the two stored loops (f1[2g], f1[2g + 1])
int check_small(Dev& d, Ws& w, const VerifyCall& c, const VerifyPlan& p, VerifyBufs& b, size_t g0, uint32_t ng) {
  hipStream_t s = c.s;
  GroupPrepArgs ga = group_prep_args(c, p, b, g0, ng);
  ga.skip_hm = 1;
  ga.gS = b.f1S;
  ga.bS = nullptr;
  ga.fe_batch = 1;
  TIMED(d, "k_group_prep", s, launch_group_prep(ga, s));
  hipStream_t sl = w.side[0];
  HCHK(hipEventRecord(w.ev_msm, s));
  HCHK(hipStreamWaitEvent(sl, w.ev_msm, 0));
  TIMED(d, "k_pair3", sl, launch_lml(b.f1S, ng, b.f1, 2, 1, nullptr, sl));
  HCHK(hipEventRecord(w.ev_side[0], sl));
  if (g0 == 0 && (c.h_ready || c.hm_ready)) HCHK(hipStreamWaitEvent(s, c.h_ready ? c.h_ready : c.hm_ready, 0));
  LmlArgs pa{};
  pa.pk = b.gP;
  pa.pk_st = b.gst;
  pa.msg_idx = b.gmsg + g0;
  pa.hm = c.hm;
  pa.n = ng;
  pa.f_out = b.f1;
  pa.f_stride = 2;
  pa.bad = b.f1bad;
  TIMED(d, "k_pair3", s, launch_lml_p(pa, s));
  HCHK(hipStreamWaitEvent(s, w.ev_side[0], 0));
  Pair3Args pf{};
  pf.pk_st = b.f1bad;
  pf.n = ng;
  pf.f_in = b.f1;
  pf.f_range = 2;
  pf.f_n = 2 * ng;
  pf.status = b.gver + g0;
  TIMED(d, "k_pair3", s, launch_pair6_fin(pf, s));
  return 0;
}

// Resolve: the groups' verdicts to their items, every item of a failing group on its own, the
// first-error reduction, and the joins of what ran beside the call
int verify_resolve(Dev& d, Ws& w, const VerifyCall& c, const VerifyPlan& p, VerifyBufs& b) {
  hipStream_t s = c.s;
  const TaFold* fold = c.fold;
  const size_t n = p.n, n_agg = p.n_agg;
  // the per-item fallback reads the messages' lines (the small calls' group checks did not wait)
  if (!p.bfe && c.hm_ready && c.h_ready) HCHK(hipStreamWaitEvent(s, c.hm_ready, 0));
  HCHK(hipMemsetAsync(b.count, 0, sizeof(uint32_t), s));
  ScatterArgs sa{};
  sa.n = (uint32_t)n;
  sa.item_grp = b.igrp;
  sa.msg_idx = c.msg_idx;
  sa.hm = c.hm;
  sa.pk = b.vpk;
  sa.pk_st = b.vpkst;
  sa.sig = b.vsig;
  sa.sig_st = b.vsigst;
  sa.gverdict = b.gver;
  sa.grp_off = c.grp_off;
  sa.n_agg = (uint32_t)n_agg;
  if (n_agg) {
    sa.ta_status = fold->ta_status;
    sa.agg_pk = b.apk;
    sa.agg_pk_st = b.apkst;
    sa.agg_sig = b.asig;
    sa.agg_status = fold->agg_status;
  }
  sa.status = c.status;
  sa.list = b.list;
  sa.count = b.count;
  if (b.wseg) {  // first_only per segment: each segment's first failing group, and only its items re-checked
    TIMED(d, "k_seg_first_group", s, launch_seg_first_group(b.gver, (uint32_t)p.n_groups, c.gseg, c.n_seg, b.wseg, s));
    TIMED(d, "k_seg_scatter", s, launch_seg_scatter(sa, c.gseg, c.n_seg, b.wseg, s));
  } else {
    if (p.first_only) {
      TIMED(d, "k_first_group", s, launch_first_group(b.gver, (uint32_t)p.n_groups, b.wfirst + 1, s));
      sa.first_group = b.wfirst + 1;
    }
    TIMED(d, "k_scatter", s, launch_scatter(sa, s));
  }
  // fallback: every item of a failing group on its own; passes beyond the list end exit at once
  for (size_t base = 0; base < n + n_agg; base += p.fbcap) {
    TIMED(d, "k_fb_lines", s,
          launch_fb_lines(b.list, b.count, (uint32_t)base, (uint32_t)p.fbcap, b.vsig, b.asig, (uint32_t)n, b.fbl, s));
    Pair3Args pa{};
    pa.pk = b.vpk;
    pa.msg_idx = c.msg_idx;
    pa.hm = c.hm;
    pa.sig_lines = b.fbl;
    pa.stride = (uint32_t)p.fbcap;
    pa.n = (uint32_t)p.fbcap;
    pa.list = b.list;
    pa.count = b.count;
    pa.base = (uint32_t)base;
    pa.n_items = (uint32_t)n;
    pa.agg_pk = b.apk;
    pa.agg_msg = b.gmsg;
    pa.status = c.status;
    pa.agg_status = n_agg ? fold->agg_status : nullptr;
    TIMED(d, "k_pair3_fallback", s, launch_pair3(pa, s));
  }
  if (c.first_out) {
    HCHK(hipMemsetAsync(c.first_out, 0xff, sizeof(uint32_t), s));
    TIMED(d, "k_first_item", s, launch_first_item(c.status, (uint32_t)n, c.first_out, s));
  }
  if (c.seg_first_out) {
    HCHK(hipMemsetAsync(c.seg_first_out, 0xff, std::max<size_t>(c.n_seg, 1) * sizeof(uint32_t), s));
    TIMED(d, "k_seg_first_item", s,
          launch_seg_first_item(c.status, c.item_seg, c.item_arrival, (uint32_t)n, c.seg_first_out, c.n_seg, s));
  }
  if (fold && fold->n_groups && !n_agg) {  // the aggregation ran beside the verification: join it
    HCHK(hipStreamWaitEvent(s, w.ev_ta, 0));
  }
  if (b.learned) HCHK(hipStreamWaitEvent(s, d.kl_ev, 0));  // (recorded by this call: d.mu is still held)
  return 0;
}

// HBLS_STATS=1: count the fallback items (synchronises; tests and diagnosis)
int verify_stats(const VerifyCall& c, const VerifyPlan& p, const VerifyBufs& b) {
  hipStream_t s = c.s;
  uint32_t k = 0;
  HCHK(hipMemcpyAsync(&k, b.count, sizeof(k), hipMemcpyDeviceToHost, s));
  HCHK(hipStreamSynchronize(s));
  g_stats[0] += p.n + p.n_agg;
  g_stats[1] += p.n_groups;
  g_stats[2] += k;
  if (p.bfe) {  // only the last chunk's count is still in gcount: enough for the tests' sizes
    HCHK(hipMemcpyAsync(&k, b.gcount, sizeof(k), hipMemcpyDeviceToHost, s));
    HCHK(hipStreamSynchronize(s));
    g_stats[3] += k;
  }
  if (p.try_msm) {
    uint8_t f = 0;
    HCHK(hipMemcpyAsync(&f, b.sfail, 1, hipMemcpyDeviceToHost, s));
    HCHK(hipStreamSynchronize(s));
    g_stats[4] += 1;
    g_stats[5] += f ? 1 : 0;
  }
  return 0;
}

// One verification, every verifying entry point's end: plan, buffers, then the phases in the
// order they enqueue.  Fills c.vsig / c.vsigst.
int verify_pipeline(Dev& d, Ws& w, VerifyCall& c) {
  const VerifyKnobs knobs{g_gcap.load(),         g_fbcap.load(),     g_fe_batch_min.load(),
                          g_slot_msm_min.load(), g_rlc_lanes.load(), g_adaptive.load(), g_subg_batch_min.load()};
  VerifyShape sh{};
  sh.n = c.n;
  sh.n_groups = c.n_groups;
  sh.n_agg = (c.fold && c.fold->dv_pks) ? c.fold->n_groups : 0;
  sh.grouped = c.grp_off != nullptr;
  sh.first_error = c.first_out != nullptr || c.gseg != nullptr;
  if (c.gseg && (c.first_out || !c.grp_off || !c.item_seg || !c.item_arrival || !c.seg_first_out))
    return set_err("verify: a segmented call takes group offsets, the items' segments and arrival indices, no first_out");
  sh.defer_msgs = c.defer_msgs;
  sh.n_cu = d.n_cu;
  // the adaptive history, read by the calls that could take the slot-wide check: the outcomes of
  // the checked calls that have completed since (never a synchronisation)
  if (knobs.adaptive && vp_slot_wide(sh, knobs))
    while (d.res_tail != d.res_head && hipEventQuery(d.res_ev[d.res_tail % N_RES]) == hipSuccess) {
      const SlotRes& r = d.res_host[d.res_tail % N_RES];
      d.attack = r.skipped ? r.gcount != 0 : r.sfail != 0;
      d.res_tail++;
    }
  sh.attack = d.attack;
  // likewise the batched subgroup test's: after a failed test the ladders run alone, until a call's
  // ladders find nothing off G2
  sh.own_sigs = c.device_entry && !c.pre_sig;
  if (knobs.adaptive && vp_subg_wide(sh, knobs))
    while (d.sres_tail != d.sres_head && hipEventQuery(d.sres_ev[d.sres_tail % N_RES]) == hipSuccess) {
      const SubgRes& r = d.sres_host[d.sres_tail % N_RES];
      d.subg_failed = r.skipped ? r.rec[1] != 0 : r.rec[0] != 0;
      d.sres_tail++;
    }
  sh.subg_failed = d.subg_failed;
  VerifyPlan p;
  if (const char* refused = verify_plan(sh, knobs, p)) return set_err(refused);
  VerifyBufs b{};
  if (verify_bufs(w, p, b)) return -1;
  c.vsig = b.vsig;
  c.vsigst = b.vsigst;
  if (p.first_only) HCHK(hipMemsetAsync(b.wfirst, 0xff, 2 * sizeof(uint32_t), c.s));
  if (p.first_only && c.gseg) {
    const size_t words = 2 * std::max<size_t>(c.n_seg, 1);
    if (wsbuf(w, W_SEGFIRST, words, &b.wseg)) return -1;
    HCHK(hipMemsetAsync(b.wseg, 0xff, words * sizeof(uint32_t), c.s));
  }
  if (verify_decompress(d, w, c, p, b) || verify_fold(d, w, c, b) || verify_combine(d, w, c, p, b)) return -1;
  for (size_t g0 = 0; g0 < p.n_groups; g0 += p.gcap) {
    const uint32_t ng = (uint32_t)std::min(p.gcap, p.n_groups - g0);
    if (p.smsm ? check_slot_wide(d, w, c, p, b, g0, ng)
        : p.bfe ? check_per_batch(d, c, p, b, g0, ng)
                : check_small(d, w, c, p, b, g0, ng))
      return -1;
  }
  if (verify_resolve(d, w, c, p, b)) return -1;
  return stats_on() ? verify_stats(c, p, b) : 0;
}

// hash every distinct message to G2 (+ its Miller line chain) into hm, on stream s
int hash_messages(Dev& d, const uint8_t* dmsg, const uint64_t* doff, const uint32_t* dlen, size_t n_msgs,
                  MsgEntry* hm, hipStream_t s, bool lines = true) {
  TIMED(d, "k_hash_to_g2", s, launch_hash_to_g2(dmsg, doff, dlen, (uint32_t)n_msgs, hm, s));
  if (lines) TIMED(d, "k_lines_msg", s, launch_lines_msg(hm, (uint32_t)n_msgs, s));
  return 0;
}

// hgroup.h defer_lines at the run-time threshold of the batched final exponentiation
bool defer_lines(size_t n_groups, size_t n_msgs) { return hb::defer_lines(n_groups, n_msgs, g_fe_batch_min.load()); }

// ---------------------------------------------------------------------------------------
// Host-buffer calls: staging, message dedup, multi-device sharding
// ---------------------------------------------------------------------------------------
// Hash messages first .. first + count - 1 of an uploaded table (dmsg, doff, dlen; entries in hm)
// on w's side stream 2 -- beside the decompression the verification forks next -- behind what
// stream `after` holds now (the table's upload, a chunk's gather; ev_ta is free until the
// verification).  The verification waits on w.ev_h before it needs H(m) and on w.ev_side[2] before
// it needs the messages' lines (computed here unless deferred).
int hash_range(Dev& d, Ws& w, hipStream_t after, const uint8_t* dmsg, const uint64_t* doff, const uint32_t* dlen,
               MsgEntry* hm, size_t first, size_t count, bool lines) {
  HCHK(hipEventRecord(w.ev_ta, after));
  hipStream_t hs = w.side[2];
  HCHK(hipStreamWaitEvent(hs, w.ev_ta, 0));
  TIMED(d, "k_hash_to_g2", hs, launch_hash_to_g2(dmsg, doff + first, dlen + first, (uint32_t)count, hm + first, hs));
  HCHK(hipEventRecord(w.ev_h, hs));
  if (lines) TIMED(d, "k_lines_msg", hs, launch_lines_msg(hm + first, (uint32_t)count, hs));
  HCHK(hipEventRecord(w.ev_side[2], hs));
  return 0;
}

// Upload the distinct messages (the call's stream) and hash them: there, or with a workspace on
// its side stream 2 (hash_range).
int hash_table(Dev& d, const MsgTable& t, MsgEntry** hm_out, bool lines, Hc* h = nullptr, Ws* w = nullptr) {
  uint8_t* dmsg;
  uint64_t* doff;
  uint32_t* dlen;
  void* hm;
  if (upload(d, I_MSG, t.bytes.data(), t.bytes.size(), &dmsg, h)) return -1;
  if (upload(d, I_OFF, t.off.data(), t.off.size(), &doff, h)) return -1;
  if (upload(d, I_LEN, t.len.data(), t.len.size(), &dlen, h)) return -1;
  if (ensure_buf(call_io(d, h)[I_HM], t.len.size() * sizeof(MsgEntry), &hm)) return -1;
  *hm_out = (MsgEntry*)hm;
  hipStream_t hs = call_stream(d, h);
  if (w) return hash_range(d, *w, hs, dmsg, doff, dlen, *hm_out, 0, t.len.size(), lines);
  return hash_messages(d, dmsg, doff, dlen, t.len.size(), *hm_out, hs, lines);
}

// The host-call contexts a call holds: one (waited for) and whatever idle ones it adds
// (hc_try_acquire), all released when the call returns.
struct HcLease {
  Dev& d;
  std::vector<Hc*> h;
  explicit HcLease(Dev& dev) : d(dev), h{&hc_acquire(dev)} {}
  HcLease(const HcLease&) = delete;
  ~HcLease() {
    for (size_t c = h.size(); c-- > 0;) hc_release(d, *h[c]);
  }
};

// The shard runner of every call that works per shard (fan_out_k, duty_add, the cluster calls): fn(k) for
// every k < nd, on the calling thread when nd == 1 and otherwise on one host thread per shard, all joined
// before this returns.  Returns the first failing k with that thread's error text in *err, or nd.
size_t run_shards(size_t nd, const std::function<int(size_t)>& fn, std::string* err) {
  std::vector<int> rc(nd, 0);
  std::vector<std::string> errs(nd);
  auto run = [&](size_t k) {
    rc[k] = fn(k);
    if (rc[k]) errs[k] = g_err;
  };
  if (nd == 1) {
    run(0);
  } else {
    std::vector<std::thread> th;
    for (size_t k = 0; k < nd; k++) th.emplace_back(run, k);
    for (auto& t : th) t.join();
  }
  for (size_t k = 0; k < nd; k++)
    if (rc[k]) {
      *err = errs[k];
      return k;
    }
  return nd;
}

// A failing shard's error, reported with its device: "who: device N: err" ("device N: err" without a who)
int shard_err(const std::string& who, const Dev& d, const std::string& err) {
  return set_err((who.empty() ? "" : who + ": ") + "device " + std::to_string(d.ord) + ": " + err);
}

// run_shards over the shards of a handle (a duty's, a cluster's), the first failing shard's error reported with its device
template <class Shard>
int each_shard(const std::string& who, const std::vector<Shard>& sh, const std::function<int(size_t)>& fn) {
  std::string err;
  const size_t bad = run_shards(sh.size(), fn, &err);
  return bad == sh.size() ? 0 : shard_err(who, *sh[bad].d, err);
}

// Run fn(dev, shard) for each device's shard of n_units concurrently (one host thread per extra
// device); a failing shard's error is reported with its device.  fn locks the device itself.
// fan_out_k: fn also learns which shard it runs, k of nd.
using ShardFn = std::function<int(Dev&, size_t, size_t)>;
using ShardKFn = std::function<int(Dev&, size_t, size_t, size_t, size_t)>;
int fan_out_k(size_t n_units, const ShardKFn& fn) {
  const std::vector<Dev*> ds = devs();
  const size_t nd = std::min(ds.size(), std::max<size_t>(n_units, 1));
  if (nd <= 1) return fn(*ds[0], 0, 1, 0, n_units);
  std::string err;
  const size_t bad = run_shards(nd, [&](size_t k) { return fn(*ds[k], k, nd, n_units * k / nd, n_units * (k + 1) / nd); }, &err);
  return bad == nd ? 0 : shard_err("", *ds[bad], err);
}
int fan_out(size_t n_units, const ShardFn& fn) {
  return fan_out_k(n_units, [&fn](Dev& d, size_t, size_t, size_t b, size_t e) -> int { return fn(d, b, e); });
}

// fan_out with the device locked throughout (the small entry points)
int for_each_device(size_t n_units, const ShardFn& fn) {
  return fan_out(n_units, [&fn](Dev& d, size_t b, size_t e) -> int {
    std::lock_guard<std::mutex> lk(d.mu);
    if (hipSetDevice(d.ord) != hipSuccess) return set_err("hipSetDevice failed");
    return fn(d, b, e);
  });
}

// fan_out for the heavy host-buffer calls: each device's share runs in a host-call context
// (acquired before the device lock); fn may release the lock once everything is enqueued and then
// wait for its own stream only
using HcFn = std::function<int(Dev&, Hc&, size_t, size_t, std::unique_lock<std::mutex>&)>;
int for_each_device_hc(size_t n_units, const HcFn& fn) {
  return fan_out(n_units, [&fn](Dev& d, size_t b, size_t e) -> int {
    HcLease hcs(d);
    std::unique_lock<std::mutex> lk(d.mu);
    if (hipSetDevice(d.ord) != hipSuccess) return set_err("hipSetDevice failed");
    return fn(d, *hcs.h[0], b, e, lk);
  });
}

// Decompress m compressed keys into entries first .. first+m-1 of d's key table (grown, keeping
// the entries before `first`).  Caller holds d.mu.
int kc_fill(Dev& d, const uint8_t* keys, size_t first, size_t m) {
  HCHK(hipSetDevice(d.ord));
  // launches enqueued earlier may still read the table: its only reader, launch_pk_cached of a
  // host-buffer verification, runs on a workspace side stream, so the library's own streams (the
  // library stream, the host-call contexts' and the workspaces' side streams) are drained before
  // any entry is rewritten or the table moves -- not the whole device: caller, torch and RCCL
  // streams keep running.  No new reader can be enqueued meanwhile (they look indices up under
  // d.mu, held here); cache adds are rare (cluster locks).
  if (drain_lib_streams(d)) return -1;
  const size_t tot = first + m;
  if (d.kc_tab.cap < tot * sizeof(G1AEntry) || d.kc_st.cap < tot) {  // grow, keeping the old entries
    DevBuf nt, ns;
    void* p;
    if (ensure_buf(nt, tot * sizeof(G1AEntry), &p) || ensure_buf(ns, tot, &p)) return -1;
    if (first) {
      HCHK(hipMemcpyAsync(nt.p, d.kc_tab.p, first * sizeof(G1AEntry), hipMemcpyDeviceToDevice, d.stream));
      HCHK(hipMemcpyAsync(ns.p, d.kc_st.p, first, hipMemcpyDeviceToDevice, d.stream));
      HCHK(hipStreamSynchronize(d.stream));
    }
    if (d.kc_tab.p) HCHK(hipFree(d.kc_tab.p));
    if (d.kc_st.p) HCHK(hipFree(d.kc_st.p));
    d.kc_tab = nt;
    d.kc_st = ns;
  }
  uint8_t* dpk;
  if (upload(d, I_PK, keys, 48 * m, &dpk)) return -1;
  TIMED(d, "k_dec_pk", d.stream,
        launch_dec_pk(dpk, (uint32_t)m, (G1AEntry*)d.kc_tab.p + first, (uint8_t*)d.kc_st.p + first, d.stream));
  // the keys and the device index (grown to >= 2 x the entries: every entry re-inserted)
  if (d.kc_keys.cap < tot * 48) {
    DevBuf nk;
    void* p;
    if (ensure_buf(nk, tot * 48, &p)) return -1;
    if (first) HCHK(hipMemcpyAsync(nk.p, d.kc_keys.p, first * 48, hipMemcpyDeviceToDevice, d.stream));
    HCHK(hipStreamSynchronize(d.stream));
    if (d.kc_keys.p) HCHK(hipFree(d.kc_keys.p));
    d.kc_keys = nk;
  }
  HCHK(hipMemcpyAsync((uint8_t*)d.kc_keys.p + 48 * first, dpk, 48 * m, hipMemcpyDeviceToDevice, d.stream));
  size_t tcap = std::max<size_t>(d.kc_tcap, 1024);
  while (tcap < 2 * tot) tcap *= 2;
  size_t from = first;
  if (tcap != d.kc_tcap || first < d.kc_n) {  // a new index: every entry
    void* p;
    if (ensure_buf(d.kc_hidx, tcap * sizeof(uint32_t), &p)) return -1;
    HCHK(hipMemsetAsync(d.kc_hidx.p, 0, tcap * sizeof(uint32_t), d.stream));
    d.kc_tcap = tcap;
    from = 0;
  }
  TIMED(d, "k_kc_index", d.stream,
        launch_kc_index((const uint8_t*)d.kc_keys.p, (uint32_t)from, (uint32_t)(tot - from), (uint32_t*)d.kc_hidx.p,
                        (uint32_t)tcap, g_sc_k0, g_sc_k1, d.stream));
  HCHK(hipStreamSynchronize(d.stream));
  d.kc_n = tot;
  return 0;
}


// ---- decompressed-signature cache (Dev::sc_*; kernels in vbatch.hip).  Both run under d.mu.
// sc_ready: the device's cache at the current capacity (allocated on first use; a capacity change
// drops the old contents), false when the cache is off.
hipEvent_t sc_event(Dev& d) {
  hipEvent_t e = nullptr;
  if (!d.sc_ev_pool.empty()) {
    e = d.sc_ev_pool.back();
    d.sc_ev_pool.pop_back();
  } else if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
    return nullptr;
  }
  return e;
}
// drop the records of completed puts and gets (wait: block until every one has completed)
void sc_prune(Dev& d, bool wait) {
  std::deque<Dev::ScPut> live_puts;
  for (Dev::ScPut& p : d.sc_inflight) {
    if (wait) (void)hipEventSynchronize(p.done);
    if (wait || hipEventQuery(p.done) == hipSuccess) {
      d.sc_ev_pool.push_back(p.pipe);
      d.sc_ev_pool.push_back(p.done);
    } else {
      live_puts.push_back(p);
    }
  }
  d.sc_inflight.swap(live_puts);
  std::vector<hipEvent_t> live;
  for (hipEvent_t e : d.sc_gets) {
    if (wait) (void)hipEventSynchronize(e);
    if (wait || hipEventQuery(e) == hipSuccess) d.sc_ev_pool.push_back(e);
    else live.push_back(e);
  }
  d.sc_gets.swap(live);
}
bool sc_ready(Dev& d, bool alloc) {
  const size_t cap = g_sc_cap.load();
  if (cap == 0) return false;
  if (d.sc_cap == cap) return true;
  if (!alloc) return false;
  sc_prune(d, true);  // the buffers may be reallocated: nothing may still use them
  void* p;
  if (ensure_buf(d.sc_key, cap * 96, &p) || ensure_buf(d.sc_ent, cap * sizeof(HmEntry), &p) ||
      ensure_buf(d.sc_st, cap, &p) || ensure_buf(d.sc_tab, 2 * cap * sizeof(uint32_t), &p))
    return false;
  if (hipMemset(d.sc_tab.p, 0, 2 * cap * sizeof(uint32_t)) != hipSuccess) return false;
  d.sc_cap = cap;
  d.sc_cursor = d.sc_filled = 0;
  return true;
}
// After a Verify batch's pipeline on s: its m signatures (bytes in group order, sig: in the staging
// buffers of the host-call context `owner`) and their decompressed points and statuses (pts, st:
// the verification's workspace w) enter the ring on the owner's put stream; the workspace is
// released behind the put -- or on s when nothing is put -- and the owner's next call waits for it
// (hc_ready).
int sc_put_release(Dev& d, Ws& w, const uint8_t* sig, const HmEntry* pts, const uint8_t* st, size_t m, hipStream_t s,
                   Hc& owner) {
  if (!m || !sc_ready(d, true)) return ws_release(w, s);
  const size_t cap = d.sc_cap;
  if (m > cap) {  // only the last cap items fit
    sig += 96 * (m - cap);
    pts += m - cap;
    st += m - cap;
    m = cap;
  }
  sc_prune(d, false);
  if (!owner.put_s) HCHK(hipStreamCreateWithFlags(&owner.put_s, hipStreamNonBlocking));
  if (!owner.put_ev) HCHK(hipEventCreateWithFlags(&owner.put_ev, hipEventDisableTiming));
  hipStream_t ps = owner.put_s;
  hipEvent_t pipe = sc_event(d), done = sc_event(d);
  if (!pipe || !done) return set_err("signature cache: no event");
  HCHK(hipEventRecord(pipe, s));
  HCHK(hipStreamWaitEvent(ps, pipe, 0));
  for (hipEvent_t g : d.sc_gets) HCHK(hipStreamWaitEvent(ps, g, 0));
  // an in-flight put [q, q + mq) (absolute positions, before this one's [P, P + m)) shares ring
  // entries with this one only if some position of this one lies a whole ring after one of its:
  // P + m - 1 - q >= cap (only when more than the ring is in flight)
  for (const Dev::ScPut& p : d.sc_inflight)
    if (p.pos + cap < d.sc_pos + m) HCHK(hipStreamWaitEvent(ps, p.done, 0));
  TIMED(d, "k_sc_put", ps,
        launch_sc_put(sig, pts, st, (uint32_t)m, (uint32_t)d.sc_cursor, (uint32_t)cap, d.sc_key.p, (HmEntry*)d.sc_ent.p,
                      (uint8_t*)d.sc_st.p, (uint32_t*)d.sc_tab.p, (uint32_t)(2 * cap), g_sc_k0, g_sc_k1, ps));
  HCHK(hipEventRecord(done, ps));
  // sig lives in the owner context's staging buffers: its next call waits for this put
  HCHK(hipEventRecord(owner.put_ev, ps));
  owner.put_pending = true;
  d.sc_inflight.push_back({d.sc_cursor, m, d.sc_pos, pipe, done});
  d.sc_cursor = (d.sc_cursor + m) & (cap - 1);
  d.sc_pos += m;
  d.sc_filled = std::min(cap, d.sc_filled + m);
  return ws_release(w, ps);
}
// before an aggregation's decompression: the cached points of its n members into pts / st, hit[i]
// set for those (k_dec_sig_pt then skips them).  Returns whether the cache was consulted.  Never
// waits for a Verify still in its pipeline: the entries its put will write are misses.
bool sc_get(Dev& d, const uint8_t* sig, size_t n, HmEntry* pts, uint8_t* st, uint8_t* hit, hipStream_t s) {
  if (!n || !d.sc_filled || !sc_ready(d, false)) return false;
  sc_prune(d, false);
  // puts whose pipeline is done: wait for them; the others: their span is a range of misses
  uint64_t busy_first = 0, busy_end = 0;
  bool busy = false;
  for (const Dev::ScPut& p : d.sc_inflight) {
    if (hipEventQuery(p.pipe) == hipSuccess) {
      if (hipStreamWaitEvent(s, p.done, 0) != hipSuccess) return false;
      continue;
    }
    if (!busy) busy_first = p.pos;
    busy = true;
    busy_end = p.pos + p.m;
  }
  size_t busy_lo = 0, busy_len = 0;
  if (busy) {
    if (busy_end - busy_first >= d.sc_cap) return false;  // every entry may be rewritten
    busy_lo = (size_t)(busy_first & (d.sc_cap - 1));
    busy_len = (size_t)(busy_end - busy_first);
  }
  hipEvent_t e = sc_event(d);
  if (!e) return false;
  TIMED(d, "k_sc_get", s,
        launch_sc_get(sig, (uint32_t)n, d.sc_key.p, (const HmEntry*)d.sc_ent.p, (const uint8_t*)d.sc_st.p,
                      (const uint32_t*)d.sc_tab.p, (uint32_t)(2 * d.sc_cap), g_sc_k0, g_sc_k1, pts, st, hit,
                      (uint32_t)d.sc_cap, (uint32_t)busy_lo, (uint32_t)busy_len, s));
  if (hipEventRecord(e, s) != hipSuccess) return false;
  d.sc_gets.push_back(e);
  return true;
}

// HBLS_HOST_TIMING=1: phases of a host-buffer Verify batch on stderr (diagnosis)
static bool host_timing() {
  static const bool on = [] {
    const char* v = getenv("HBLS_HOST_TIMING");
    return v && v[0] == '1';
  }();
  return on;
}
static double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// One enqueued chunk of a host-buffer Verify -- a whole call, one device's shard of it, or one
// chunk of a large call.  vc names the chunk's device buffers (keys and signatures in group order,
// msg_idx, the group offsets, hm, the deferred range, status, first_out); its messages were hashed
// by hash_range on workspace w.  Verifies it on stream s (w released behind it), then enters its
// decompressed signatures into the signature cache (the aggregation of these partials reads them)
// through the context `owner`, whose staging buffers hold vc.sigs.
int verify_chunk(Dev& d, Ws& w, VerifyCall& vc, hipStream_t s, Hc& owner) {
  vc.s = s;
  vc.hm_ready = w.ev_side[2];
  vc.h_ready = w.ev_h;
  // the key cache is looked up on the device (k_pk_cached): its tables are only rewritten under
  // Dev::mu, held while this call enqueues, after every launch that may still read them
  vc.key_cache = true;
  return verify_pipeline(d, w, vc) || sc_put_release(d, w, vc.sigs, vc.vsig, vc.vsigst, vc.n, s, owner) ? -1 : 0;
}

// The bracket of a chunk whose keys and signatures went up in the caller's order (pk, sig): its m
// items `ord` gathered into group order on the device before the verification, their statuses
// scattered back to the caller's positions after it.
int gather_items(const uint8_t* pk, const uint8_t* sig, const uint32_t* ord, size_t m, uint8_t* gpk, uint8_t* gsig,
                 hipStream_t s) {
  LAUNCH(k_gather_items, m, s, (const uint4*)pk, (const uint4*)sig, ord, (uint32_t)m, (uint4*)gpk, (uint4*)gsig);
  return 0;
}
int scatter_status(const uint8_t* st, const uint32_t* ord, size_t m, uint8_t* st_out, hipStream_t s) {
  LAUNCH(k_scatter_status, m, s, st, ord, (uint32_t)m, st_out);
  return 0;
}

// the distinct messages of a host call: the parallel dedup for large calls on hosts with the threads
void dedup_call(const uint8_t* msgs, const uint64_t* msg_off, const uint32_t* msg_len, size_t n, MsgTable& all) {
  const unsigned hw = std::thread::hardware_concurrency();
  if (n >= (1u << 16) && hw >= 4)
    dedup_messages_par(msgs, msg_off, msg_len, n, all, hw >= 8 ? 8u : 4u);
  else
    dedup_messages(msgs, msg_off, msg_len, n, nullptr, all);
}

// A large one-device Verify batch.  Its keys and signatures go up in the caller's order while the
// host groups them (message dedup and sort, ~7-12 ms for a slot's million partials: beside the
// PCIe upload instead of in front of it); then the groups run in chunks of whole groups, each on
// its own host-call context (stream) and workspace set, so that -- like consecutive slots in
// flight -- one chunk's gather, decompression and hashing overlap the previous chunk's pairings
// and latency-bound tail.  Each chunk gathers its items in group order on the device
// (k_gather_items), hashes its own contiguous range of the message table (items are sorted by
// message; chunks only when every message has one group), verifies, enters its signatures into
// the signature cache and scatters its statuses into the call's status array, downloaded once.
// Extra contexts are taken only if idle (hc_try_acquire).
constexpr size_t CHUNK_MIN_ITEMS = size_t(1) << 18;
int verify_large(Dev& d, const uint8_t* pks, const uint8_t* sigs, const uint8_t* msgs, const uint64_t* msg_off,
                 const uint32_t* msg_len, size_t n, uint8_t* status) {
  const double t_start = now_ms();
  HcLease hcs(d);
  Hc& h0 = *hcs.h[0];
  std::unique_lock<std::mutex> lk(d.mu);
  if (hipSetDevice(d.ord) != hipSuccess) return set_err("hipSetDevice failed");
  const double t_locked0 = now_ms();
  // 1. keys and signatures up in the caller's order
  uint8_t *rpk, *rsig;
  if (upload(d, I_PK, pks, 48 * n, &rpk, &h0) || upload(d, I_SIG, sigs, 96 * n, &rsig, &h0)) return -1;
  lk.unlock();
  const double t_up = now_ms();
  // 2. the grouping on the host, beside the upload (hgroup.h): message ids, items ordered by
  // message, groups of <= HBLS_GROUP_MAX items over one message
  MsgTable all;
  dedup_call(msgs, msg_off, msg_len, n, all);
  const size_t nm = all.len.size();
  const MsgGroups g = group_by_message(all.idx.data(), n, nm, std::max<size_t>(1, g_gmax.load()));
  const bool defer = defer_lines(g.n_groups(), nm);
  // chunks (one per idle context, messages of one group each) at group starts, ~n / K items each
  const size_t k_want = defer ? std::min<size_t>((size_t)g_ws_sets, std::max<size_t>(1, n / CHUNK_MIN_ITEMS)) : 1;
  for (Hc* x; hcs.h.size() < k_want && (x = hc_try_acquire(d));) hcs.h.push_back(x);
  const size_t K = hcs.h.size();
  const ChunkSplit cs = split_chunks(g.gstart.data(), g.n_groups(), K);
  const double t_grouped = now_ms();
  lk.lock();
  const double t_locked = now_ms();
  // 3. the grouping up (pinned: queued behind the raw upload without waiting for it), then the chunks
  uint32_t *dord, *dmidx, *dlen, *dgoffs;
  uint8_t* dmsg;
  uint64_t* doff;
  void *hmp, *stp, *gp;
  PinnedUploads up;
  up.add(I_IDX, g.order.data(), n, &dord);
  up.add(I_MIDX, g.midx.data(), n, &dmidx);
  up.add(I_MSG, all.bytes.data(), all.bytes.size(), &dmsg);
  up.add(I_OFF, all.off.data(), all.off.size(), &doff);
  up.add(I_LEN, all.len.data(), all.len.size(), &dlen);
  up.add(I_VGOFF, cs.goffs.data(), cs.goffs.size(), &dgoffs);
  if (upload_pinned(d, h0, up) || ensure_buf(h0.io[I_HM], nm * sizeof(MsgEntry), &hmp) ||
      ensure_buf(h0.io[I_HM2], n, &stp) || ensure_buf(h0.io[I_OUT], 144 * n, &gp))
    return -1;
  MsgEntry* hm = (MsgEntry*)hmp;
  uint8_t* dst_out = (uint8_t*)stp;
  uint8_t *gpk = (uint8_t*)gp, *gsig = gpk + 48 * n;  // group order
  HCHK(hipEventRecord(h0.ev, h0.s));
  for (size_t c = 0; c < cs.n_chunks(); c++) {
    Hc& hc = *hcs.h[c];
    hipStream_t sc = hc.s;
    if (c) HCHK(hipStreamWaitEvent(sc, h0.ev, 0));
    const size_t ib = g.gstart[cs.cg[c]], m = g.gstart[cs.cg[c + 1]] - ib;
    // the chunk's messages: all of them for one chunk, else its contiguous range
    const size_t mfirst = K == 1 ? 0 : g.midx[ib], mcount = K == 1 ? nm : g.midx[ib + m - 1] + 1 - g.midx[ib];
    VerifyCall vc;
    vc.n = m;
    vc.n_groups = cs.cg[c + 1] - cs.cg[c];
    // deferred lines per chunk: verify_pipeline decides its batched final exponentiation from the
    // chunk's own group count, so a chunk below that size computes its lines here
    const bool cdefer = defer && defer_lines(vc.n_groups, mcount);
    Ws& w = ws_acquire(d, sc);
    void* sio;
    if (ensure_buf(hc.io[I_STAT], m, &sio)) return -1;
    uint8_t *cpk = gpk + 48 * ib, *csig = gsig + 96 * ib;
    if (gather_items(rpk, rsig, dord + ib, m, cpk, csig, sc) ||
        hash_range(d, w, sc, dmsg, doff, dlen, hm, mfirst, mcount, !cdefer))
      return -1;
    vc.pks = cpk;
    vc.sigs = csig;
    vc.msg_idx = dmidx + ib;
    vc.grp_off = dgoffs + cs.goff_base[c];
    vc.hm = hm;
    vc.defer_hm = hm + mfirst;
    vc.defer_msgs = cdefer ? mcount : 0;
    vc.status = (uint8_t*)sio;
    if (verify_chunk(d, w, vc, sc, h0) || scatter_status(vc.status, dord + ib, m, dst_out, sc)) return -1;
    if (c) {
      HCHK(hipEventRecord(hc.ev, sc));
      HCHK(hipStreamWaitEvent(h0.s, hc.ev, 0));
    }
  }
  lk.unlock();  // enqueued: other callers may enqueue while this one waits
  const double t_enq = now_ms();
  HCHK(hipMemcpyAsync(status, dst_out, n, hipMemcpyDeviceToHost, h0.s));
  HCHK(hipStreamSynchronize(h0.s));
  if (host_timing())
    fprintf(stderr, "hbls verify_large n=%zu chunks=%zu: lock %.2f ms, upload enqueue %.2f, grouping %.2f (beside the "
            "upload), lock wait %.2f, enqueue %.2f, device %.2f\n", n, cs.n_chunks(), t_locked0 - t_start,
            t_up - t_locked0, t_grouped - t_up, t_locked - t_grouped, t_enq - t_locked, now_ms() - t_enq);
  return 0;
}

// Verify n host-buffer items (tbls.Verify per item): items are ordered by message and grouped
// (at most HBLS_GROUP_MAX per group, hgroup.h), the groups sharded over the devices, statuses
// scattered back.
int verify_host(const uint8_t* pks, const uint8_t* sigs, const uint8_t* msgs, const uint64_t* msg_off,
                const uint32_t* msg_len, size_t n, uint8_t* status) {
  if (n == 0) return 0;
  if (n >= 0xffffffffull) return set_err("verify batch: too many items");
  {
    const std::vector<Dev*> ds = devs();
    if (ds.size() == 1 && n >= 2 * CHUNK_MIN_ITEMS && g_ws_sets > 1)
      return verify_large(*ds[0], pks, sigs, msgs, msg_off, msg_len, n, status);
  }
  const double t_start = now_ms();
  MsgTable all;
  dedup_call(msgs, msg_off, msg_len, n, all);
  // a call below the batched final exponentiation's size (the latency-bound small calls, e.g. the
  // coalesced single-item callers) checks every item alone: a group of several items needs random
  // coefficients, i.e. a 64-bit scalar ladder per item on the call's critical path (~3.7 ms for a
  // lone lane), where separate checks only add lanes to kernels that have them to spare
  // (HBLS_SINGLE_MAX at init, hbls_single_max at run time: items below which every item is its own
  // group; default the batched final exponentiation's group threshold)
  const size_t gmax = call_gmax(n, g_single_max.load(), g_fe_batch_min.load(), g_gmax.load());
  const MsgGroups g = group_by_message(all.idx.data(), n, all.len.size(), gmax);
  const double t_grouped = now_ms();
  return for_each_device_hc(g.n_groups(), [&](Dev& d, Hc& h, size_t gb, size_t ge, std::unique_lock<std::mutex>& lk) -> int {
    const size_t ib = g.gstart[gb], ie = g.gstart[ge], m = ie - ib;
    if (m == 0) return 0;
    const bool whole = gb == 0 && ge == g.n_groups();
    const uint32_t* ord = g.order.data() + ib;  // the shard's items
    // host preparation without the device lock (other callers enqueue meanwhile).  One device
    // taking every group uses the whole call's table; several devices each dedup their shard's
    // messages and upload only its keys and signatures, in group order
    lk.unlock();
    MsgTable tl;
    std::vector<uint8_t> hpk, hsig;
    if (!whole) {
      const std::vector<size_t> items(ord, ord + m);
      dedup_messages(msgs, msg_off, msg_len, m, items.data(), tl);
      hpk.resize(48 * m);
      hsig.resize(96 * m);
      for (size_t k = 0; k < m; k++) {
        memcpy(&hpk[48 * k], pks + 48 * items[k], 48);
        memcpy(&hsig[96 * k], sigs + 96 * items[k], 96);
      }
    }
    const MsgTable& t = whole ? all : tl;
    const uint32_t* tidx = whole ? g.midx.data() : tl.idx.data();
    std::vector<uint32_t> goff;
    rebase_offsets(g.gstart.data(), gb, ge, goff);
    const double t_prep = now_ms();
    lk.lock();
    const double t_locked = now_ms();
    // the messages hash on a side stream while the keys and signatures decompress (latency of
    // one call: the two chains run side by side)
    Ws& w = ws_acquire(d, h.s);
    VerifyCall vc;
    vc.n = m;
    vc.n_groups = ge - gb;
    const bool defer = defer_lines(vc.n_groups, t.len.size());
    if (hash_table(d, t, &vc.defer_hm, !defer, &h, &w)) return -1;
    vc.hm = vc.defer_hm;
    vc.defer_msgs = defer ? t.len.size() : 0;
    uint8_t *dpk, *dsig, *dst_out = nullptr;
    uint32_t* dord = nullptr;
    void* pst;
    if (whole) {  // caller order up, group order on the device
      uint8_t *rpk, *rsig;
      void *p1, *p2;
      if (upload(d, I_PK, pks, 48 * m, &rpk, &h) || upload(d, I_SIG, sigs, 96 * m, &rsig, &h) ||
          upload(d, I_IDX, ord, m, &dord, &h) || ensure_buf(h.io[I_OUT], 144 * m, &p1) ||
          ensure_buf(h.io[I_HM2], m, &p2) || ensure_buf(h.io[I_STAT], m, &pst))
        return -1;
      dpk = (uint8_t*)p1;
      dsig = dpk + 48 * m;
      dst_out = (uint8_t*)p2;
      if (gather_items(rpk, rsig, dord, m, dpk, dsig, h.s)) return -1;
    } else if (upload(d, I_PK, hpk.data(), hpk.size(), &dpk, &h) || upload(d, I_SIG, hsig.data(), hsig.size(), &dsig, &h) ||
               ensure_buf(h.io[I_STAT], m, &pst)) {
      return -1;
    }
    uint32_t *didx, *dgoff;
    if (upload(d, I_MIDX, tidx, m, &didx, &h) || upload(d, I_VGOFF, goff.data(), goff.size(), &dgoff, &h)) return -1;
    vc.pks = dpk;
    vc.sigs = dsig;
    vc.msg_idx = didx;
    vc.grp_off = dgoff;
    vc.status = (uint8_t*)pst;
    if (verify_chunk(d, w, vc, h.s, h)) return -1;
    if (whole && scatter_status(vc.status, dord, m, dst_out, h.s)) return -1;
    lk.unlock();  // enqueued: other callers may enqueue while this one waits for its stream
    const double t_enq = now_ms();
    if (whole) {
      HCHK(hipMemcpyAsync(status, dst_out, m, hipMemcpyDeviceToHost, h.s));
      HCHK(hipStreamSynchronize(h.s));
      if (host_timing())
        fprintf(stderr, "hbls verify_host n=%zu: group %.2f ms, prep %.2f, lock wait %.2f, enqueue+upload %.2f, device %.2f\n",
                n, t_grouped - t_start, t_prep - t_grouped, t_locked - t_prep, t_enq - t_locked, now_ms() - t_enq);
      return 0;
    }
    std::vector<uint8_t> hst(m);
    HCHK(hipMemcpyAsync(hst.data(), vc.status, m, hipMemcpyDeviceToHost, h.s));
    HCHK(hipStreamSynchronize(h.s));
    for (size_t k = 0; k < m; k++) status[ord[k]] = hst[k];
    return 0;
  });
}

// First-error Verify of an ordered set (hbls_verify_batch_first_error): the callers' loops that
// stop at their first failing item -- parsigex verifies a peer's set and drops it on the first
// bad partial (core/parsigex/parsigex.go:93-98), sigagg returns on the first failure
// (core/sigagg/sigagg.go:56-63), validatorapi on the first bad submission
// (core/validatorapi/validatorapi.go:302-306).  Groups are runs of consecutive items over one
// message in the caller's order (at most HBLS_GROUP_MAX items; hgroup.h split_runs), so batches
// and groups are in item order and verify_pipeline's first-error mode resolves only the first
// failing batch's groups and the first failing group's items: under attack O(groups / batch +
// batch + group) checks instead of one per item of every failing group.  One device (the order
// must not be split).
int verify_first_host(const uint8_t* pks, const uint8_t* sigs, const uint8_t* msgs, const uint64_t* msg_off,
                      const uint32_t* msg_len, size_t n, int64_t* first, uint8_t* first_status, uint8_t* status) {
  *first = -1;
  if (first_status) *first_status = ST_OK;
  if (n == 0) return 0;
  if (n >= 0xffffffffull) return set_err("verify first error: too many items");
  MsgTable all;
  dedup_call(msgs, msg_off, msg_len, n, all);
  std::vector<uint32_t> goff;
  split_runs(all.idx.data(), n, std::max<size_t>(1, g_gmax.load()), goff);
  Dev& d = *devs()[0];
  HcLease hcs(d);
  Hc& h = *hcs.h[0];
  std::unique_lock<std::mutex> lk(d.mu);
  if (hipSetDevice(d.ord) != hipSuccess) return set_err("hipSetDevice failed");
  Ws& w = ws_acquire(d, h.s);
  VerifyCall vc;
  vc.n = n;
  vc.n_groups = goff.size() - 1;
  const bool defer = defer_lines(vc.n_groups, all.len.size());
  if (hash_table(d, all, &vc.defer_hm, !defer, &h, &w)) return -1;
  vc.hm = vc.defer_hm;
  vc.defer_msgs = defer ? all.len.size() : 0;
  uint8_t *dpk, *dsig;
  uint32_t *didx, *dgoff;
  void *pst, *pfirst;
  if (upload(d, I_PK, pks, 48 * n, &dpk, &h) || upload(d, I_SIG, sigs, 96 * n, &dsig, &h) ||
      upload(d, I_MIDX, all.idx.data(), n, &didx, &h) || upload(d, I_VGOFF, goff.data(), goff.size(), &dgoff, &h) ||
      ensure_buf(h.io[I_STAT], n, &pst) || ensure_buf(h.io[I_HM2], sizeof(uint32_t), &pfirst))
    return -1;
  vc.pks = dpk;
  vc.sigs = dsig;
  vc.msg_idx = didx;
  vc.grp_off = dgoff;
  vc.status = (uint8_t*)pst;
  vc.first_out = (uint32_t*)pfirst;
  if (verify_chunk(d, w, vc, h.s, h)) return -1;
  lk.unlock();
  uint32_t f = 0;
  std::vector<uint8_t> own;
  uint8_t* hst = status;
  if (!hst) {
    own.resize(n);
    hst = own.data();
  }
  HCHK(hipMemcpyAsync(&f, vc.first_out, sizeof(f), hipMemcpyDeviceToHost, h.s));
  HCHK(hipMemcpyAsync(hst, vc.status, n, hipMemcpyDeviceToHost, h.s));
  HCHK(hipStreamSynchronize(h.s));
  if (f != 0xffffffffu) {
    if (f >= n) return set_err("verify first error: index out of range");
    *first = (int64_t)f;
    if (first_status) *first_status = hst[f];
  }
  return 0;
}

int check_offsets(const uint32_t* grp_off, size_t n_groups) {
  if (grp_off[0] != 0) return set_err("grp_off[0] must be 0");
  for (size_t g = 0; g < n_groups; g++)
    if (grp_off[g + 1] < grp_off[g]) return set_err("grp_off must be non-decreasing");
  return 0;
}

// ThresholdAggregate (mode 0) / Aggregate (mode 1) of host-buffer groups, sharded over devices
int group_op_host(const uint8_t* sigs, const int64_t* idx, const uint32_t* grp_off, size_t n_groups, int mode,
                  uint8_t* out, uint8_t* status) {
  if (check_offsets(grp_off, n_groups)) return -1;
  const double t_start = now_ms();
  return for_each_device_hc(n_groups, [&](Dev& d, Hc& h, size_t gb, size_t ge, std::unique_lock<std::mutex>& lk) -> int {
    const size_t ng = ge - gb, pb = grp_off[gb], np = grp_off[ge] - pb;
    if (ng == 0) return 0;
    const double t_locked = now_ms();
    std::vector<uint32_t> goff;
    rebase_offsets(grp_off, gb, ge, goff);
    uint8_t* dsig;
    int64_t* didx = nullptr;
    uint32_t* dgoff;
    if (upload(d, I_SIG, sigs + 96 * pb, np * 96, &dsig, &h)) return -1;
    if (mode == 0 && upload(d, I_IDX, idx + pb, np, &didx, &h)) return -1;
    if (upload(d, I_GOFF, goff.data(), ng + 1, &dgoff, &h)) return -1;
    void *dout, *dst;
    if (ensure_buf(h.io[I_OUT], ng * 96, &dout) || ensure_buf(h.io[I_STAT], ng, &dst)) return -1;
    Ws& w = ws_acquire(d, h.s);
    HmEntry* pts;
    uint8_t *mst0, *hit = nullptr;
    if (wsbuf(w, W_TAPTS, np, &pts) || wsbuf(w, W_TADST, np, &mst0)) return -1;
    // members verified by an earlier host-buffer Verify batch come from the signature cache; the
    // rest are decompressed (the same kernels, so the same points and statuses)
    if (mode == 0 && np && d.sc_filled) {
      if (wsbuf(w, W_TAHIT, np, &hit)) return -1;
      if (!sc_get(d, dsig, np, pts, mst0, hit, h.s)) hit = nullptr;
    }
    if (np) TIMED(d, "k_dec_sig_pt", h.s, launch_dec_sig_pt(dsig, (uint32_t)np, pts, mst0, h.s, hit));
    if (ta_tail(d, w, pts, nullptr, mst0, didx, dgoff, ng, np, mode, (uint8_t*)dout, (uint8_t*)dst, nullptr, h.s))
      return -1;
    // diagnosis (HBLS_STATS / HBLS_HOST_TIMING): the cache's hit flags, copied on the call's stream
    // before the workspace holding them is released to other callers
    std::vector<uint8_t> hh;
    if (hit && (host_timing() || stats_on())) {
      hh.resize(np);
      HCHK(hipMemcpyAsync(hh.data(), hit, np, hipMemcpyDeviceToHost, h.s));
    }
    if (ws_release(w, h.s)) return -1;
    lk.unlock();  // enqueued: other callers may enqueue while this one waits for its stream
    const double t_enq = now_ms();
    HCHK(hipMemcpyAsync(out + 96 * gb, dout, ng * 96, hipMemcpyDeviceToHost, h.s));
    HCHK(hipMemcpyAsync(status + gb, dst, ng, hipMemcpyDeviceToHost, h.s));
    HCHK(hipStreamSynchronize(h.s));
    size_t hits = 0;
    if (!hh.empty()) {
      for (uint8_t x : hh) hits += x;
      g_stats[6] += np;
      g_stats[7] += hits;
    }
    if (host_timing()) {
      fprintf(stderr, "hbls group_op mode=%d groups=%zu members=%zu cache=%d hits=%zu: lock wait %.2f ms, enqueue+upload "
              "%.2f, device %.2f\n", mode, ng, np, hit ? 1 : 0, hits, t_locked - t_start, t_enq - t_locked,
              now_ms() - t_enq);
    }
    return 0;
  });
}

// ---------------------------------------------------------------------------------------
// Coalescing of concurrent host calls (coalesce.h): the first caller of an idle queue becomes the
// leader, waits at most HBLS_COALESCE_US for more requests (or until HBLS_COALESCE_MAX items queue
// up), runs them as one batch and wakes every requester with its own statuses.  Requests that
// arrive while a batch runs form the next batch.
// ---------------------------------------------------------------------------------------
Coalescer g_vq;
CoalesceParams g_cp;
std::once_flag g_cp_once;

// read once, by the first caller, before any request is queued (std::call_once: concurrent first
// callers all see the three parameters set)
const CoalesceParams& coalesce_params() {
  std::call_once(g_cp_once, [] {
    g_cp.us = env_size("HBLS_COALESCE_US", 200);
    g_cp.max_items = env_size("HBLS_COALESCE_MAX", 1u << 16);
    // batches in flight at once (HBLS_COALESCE_INFLIGHT, default: the host-call contexts): the
    // requests that arrive while batches run form the next one, which starts at once instead of
    // behind them -- a small batch leaves most of the chip idle
    g_cp.inflight = std::max<size_t>(1, env_size("HBLS_COALESCE_INFLIGHT", (size_t)g_ws_sets));
  });
  return g_cp;
}

void run_verify_batch(std::vector<VReq*>& batch) {
  size_t tot = 0;
  for (VReq* r : batch) tot += r->n;
  std::vector<uint8_t> pk(48 * tot), sig(96 * tot), msg, st(tot);
  std::vector<uint64_t> off(tot);
  std::vector<uint32_t> len(tot);
  size_t k = 0;
  for (VReq* r : batch)
    for (size_t i = 0; i < r->n; i++, k++) {
      memcpy(&pk[48 * k], r->pk + 48 * i, 48);
      memcpy(&sig[96 * k], r->sig + 96 * i, 96);
      off[k] = msg.size();
      len[k] = r->len[i];
      msg.insert(msg.end(), r->msg + r->off[i], r->msg + r->off[i] + r->len[i]);
    }
  if (msg.empty()) msg.push_back(0);
  int rc = verify_host(pk.data(), sig.data(), msg.data(), off.data(), len.data(), tot, st.data());
  std::string err = rc ? g_err : std::string();
  k = 0;
  for (VReq* r : batch) {
    r->rc = rc;
    r->err = err;
    if (!rc) memcpy(r->st, &st[k], r->n);
    k += r->n;
  }
}

int verify_coalesced(const uint8_t* pks, const uint8_t* sigs, const uint8_t* msgs, const uint64_t* msg_off,
                     const uint32_t* msg_len, size_t n, uint8_t* status) {
  const CoalesceParams& p = coalesce_params();
  if (p.us == 0 || n >= p.max_items) return verify_host(pks, sigs, msgs, msg_off, msg_len, n, status);
  VReq me;
  me.pk = pks;
  me.sig = sigs;
  me.msg = msgs;
  me.off = msg_off;
  me.len = msg_len;
  me.n = n;
  me.st = status;
  coalesce_submit(g_vq, p, me, run_verify_batch);  // coalesce.h
  if (me.rc) g_err = me.err;
  return me.rc;
}

// ---------------------------------------------------------------------------------------
// VerifyAggregate (FastAggregateVerify, herumi.go:318-342) of n_groups groups whose public keys
// are pks[goff[g] .. goff[g+1]) (goff on the HOST, goff[0] == 0): every key decompressed in
// parallel (k_dec_pk), the keys of each group summed by a segmented tree reduction of segments of
// VA_SEG points (k_seg_sum; planned here from goff: a 7M-key group takes 5 launches), the sums
// paired with H(m_g) against the group's signature (k_pair3), herumi's checks applied in its
// order (k_va_status).  hm: one hashed message (with lines) per group, written by hash_fn (if
// given) on s while the side streams decompress: side 0 the keys and their reduction, side 1 the
// signatures and their lines.
// ---------------------------------------------------------------------------------------
constexpr uint32_t VA_SEG = 32;

// The reduction's plan: the segment boundaries of every pass (pass k: pass_n[k] segments from
// plan[pass_off[k]]), then the sum index of each group (0xffffffff: an empty group), then the identity map.
struct VaPlan {
  std::vector<uint32_t> plan;
  std::vector<size_t> pass_off, pass_n;
  size_t sog_off = 0, iota_off = 0;
};
void va_plan(const uint32_t* goff, size_t ng, size_t np, VaPlan& v) {
  std::vector<uint32_t>& plan = v.plan;
  std::vector<uint32_t> lo(ng), hi(ng);
  for (size_t g = 0; g < ng; g++) lo[g] = goff[g], hi[g] = goff[g + 1];
  bool more = np > 0;
  while (more) {
    v.pass_off.push_back(plan.size());
    plan.push_back(0);
    uint32_t out = 0;
    more = false;
    for (size_t g = 0; g < ng; g++) {
      if (hi[g] == lo[g]) continue;
      const uint32_t first = out;
      for (uint32_t b = lo[g]; b < hi[g]; b += VA_SEG) {
        plan.push_back(std::min<uint32_t>(b + VA_SEG, hi[g]));
        out++;
      }
      lo[g] = first;
      hi[g] = out;
      more |= out - first > 1;
    }
    v.pass_n.push_back(out);
  }
  v.sog_off = plan.size();
  for (size_t g = 0; g < ng; g++) plan.push_back(hi[g] > lo[g] ? lo[g] : 0xffffffffu);
  v.iota_off = plan.size();
  for (size_t g = 0; g < ng; g++) plan.push_back((uint32_t)g);
}

// The plan's passes on stream s0 over `in` (affine entries, or Jacobian partial sums: every pass is then
// k_seg_sum<false>) with their flags, alternating between (sa, sta) and (sb, stb); out / out_st: where the
// last pass left the groups' sums (sa / sta when the plan has no pass).
int va_reduce(Dev& d, const VaPlan& v, const uint32_t* dplan, bool affine, const void* in, const uint8_t* in_st, G1JEntry* sa,
              uint8_t* sta, G1JEntry* sb, uint8_t* stb, hipStream_t s0, G1JEntry** out, uint8_t** out_st) {
  *out = sa;
  *out_st = sta;
  for (size_t k = 0; k < v.pass_n.size(); k++) {
    *out = (k & 1) ? sb : sa;
    *out_st = (k & 1) ? stb : sta;
    TIMED(d, "k_seg_sum", s0,
          launch_seg_sum(affine && k == 0, in, in_st, dplan + v.pass_off[k], (uint32_t)v.pass_n[k], *out, *out_st, s0));
    in = *out;
    in_st = *out_st;
  }
  return 0;
}

// Where va_pipeline's np summands come from: compressed public keys (hbls_verify_aggregate_batch and the
// device entry: k_dec_pk, then an affine first pass), or Jacobian partial sums with their flags, already
// on the device (hbls_cluster_verify_aggregate: the shards' sums of the cluster's resident keys).
struct VaKeys {
  const uint8_t* dpk = nullptr;
  const G1JEntry* sums = nullptr;
  const uint8_t* sums_st = nullptr;
};

int va_pipeline(Dev& d, Ws& w, const VaKeys& keys, size_t np, const uint32_t* goff, size_t ng, const uint8_t* dsig,
                const MsgEntry* hm, uint8_t* dst, hipStream_t s, const std::function<int()>& hash_fn) {
  if (ng == 0) return 0;
  if (np > 0xffffffffull || ng > 0x7fffffffull) return set_err("verify aggregate: too many keys");
  VaPlan v;
  va_plan(goff, ng, np, v);
  const std::vector<uint32_t>& plan = v.plan;
  const std::vector<size_t>& pass_n = v.pass_n;
  const size_t sog_off = v.sog_off, iota_off = v.iota_off;
  uint32_t* dplan;  // in the workspace set (event-ordered), copied on the call's stream
  if (wsbuf(w, W_PLAN, plan.size(), &dplan)) return -1;
  HCHK(hipMemcpyAsync(dplan, plan.data(), plan.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));

  G1AEntry *pts = nullptr, *vapt;
  uint8_t *mst = nullptr, *sigst, *pv, *sta, *stb;
  HmEntry* sigpt;
  G1JEntry *sa, *sb;
  LineEntry* lines;
  const size_t na = pass_n.empty() ? 1 : pass_n[0], nb = pass_n.size() > 1 ? pass_n[1] : 1;
  if ((keys.dpk && (wsbuf(w, W_VPK, np, &pts) || wsbuf(w, W_VPKST, np, &mst))) || wsbuf(w, W_VSIG, ng, &sigpt) ||
      wsbuf(w, W_VSIGST, ng, &sigst) || wsbuf(w, W_FBLINES, ng * N_LINES, &lines) || wsbuf(w, W_SEGA, na, &sa) ||
      wsbuf(w, W_SEGSTA, na, &sta) || wsbuf(w, W_SEGB, nb, &sb) || wsbuf(w, W_SEGSTB, nb, &stb) ||
      wsbuf(w, W_VAPT, ng, &vapt) || wsbuf(w, W_VAPV, ng, &pv))
    return -1;
  hipStream_t s0 = w.side[0], s1 = w.side[1];
  HCHK(hipEventRecord(w.ev_fork, s));
  HCHK(hipStreamWaitEvent(s0, w.ev_fork, 0));
  HCHK(hipStreamWaitEvent(s1, w.ev_fork, 0));
  TIMED(d, "k_dec_sig_pt", s1, launch_dec_sig_pt(dsig, (uint32_t)ng, sigpt, sigst, s1));
  TIMED(d, "k_sig_lines", s1, launch_sig_lines(sigpt, (uint32_t)ng, lines, (uint32_t)ng, s1));
  HCHK(hipEventRecord(w.ev_side[1], s1));
  if (hash_fn && hash_fn()) return -1;
  if (keys.dpk && np) TIMED(d, "k_dec_pk", s0, launch_dec_pk(keys.dpk, (uint32_t)np, pts, mst, s0));
  G1JEntry* out;
  uint8_t* out_st;
  if (va_reduce(d, v, dplan, keys.dpk != nullptr, keys.dpk ? (const void*)pts : (const void*)keys.sums,
                keys.dpk ? mst : keys.sums_st, sa, sta, sb, stb, s0, &out, &out_st))
    return -1;
  HCHK(hipEventRecord(w.ev_side[0], s0));
  HCHK(hipStreamWaitEvent(s, w.ev_side[0], 0));
  HCHK(hipStreamWaitEvent(s, w.ev_side[1], 0));
  TIMED(d, "k_va_point", s, launch_va_point(out, dplan + sog_off, (uint32_t)ng, vapt, s));
  Pair3Args a{};
  a.pk = vapt;
  a.msg_idx = dplan + iota_off;
  a.hm = hm;
  a.sig_lines = lines;
  a.stride = (uint32_t)ng;
  a.n = (uint32_t)ng;
  a.n_items = (uint32_t)ng;
  a.status = pv;
  TIMED(d, "k_pair3", s, launch_pair3(a, s));
  TIMED(d, "k_va_status", s, launch_va_status(sigpt, sigst, out_st, dplan + sog_off, pv, (uint32_t)ng, dst, s));
  return 0;
}

// The selection-and-aggregation tail shared by slot_select_core (phases 2-4) and a duty shard's
// aggregation of its fired groups (DutyShardAdd::aggregate_fired_): sel_ws, the caller's own kernel that
// fills the groups' candidates (k_ta_select / k_duty_gather), sel_aggregate, sel_verify.  SelWs: sa's buffers
// (the rest of sa is the caller's), the aggregation's rows in class order, the aggregates for sel_verify
struct SelWs {
  TaSelectArgs sa{};
  uint8_t *pout = nullptr, *pst = nullptr, *ast = nullptr;
  HmEntry *ppt = nullptr, *apt = nullptr;
};

// ng groups of t members in workspace set w; enqueues the histogram's reset, the tail's first operation on s
int sel_ws(Ws& w, size_t ng, size_t t, hipStream_t s, SelWs& x) {
  TaSelectArgs& sa = x.sa;
  if (wsbuf(w, W_SELCIDX, ng * t, &sa.cidx) || wsbuf(w, W_SELKEY, ng, &sa.key) || wsbuf(w, W_SELSTATE, ng, &sa.state) ||
      wsbuf(w, W_SELGMSG, ng, &sa.gmsg) || wsbuf(w, W_SELHIST, 2 * (size_t)TASEL_KEYS, &sa.hist) ||
      wsbuf(w, W_SELOFF, (size_t)TASEL_KEYS + 1, &sa.off) || wsbuf(w, W_SELPERM, ng, &sa.perm) ||
      wsbuf(w, W_SELPMEM, ng * t, &sa.pmem) || wsbuf(w, W_SELPIDX, ng * t, &sa.pidx) ||
      wsbuf(w, W_SELPGOFF, ng + 1, &sa.pgoff) || wsbuf(w, W_SELPOUT, 96 * ng, &x.pout) || wsbuf(w, W_SELPST, ng, &x.pst) ||
      wsbuf(w, W_SELPPT, ng, &x.ppt) || wsbuf(w, W_SELAPT, ng, &x.apt) || wsbuf(w, W_SELAST, ng, &x.ast))
    return -1;
  sa.cur = sa.hist + TASEL_KEYS;
  sa.n_groups = (uint32_t)ng;
  sa.t = (uint32_t)t;
  HCHK(hipMemsetAsync(sa.hist, 0, 2 * (size_t)TASEL_KEYS * sizeof(uint32_t), s));
  return 0;
}

// The groups in class order, ThresholdAggregate over the chosen members of pts / pts_st (ta_tail on
// w, x's workspace set), the rows back in group order into ta_out / ta_status, counted into ctr
int sel_aggregate(Dev& d, Ws& w, SelWs& x, const HmEntry* pts, const uint8_t* pts_st, uint8_t* ta_out, uint8_t* ta_status,
                  uint64_t* ctr, hipStream_t s) {
  TaSelectArgs& sa = x.sa;
  const size_t ng = sa.n_groups, t = sa.t;
  TIMED(d, "k_ta_sel_scan", s, launch_scan(sa.hist, TASEL_KEYS, sa.off, s));
  TIMED(d, "k_ta_sel_fill", s, launch_ta_sel_fill(sa, s));
  const uint8_t* sdone = nullptr;
  if (ta_tail(d, w, pts, sa.pmem, pts_st, sa.pidx, sa.pgoff, ng, ng * t, 0, x.pout, x.pst, x.ppt, s, nullptr, nullptr, &sdone))
    return -1;
  TaScatterArgs sc{};
  sc.n_groups = (uint32_t)ng;
  sc.perm = sa.perm;
  sc.state = sa.state;
  sc.pout = x.pout;
  sc.pstatus = x.pst;
  sc.ppt = x.ppt;
  sc.sdone = sdone;
  sc.ta_out = ta_out;
  sc.ta_status = ta_status;
  sc.rows16 = (((uintptr_t)ta_out | (uintptr_t)x.pout) & 15) == 0 ? 1 : 0;
  sc.agg_pt = x.apt;
  sc.agg_st = x.ast;
  sc.ctr = ctr;
  TIMED(d, "k_ta_sel_scatter", s, launch_ta_sel_scatter(sc, s));
  return 0;
}

// The aggregates verified, one item per group: a second verify_pipeline on workspace set w, handed
// the affine aggregates in place of signature bytes (pre_sig); a group without an aggregate is an
// item with a bad signature status, which costs no pairing.  v2 comes with the caller's own fields (pks,
// hm, fold, defer_hm, defer_msgs).  Then the groups' verdicts
int sel_verify(Dev& d, Ws& w, const SelWs& x, VerifyCall& v2, const uint8_t* ta_status, uint8_t* agg_vstatus, hipStream_t s) {
  const size_t ng = x.sa.n_groups;
  v2.pre_sig = x.apt;
  v2.pre_sigst = x.ast;
  v2.msg_idx = x.sa.gmsg;
  v2.n = ng;
  v2.n_groups = ng;
  v2.status = agg_vstatus;
  v2.s = s;
  if (verify_pipeline(d, w, v2)) return -1;
  TIMED(d, "k_ta_sel_verdicts", s, launch_ta_sel_verdicts(ta_status, (uint32_t)ng, agg_vstatus, s));
  return 0;
}

// The core of hbls_slot_select_device and hbls_slot_select_batch: hbls_slot_device with
// verified-member selection, over device buffers (a: as the device entry takes it, checked by the
// caller, who holds d.mu) on stream s.  mode: how members are picked (tasel.h TASEL_MODE_*).
// behind_default: the device entry, whose caller may have prepared its buffers on the default stream;
// it takes the next workspace set for phase 4.  The host entry keeps phase 4 on the set of phases
// 1-3 (what HBLS_WS_SETS=1 does to the device entry): its calls come from several threads, one set
// each then holds a whole call, and no call enqueues onto streams still busy with another call's work
// (measured: that enqueue held the calling thread, and the device lock, until the other call ended).
// Four phases on the stream, each behind the one before (the aggregation needs the verdicts, the
// second verification the aggregates):
//   1. hash, and verify the partials without a fold (workspace set w: the decompressed partials stay)
//   2. select each group's members (threshold.hip k_ta_select) and put the groups in class order
//   3. ThresholdAggregate over the chosen members through src into the retained points
//      (sel_aggregate: the shared tail, with the class order of phase 2)
//   4. verify the aggregates under the DV keys on the next workspace set (sel_verify: the shared tail)
thread_local double g_core_marks[3];  // HBLS_HOST_TIMING: phase 1, phases 2-3 and phase 4 enqueued
int slot_select_core(Dev& d, hipStream_t s, const hbls_slot& a, uint32_t threshold, uint32_t* chosen,
                     uint32_t* ta_count, uint32_t mode, bool behind_default) {
  const size_t ng = a.n_groups, t = threshold;
  g_core_marks[0] = g_core_marks[1] = g_core_marks[2] = 0;
  Ws& w = ws_acquire(d, s);
  if (behind_default && s) {  // behind what the default stream holds now, as hbls_slot_device
    HCHK(hipEventRecord(w.ev_dflt, nullptr));
    HCHK(hipStreamWaitEvent(s, w.ev_dflt, 0));
  }
  // phase 1
  bool defer = false;
  if (a.n) {
    HCHK(hipEventRecord(w.ev_fork, s));
    hipStream_t sh = w.side[2];
    HCHK(hipStreamWaitEvent(sh, w.ev_fork, 0));
    defer = defer_lines(a.n_vgroups, a.n_msgs);
    if (hash_messages(d, a.msgs, a.msg_off, a.msg_len, a.n_msgs, (MsgEntry*)a.hm, sh, !defer)) return -1;
    HCHK(hipEventRecord(w.ev_side[2], sh));
  }
  TaFold tables{};
  tables.pk_table = (const G1AEntry*)a.pk_table;
  tables.pk_table_st = a.pk_table_st;
  VerifyCall vc;
  vc.pks = a.pks;
  vc.sigs = a.sigs;
  vc.msg_idx = a.msg_idx;
  vc.hm = (const MsgEntry*)a.hm;
  vc.n = a.n;
  vc.grp_off = a.vgrp_off;
  vc.n_groups = a.n_vgroups;
  vc.status = a.vstatus;
  vc.s = s;
  vc.device_entry = true;
  vc.hm_ready = w.ev_side[2];
  vc.fold = a.pk_table ? &tables : nullptr;
  vc.defer_hm = (MsgEntry*)a.hm;
  vc.defer_msgs = defer ? a.n_msgs : 0;
  if (a.n) {
    if (verify_pipeline(d, w, vc)) return -1;
    HCHK(hipStreamWaitEvent(s, w.ev_side[2], 0));
  }
  if (!ng) return ws_release(w, s);
  if (host_timing()) g_core_marks[0] = now_ms();
  // phase 2
  const bool first_use = d.sel_ctr.p == nullptr;
  uint64_t* ctr;
  if (ensure_buf(d.sel_ctr, SEL_COUNTERS * sizeof(uint64_t), (void**)&ctr)) return -1;
  if (first_use) {  // once per device, and complete before any stream's kernel counts
    HCHK(hipMemset(ctr, 0, SEL_COUNTERS * sizeof(uint64_t)));
    HCHK(hipStreamSynchronize(nullptr));
  }
  SelWs x;
  if (sel_ws(w, ng, t, s, x)) return -1;
  TaSelectArgs& sa = x.sa;
  sa.vstatus = a.vstatus;
  sa.msg_idx = a.msg_idx;
  sa.n = (uint32_t)a.n;
  sa.src = a.ta_src;
  sa.idx = a.ta_idx;
  sa.grp_off = a.grp_off;
  sa.n_cand = (uint32_t)a.n_ta_partials;
  sa.mode = mode;
  sa.chosen = chosen;
  sa.ta_count = ta_count;
  sa.ctr = ctr;
  TIMED(d, "k_ta_select", s, launch_ta_select(sa, s));
  if (!a.n) {  // no partial: no group has a member
    TaScatterArgs sc{};
    sc.n_groups = (uint32_t)ng;
    sc.state = sa.state;
    sc.ta_out = a.ta_out;
    sc.ta_status = a.ta_status;
    sc.ctr = ctr;
    TIMED(d, "k_ta_sel_scatter", s, launch_ta_sel_scatter(sc, s));
    TIMED(d, "k_ta_sel_verdicts", s, launch_ta_sel_verdicts(a.ta_status, (uint32_t)ng, a.agg_vstatus, s));
    return ws_release(w, s);
  }
  // phase 3, with the rest of phase 2
  if (sel_aggregate(d, w, x, vc.vsig, vc.vsigst, a.ta_out, a.ta_status, ctr, s)) return -1;
  if (host_timing()) g_core_marks[1] = now_ms();
  // phase 4.  The messages' lines: computed by phase 1 unless it deferred them; then this pass
  // defers them too where its plan can (the batched sizes), else they are computed first
  Ws& w2 = behind_default ? ws_acquire(d, s) : w;
  size_t defer2 = 0;
  if (defer) {
    if (vp_bfe(VerifyShape{ng, ng, 0, false, false, 0, d.n_cu, false},
               VerifyKnobs{g_gcap.load(), g_fbcap.load(), g_fe_batch_min.load(), g_slot_msm_min.load(),
                           g_rlc_lanes.load(), g_adaptive.load()}))
      defer2 = a.n_msgs;
    else
      TIMED(d, "k_lines_msg", s, launch_lines_msg((MsgEntry*)a.hm, (uint32_t)a.n_msgs, s));
  }
  TaFold tables2{};
  tables2.pk_table = (const G1AEntry*)a.dv_pk_table;
  tables2.pk_table_st = a.dv_pk_table_st;
  VerifyCall v2;
  v2.pks = a.dv_pks;
  v2.hm = (const MsgEntry*)a.hm;
  v2.fold = a.dv_pk_table ? &tables2 : nullptr;
  v2.defer_hm = (MsgEntry*)a.hm;
  v2.defer_msgs = defer2;
  if (sel_verify(d, w2, x, v2, a.ta_status, a.agg_vstatus, s)) return -1;
  if (host_timing()) g_core_marks[2] = now_ms();
  if (ws_release(w, s)) return -1;
  return &w2 == &w ? 0 : ws_release(w2, s);
}

// hbls_slot_select_batch: one duty from host buffers to aggregates (hslot.h is the plan).  The
// aggregation groups are sharded over the devices; each shard plans on the host without the device
// lock, uploads on its context's stream, runs slot_select_core under the matching rule, and waits
// for that stream only.  A shard that is the whole call uploads the caller's keys and signatures as
// they are, plans beside that transfer, and reorders them on the device (gather_items /
// scatter_status, as verify_host and verify_large); several shards copy their items on the host.
// Nothing is entered into the decompressed-signature cache: the aggregation reads the partials the
// verification left in its workspace.
int slot_select_host(const uint8_t* pks, const uint8_t* sigs, const uint8_t* msgs, const uint64_t* msg_off,
                     const uint32_t* msg_len, size_t n, const uint32_t* cand, const int64_t* cand_idx,
                     const uint32_t* grp_off, size_t n_groups, const uint8_t* dv_pks, uint32_t threshold,
                     uint8_t* vstatus, uint32_t* chosen, uint32_t* ta_count, uint8_t* ta_out, uint8_t* ta_status,
                     uint8_t* agg_vstatus) {
  const double t_start = now_ms();
  const size_t t = threshold;
  const size_t gmax = call_gmax(n, g_single_max.load(), g_fe_batch_min.load(), g_gmax.load());
  std::vector<uint8_t> listed;  // several shards: which partials some group lists
  if (slot_shards(devs().size(), n_groups) > 1) listed = slot_listed(cand + grp_off[0], grp_off[n_groups] - grp_off[0], n);
  return fan_out_k(n_groups, [&](Dev& d, size_t k, size_t nd, size_t gb, size_t ge) -> int {
    HcLease hcs(d);
    Hc& h = *hcs.h[0];
    if (nd > 1 && listed.size() != n) return set_err("hbls_slot_select_batch: the devices changed during the call");
    std::unique_lock<std::mutex> lk(d.mu, std::defer_lock);
    // a shard that is the whole call: the caller's keys and signatures go up as they are, the first
    // work on the context's stream, and the plan is made beside that transfer (as verify_large)
    uint8_t *rpk = nullptr, *rsig = nullptr;
    if (nd == 1) {
      lk.lock();
      if (hipSetDevice(d.ord) != hipSuccess) return set_err("hipSetDevice failed");
      if (upload(d, I_PK, pks, 48 * n, &rpk, &h) || upload(d, I_SIG, sigs, 96 * n, &rsig, &h)) return -1;
      lk.unlock();
    }
    SlotShard sh;
    const unsigned hw = std::thread::hardware_concurrency();
    slot_plan_shard(msgs, msg_off, msg_len, n, cand, grp_off, gb, ge, k, nd, listed, gmax,
                    nd == 1 && n >= (1u << 16) && hw >= 4 ? (hw >= 8 ? 8u : 4u) : 0u, sh);
    const size_t m = sh.m(), ng = ge - gb, nm = sh.tab.len.size(), nc = sh.cand.size();
    std::vector<uint8_t> hpk, hsig;
    if (!sh.whole) {  // the shard's keys and signatures in verification order
      hpk.resize(48 * m);
      hsig.resize(96 * m);
      for (size_t q = 0; q < m; q++) {
        memcpy(&hpk[48 * q], pks + 48ull * sh.order[q], 48);
        memcpy(&hsig[96 * q], sigs + 96ull * sh.order[q], 96);
      }
    }
    const double t_prep = now_ms();
    lk.lock();
    if (hipSetDevice(d.ord) != hipSuccess) return set_err("hipSetDevice failed");
    const double t_locked = now_ms();
    hbls_slot a{};
    uint8_t *dmsg, *dpk, *dsig, *ddv, *dst_out = nullptr;
    uint64_t* doff;
    uint32_t *dlen, *dmidx, *dvgoff, *dcand, *dgoff, *dord = nullptr;
    int64_t* dcidx;
    void *hm, *pst, *pchosen, *pcount, *pout, *ptst, *past;
    if (!sh.whole && (upload(d, I_PK, hpk.data(), hpk.size(), &dpk, &h) || upload(d, I_SIG, hsig.data(), hsig.size(), &dsig, &h)))
      return -1;
    // everything else through the context's pinned staging: a pageable copy queued behind the call's
    // kernels, or beside another call's, holds the calling thread (Hc::pin)
    PinnedUploads up;
    up.add(I_MSG, sh.tab.bytes.data(), sh.tab.bytes.size(), &dmsg);
    up.add(I_OFF, sh.tab.off.data(), nm, &doff);
    up.add(I_LEN, sh.tab.len.data(), nm, &dlen);
    if (sh.whole) up.add(I_IDX, sh.order.data(), m, &dord);
    up.add(I_MIDX, sh.vg.midx.data(), m, &dmidx);
    up.add(I_VGOFF, sh.vgoff.data(), sh.vgoff.size(), &dvgoff);
    up.add(I_CAND, sh.cand.data(), nc, &dcand);
    up.add(I_CIDX, ng ? cand_idx + grp_off[gb] : (const int64_t*)nullptr, nc, &dcidx);
    up.add(I_SGOFF, sh.goff.data(), sh.goff.size(), &dgoff);
    up.add(I_DVPK, ng ? dv_pks + 48 * gb : (const uint8_t*)nullptr, 48 * ng, &ddv);
    if (upload_pinned(d, h, up) || ensure_buf(h.io[I_HM], nm * sizeof(MsgEntry), &hm) || ensure_buf(h.io[I_STAT], m, &pst) ||
        ensure_buf(h.io[I_CHOSEN], ng * t * sizeof(uint32_t), &pchosen) ||
        ensure_buf(h.io[I_TACNT], ng * sizeof(uint32_t), &pcount) || ensure_buf(h.io[I_TAOUT], 96 * ng, &pout) ||
        ensure_buf(h.io[I_TAST], ng, &ptst) || ensure_buf(h.io[I_AGGST], ng, &past))
      return -1;
    if (sh.whole) {  // verification order on the device
      void *p1, *p2;
      if (ensure_buf(h.io[I_OUT], 144 * m, &p1) || ensure_buf(h.io[I_HM2], m, &p2)) return -1;
      dpk = (uint8_t*)p1;
      dsig = dpk + 48 * m;
      dst_out = (uint8_t*)p2;
      if (gather_items(rpk, rsig, dord, m, dpk, dsig, h.s)) return -1;
    }
    a.msgs = dmsg;
    a.msg_off = doff;
    a.msg_len = dlen;
    a.n_msgs = nm;
    a.hm = hm;
    a.pks = dpk;
    a.sigs = dsig;
    a.msg_idx = dmidx;
    a.n = m;
    a.vgrp_off = dvgoff;
    a.n_vgroups = sh.vg.n_groups();
    a.vstatus = (uint8_t*)pst;
    a.ta_src = dcand;
    a.ta_idx = dcidx;
    a.grp_off = dgoff;
    a.n_groups = ng;
    a.n_ta_partials = nc;
    a.ta_out = (uint8_t*)pout;
    a.ta_status = (uint8_t*)ptst;
    a.dv_pks = ddv;
    a.agg_vstatus = (uint8_t*)past;
    const double t_up = now_ms();
    if (slot_select_core(d, h.s, a, threshold, (uint32_t*)pchosen, (uint32_t*)pcount, TASEL_MODE_MATCHING, false)) return -1;
    if (sh.whole && scatter_status(a.vstatus, dord, m, dst_out, h.s)) return -1;
    lk.unlock();  // enqueued: other callers may enqueue while this one waits for its stream
    const double t_enq = now_ms();
    std::vector<uint8_t> hst;
    if (sh.whole) {
      if (m) HCHK(hipMemcpyAsync(vstatus, dst_out, m, hipMemcpyDeviceToHost, h.s));
    } else if (m) {
      hst.resize(m);
      HCHK(hipMemcpyAsync(hst.data(), a.vstatus, m, hipMemcpyDeviceToHost, h.s));
    }
    if (ng) {
      HCHK(hipMemcpyAsync(chosen + gb * t, pchosen, ng * t * sizeof(uint32_t), hipMemcpyDeviceToHost, h.s));
      HCHK(hipMemcpyAsync(ta_count + gb, pcount, ng * sizeof(uint32_t), hipMemcpyDeviceToHost, h.s));
      HCHK(hipMemcpyAsync(ta_out + 96 * gb, pout, 96 * ng, hipMemcpyDeviceToHost, h.s));
      HCHK(hipMemcpyAsync(ta_status + gb, ptst, ng, hipMemcpyDeviceToHost, h.s));
      HCHK(hipMemcpyAsync(agg_vstatus + gb, past, ng, hipMemcpyDeviceToHost, h.s));
    }
    HCHK(hipStreamSynchronize(h.s));
    for (size_t q = 0; q < hst.size(); q++) vstatus[sh.order[q]] = hst[q];
    slot_chosen_to_caller(sh, chosen + gb * t, ng * t);
    if (host_timing())
      fprintf(stderr, "hbls slot_select_host shard %zu/%zu n=%zu groups=%zu: plan %.2f ms, lock wait %.2f, enqueue+upload "
              "%.2f (uploads %.2f, verify %.2f, select+aggregate %.2f, aggregates' verify %.2f), device %.2f\n", k, nd, m, ng,
              t_prep - t_start, t_locked - t_prep, t_enq - t_locked, t_up - t_locked, g_core_marks[0] - t_up,
              g_core_marks[1] - g_core_marks[0], g_core_marks[2] - g_core_marks[1], now_ms() - t_enq);
    return 0;
  });
}

// ---------------------------------------------------------------------------------------
// Duty sessions (hbls_duty_open / _add / _state / _stats / _close; hduty.h is the host plan,
// dutysel.h the rule, duty.hip the kernels): hbls_slot_select_batch's pipeline under the arrival
// pattern of the reference node, one call per peer's set.  A duty keeps in device memory, per shard
// (a contiguous range of its groups on one device, the rule of hslot.h and fan_out): the hashed
// messages with their lines, and per group max_stored slots of decompressed partials with their
// share indices, message ids and serials, the count and the fired flag.
// ---------------------------------------------------------------------------------------
// Cluster handles (hbls_cluster_open / _close / _stats, hbls_duty_open_cluster; cluster.h is the rule,
// cluster.hip the kernels): the keys of a cluster lock -- per validator its DV key and its n_shares
// pubshares -- decompressed, subgroup-checked and (ladder_tables) given ladder tables once, resident per
// shard (the duty's rule: contiguous ranges of the validators over the devices as they were at open).
struct ClusterShard {
  Dev* d = nullptr;
  size_t gb = 0, ge = 0;
  G1AEntry* ent = nullptr;  // (ge - gb) (1 + n_shares) entries, row-major: cluster.h's key numbers
  uint8_t* st = nullptr;    // their statuses, as hbls_decompress_pubkeys_device reports them
  G1WidePt* wide = nullptr;  // ladder_tables: 15 points per key (written for the good, finite keys only)
  size_t n_keys = 0;
};
// INVARIANT: a cluster is immutable once hbls_cluster_open has returned.  Open writes the shards' buffers
// on the library stream of each device and synchronises before the handle exists; after that every
// kernel of every duty and call only reads them, so any number read them concurrently on any stream
// with no lock and no event.  Nothing frees them while a reader can exist: the memory goes with the
// last shared_ptr -- g_clusters' (hbls_cluster_close) or that of a duty opened on the cluster
// (hbls_duty_close, behind the duty's last call).  The counters are the only thing that changes.
struct Cluster {
  size_t n_validators = 0;
  uint32_t n_shares = 0;
  bool tables = false;
  std::vector<ClusterShard> sh;
  std::atomic<uint64_t> stats[6] = {};  // hbls_cluster_stats
  std::atomic<uint64_t> check_stats[2] = {};  // hbls_cluster_check_stats
  std::atomic<uint64_t> verify_stats[5] = {};  // hbls_cluster_verify_stats
  ~Cluster() {
    for (ClusterShard& s : sh) {
      if (!s.d) continue;
      std::lock_guard<std::mutex> lk(s.d->mu);
      if (hipSetDevice(s.d->ord) != hipSuccess) continue;
      DevBufs own({s.ent, s.st, s.wide});  // freed at the end of this round, under lk
    }
  }
};

// The open handles of one kind (duties, clusters): numbered from 1, a number never issued twice
template <class T>
struct HandleTable {
  std::mutex mu;
  std::unordered_map<uint64_t, std::shared_ptr<T>> map;
  uint64_t next = 1;
  uint64_t add(std::shared_ptr<T> p) {
    std::lock_guard<std::mutex> l(mu);
    map[next] = std::move(p);
    return next++;
  }
  std::shared_ptr<T> find(uint64_t handle, bool erase = false) {
    std::lock_guard<std::mutex> l(mu);
    auto it = map.find(handle);
    if (it == map.end()) return nullptr;
    std::shared_ptr<T> p = it->second;
    if (erase) map.erase(it);
    return p;
  }
  std::shared_ptr<T> take(uint64_t handle) { return find(handle, true); }  // found: no longer a handle
};
HandleTable<Cluster> g_clusters;

// take: hbls_cluster_close (the handle's last use)
std::shared_ptr<Cluster> cluster_get(const std::string& who, uint64_t handle, bool take = false) {
  std::shared_ptr<Cluster> cl = take ? g_clusters.take(handle) : g_clusters.find(handle);
  if (!cl) set_err(who + ": no such cluster (never opened, or closed)");
  return cl;
}

// The shard's keys for k_cluster_keys over items named by group and share index, device arrays (share_idx
// null: the groups' DV keys); any_entry: index 0 names the DV key (cluster.h cluster_key)
ClusterKeysArgs cluster_keys_args(const ClusterShard& cs, uint32_t n_shares, const uint32_t* group, const int64_t* share_idx,
                                  bool any_entry) {
  ClusterKeysArgs ck{};
  ck.group = group;
  ck.share_idx = share_idx;
  ck.group_base = (uint32_t)cs.gb;
  ck.n_groups = (uint32_t)(cs.ge - cs.gb);
  ck.n_shares = n_shares;
  ck.n_keys = (uint32_t)cs.n_keys;
  ck.any_entry = any_entry ? 1 : 0;
  ck.ent = cs.ent;
  ck.st = cs.st;
  return ck;
}

// A shard's items as its plan orders them, like everything the verification reads per item: their signatures
// and, where the keys are a cluster's (group non-null), the groups and key indices that name them
void gather_plan_order(const std::vector<uint32_t>& order, const uint32_t* group, const int64_t* key_idx, const uint8_t* sigs,
                       std::vector<uint32_t>& hcg, std::vector<int64_t>& hci, std::vector<uint8_t>& hsig) {
  const size_t m = order.size();
  hcg.resize(group ? m : 0);
  hci.resize(group ? m : 0);
  hsig.resize(96 * m);
  for (size_t q = 0; q < m; q++) {
    if (group) {
      hcg[q] = group[order[q]];
      hci[q] = key_idx[order[q]];
    }
    memcpy(&hsig[96 * q], sigs + 96ull * order[q], 96);
  }
}

// msgs may be null only where no item has a message of non-zero length
bool msgs_missing(const uint8_t* msgs, const uint32_t* msg_len, size_t n) {
  if (msgs) return false;
  for (size_t i = 0; i < n; i++)
    if (msg_len[i]) return true;
  return false;
}

// The stats calls of a handle read the first n of one of its N counters: the check of out and n, and the copy
// (a cluster's counters are atomic; a duty's are plain, copied under its lock)
int counters_args(const std::string& who, const uint64_t* out, size_t n, size_t N) {
  return !out || n > N ? set_err(who + ": out is null or n above " + std::to_string(N)) : 0;
}
template <class C>
void counters_copy(const C* stats, uint64_t* out, size_t n) {
  for (size_t k = 0; k < n; k++) out[k] = stats[k];
}

// hbls_cluster_stats, hbls_cluster_check_stats and hbls_cluster_verify_stats
template <size_t N>
int cluster_counters(const std::string& who, uint64_t cluster, std::atomic<uint64_t> (Cluster::*ctr)[N], uint64_t* out, size_t n) {
  if (ensure_init()) return -1;
  std::shared_ptr<Cluster> cl = cluster_get(who, cluster);
  if (!cl || counters_args(who, out, n, N)) return -1;
  counters_copy((*cl).*ctr, out, n);
  return 0;
}

// One shard of hbls_cluster_open: its rows' compressed keys up, the decompression and membership test of
// hbls_decompress_pubkeys_device into the resident table, the ladder tables, the statuses back; complete
// (synchronised) when it returns.  What it allocates for the cluster stays in s (on failure too: it goes
// with the cluster); its staging buffer goes when it returns, under the lock it holds.
int cluster_fill_shard(ClusterShard& s, const uint8_t* dv_pks, const uint8_t* pubshares, uint32_t n_shares, bool tables,
                       uint8_t* hst) {
  Dev& d = *s.d;
  const size_t ng = s.ge - s.gb, row = 1 + (size_t)n_shares, nk = ng * row;
  s.n_keys = nk;
  if (!nk) return 0;
  std::vector<uint8_t> keys(48 * nk);
  for (size_t g = 0; g < ng; g++) {
    memcpy(&keys[48 * g * row], dv_pks + 48 * (s.gb + g), 48);
    memcpy(&keys[48 * (g * row + 1)], pubshares + 48 * (s.gb + g) * n_shares, 48 * (size_t)n_shares);
  }
  std::lock_guard<std::mutex> lk(d.mu);
  if (hipSetDevice(d.ord) != hipSuccess) return set_err("hipSetDevice failed");
  DevBufs staging;
  uint8_t* tmp;
  HCHK(hipMalloc((void**)&s.ent, nk * sizeof(G1AEntry)));
  HCHK(hipMalloc((void**)&s.st, nk));
  if (tables) HCHK(hipMalloc((void**)&s.wide, nk * KEY_WIDE_PTS * sizeof(G1WidePt)));
  if (staging.alloc(&tmp, 48 * nk)) return -1;
  HCHK(hipMemcpyAsync(tmp, keys.data(), 48 * nk, hipMemcpyHostToDevice, d.stream));
  TIMED(d, "k_dec_pk", d.stream, launch_dec_pk(tmp, (uint32_t)nk, s.ent, s.st, d.stream));
  if (tables) TIMED(d, "k_cluster_wide", d.stream, launch_cluster_wide(s.ent, s.st, (uint32_t)nk, s.wide, d.stream));
  HCHK(hipMemcpyAsync(hst, s.st, nk, hipMemcpyDeviceToHost, d.stream));
  HCHK(hipStreamSynchronize(d.stream));  // complete before any stream's kernel reads them: the cluster is immutable from here
  return 0;
}

// A checked hbls_cluster_open: the shards one after the other, then the handle
int cluster_open(const uint8_t* dv_pks, const uint8_t* pubshares, size_t n_validators, uint32_t n_shares, bool tables,
                 uint8_t* key_status, uint64_t* handle) {
  auto cl = std::make_shared<Cluster>();  // (whatever a failing shard leaves allocated goes with it: nothing stays)
  cl->n_validators = n_validators;
  cl->n_shares = n_shares;
  cl->tables = tables;
  const std::vector<Dev*> ds = devs();
  const size_t nd = slot_shards(ds.size(), n_validators), row = 1 + (size_t)n_shares;
  cl->sh.resize(nd);
  std::vector<uint8_t> hst(n_validators * row);
  for (size_t k = 0; k < nd; k++) {
    ClusterShard& s = cl->sh[k];
    s.d = ds[k];
    s.gb = n_validators * k / nd;
    s.ge = n_validators * (k + 1) / nd;
    if (cluster_fill_shard(s, dv_pks, pubshares, n_shares, tables, hst.data() + s.gb * row))
      return shard_err("hbls_cluster_open", *s.d, g_err);
  }
  uint64_t bad = 0, built = 0;
  for (size_t g = 0; g < n_validators; g++)
    for (size_t j = 0; j < row; j++) {
      const uint8_t st = hst[g * row + j];
      const uint8_t* key = j ? pubshares + 48 * (g * n_shares + j - 1) : dv_pks + 48 * g;
      bad += st ? 1 : 0;
      built += (tables && !st && !(key[0] & 0x40)) ? 1 : 0;  // good and finite (the compressed form's infinity bit)
    }
  if (key_status && !hst.empty()) memcpy(key_status, hst.data(), hst.size());
  cl->stats[0] = hst.size();
  cl->stats[1] = bad;
  cl->stats[2] = built;
  *handle = g_clusters.add(cl);
  return 0;
}

// One shard of hbls_cluster_check: k_lock_check and k_lock_fold over the shard's own rows on its library
// stream, the rows' statuses and window masks into the caller's host arrays (the shard's part of them);
// complete (synchronised) when it returns.  The kernels only read the cluster.  What it allocates goes
// when it returns, whatever it returns.
int cluster_check_shard(const ClusterShard& s, const LockPlan& plan, uint8_t* hstatus, uint64_t* hwindows) {
  const size_t ng = s.ge - s.gb;
  if (!ng) return 0;
  Dev& d = *s.d;
  std::lock_guard<std::mutex> lk(d.mu);
  if (hipSetDevice(d.ord) != hipSuccess) return set_err("hipSetDevice failed");
  DevBufs b;
  uint8_t *win_st, *row_st;
  uint64_t* row_win;
  if (b.alloc(&win_st, ng * plan.windows) || b.alloc(&row_st, ng) || b.alloc(&row_win, ng * sizeof(uint64_t))) return -1;
  HCHK(hipMemsetAsync(row_win, 0, ng * sizeof(uint64_t), d.stream));  // a row with a bad-status key: no window
  TIMED(d, "k_lock_check", d.stream, launch_lock_check(s.ent, s.st, (uint32_t)ng, plan, win_st, row_st, row_win, d.stream));
  HCHK(hipMemcpyAsync(hstatus, row_st, ng, hipMemcpyDeviceToHost, d.stream));
  HCHK(hipMemcpyAsync(hwindows, row_win, ng * sizeof(uint64_t), hipMemcpyDeviceToHost, d.stream));
  HCHK(hipStreamSynchronize(d.stream));
  return 0;
}

// A checked hbls_cluster_check: the shards one after the other
int cluster_check(Cluster& cl, const LockPlan& plan, uint8_t* row_status, uint64_t* row_windows, size_t* n_bad) {
  // the shards' results gather here: the caller's arrays are written once every shard has succeeded
  std::vector<uint8_t> hst(cl.n_validators);
  std::vector<uint64_t> hwin(cl.n_validators);
  for (const ClusterShard& s : cl.sh)
    if (cluster_check_shard(s, plan, hst.data() + s.gb, hwin.data() + s.gb)) return shard_err("hbls_cluster_check", *s.d, g_err);
  uint64_t bad = 0, inconsistent = 0;
  for (uint8_t st : hst) {
    bad += st ? 1 : 0;
    inconsistent += st == ST_NOT_VERIFIED ? 1 : 0;
  }
  if (!hst.empty()) memcpy(row_status, hst.data(), hst.size());
  if (row_windows && !hwin.empty()) memcpy(row_windows, hwin.data(), hwin.size() * sizeof(uint64_t));
  if (n_bad) *n_bad = (size_t)bad;
  cl.check_stats[0] += 1;
  cl.check_stats[1] += inconsistent;
  return 0;
}

// What hbls_cluster_verify_batch was called with
struct ClusterVerifyArgs {
  const uint32_t* group;
  const int64_t* key_idx;
  const uint8_t *sigs, *msgs;
  const uint64_t* msg_off;
  const uint32_t* msg_len;
  size_t n;
  uint8_t* status;
};

// One shard of hbls_cluster_verify_batch: its items (caller indices, increasing), all of groups the shard
// owns.  Phase one of a cluster duty's add (DutyShardAdd::verify_) with a message table that lives for
// this call only: the plan (hduty.h duty_plan_shard), the upload, the hashing of the call's distinct
// messages, then verify_pipeline with the shard's keys by (group, key index), entry 0 allowed.  Not
// chunked, as a duty add is not.  The statuses go to hst at the items' caller indices; complete
// (synchronised) when it returns.  The kernels only read the cluster.
int cluster_verify_shard(const Cluster& cl, const ClusterShard& cs, const ClusterVerifyArgs& a, const std::vector<uint32_t>& items,
                         size_t gmax, uint8_t* hst) {
  const size_t m = items.size();
  if (!m) return 0;
  Dev& d = *cs.d;
  HcLease hcs(d);
  Hc& h = *hcs.h[0];
  DutyMsgTable tab;
  DutyShardPlan p;
  duty_plan_shard(a.msgs, a.msg_off, a.msg_len, a.group, a.key_idx, items, cs.gb, cs.ge, 0, gmax, tab, p);
  const size_t nm = tab.size();
  std::vector<uint8_t> hsig, st(m);
  std::vector<uint32_t> hcg;
  std::vector<int64_t> hci;
  gather_plan_order(p.order, a.group, a.key_idx, a.sigs, hcg, hci, hsig);
  std::unique_lock<std::mutex> lk(d.mu);
  if (hipSetDevice(d.ord) != hipSuccess) return set_err("hipSetDevice failed");
  hipStream_t s = h.s;
  uint8_t *dsig, *dmsg;
  uint64_t* doff;
  uint32_t *dlen, *dmidx, *dvgoff, *dcg;
  int64_t* dci;
  void *pst, *phm;
  if (upload(d, I_SIG, hsig.data(), hsig.size(), &dsig, &h)) return -1;
  PinnedUploads up;
  up.add(I_DCGRP, hcg.data(), m, &dcg);
  up.add(I_DCSHARE, hci.data(), m, &dci);
  up.add(I_MSG, tab.t.bytes.data(), tab.t.bytes.size(), &dmsg);
  up.add(I_OFF, tab.t.off.data(), nm, &doff);
  up.add(I_LEN, tab.t.len.data(), nm, &dlen);
  up.add(I_MIDX, p.midx.data(), m, &dmidx);
  up.add(I_VGOFF, p.vgoff.data(), p.vgoff.size(), &dvgoff);
  if (upload_pinned(d, h, up) || ensure_buf(h.io[I_STAT], m, &pst) || ensure_buf(h.io[I_HM], nm * sizeof(MsgEntry), &phm))
    return -1;
  MsgEntry* hm = (MsgEntry*)phm;
  Ws& w = ws_acquire(d, s);
  // the table is the call's own, so its lines are deferred where a host Verify defers them (verify_host)
  const bool defer = defer_lines(p.n_vgroups(), nm);
  if (hash_range(d, w, s, dmsg, doff, dlen, hm, 0, nm, !defer)) return -1;
  VerifyCall vc;
  vc.h_ready = w.ev_h;
  vc.defer_hm = hm;
  vc.defer_msgs = defer ? nm : 0;
  vc.sigs = dsig;
  vc.msg_idx = dmidx;
  vc.hm = hm;
  vc.n = m;
  vc.grp_off = dvgoff;
  vc.n_groups = p.n_vgroups();
  vc.status = (uint8_t*)pst;
  vc.s = s;
  vc.device_entry = true;
  vc.hm_ready = w.ev_side[2];
  const ClusterKeysArgs ck = cluster_keys_args(cs, cl.n_shares, dcg, dci, true);
  vc.cluster = &ck;
  vc.cluster_wide = cs.wide;
  if (verify_pipeline(d, w, vc)) return -1;
  HCHK(hipStreamWaitEvent(s, w.ev_side[2], 0));
  if (ws_release(w, s)) return -1;
  lk.unlock();  // enqueued: other callers may enqueue while this one waits for its stream
  HCHK(hipMemcpyAsync(st.data(), pst, m, hipMemcpyDeviceToHost, s));
  HCHK(hipStreamSynchronize(s));
  for (size_t q = 0; q < m; q++) hst[p.order[q]] = st[q];
  return 0;
}

// A checked hbls_cluster_verify_batch over the cluster's shards
int cluster_verify_batch(Cluster& cl, const ClusterVerifyArgs& a) {
  // an item goes to the shard that owns its group; one that names no validator needs no device
  const size_t n = a.n, nd = cl.sh.size();
  std::vector<std::vector<uint32_t>> items(nd);
  std::vector<uint8_t> hst(n, (uint8_t)ST_BAD_PUBKEY);
  uint64_t named = 0;
  for (size_t i = 0; i < n; i++) {
    if (a.group[i] >= cl.n_validators) continue;
    const size_t k = duty_shard_of_group(a.group[i], cl.n_validators, nd);
    items[k].push_back((uint32_t)i);
    const ClusterShard& s = cl.sh[k];
    named += cluster_key(a.group[i], a.key_idx[i], (uint32_t)s.gb, (uint32_t)(s.ge - s.gb), cl.n_shares, true) != CLUSTER_NO_KEY;
  }
  const size_t gmax = call_gmax(n, g_single_max.load(), g_fe_batch_min.load(), g_gmax.load());
  if (n && each_shard("hbls_cluster_verify_batch", cl.sh,
                      [&](size_t k) { return cluster_verify_shard(cl, cl.sh[k], a, items[k], gmax, hst.data()); }))
    return -1;
  // the caller's array is written once every shard has succeeded; a failed call counts nothing
  if (n) memcpy(a.status, hst.data(), n);
  cl.verify_stats[0] += 1;
  cl.verify_stats[1] += named;
  cl.verify_stats[2] += n - named;
  return 0;
}

// One shard of hbls_cluster_verify_aggregate, on its library stream: k_cluster_row_sum over the shard's
// own rows, then the k_seg_sum<false> passes of one group down to one Jacobian point and one flag, which
// come to the host (sum: 144 bytes); complete (synchronised) when it returns.  The kernels only read the
// cluster.  What it allocates goes when it returns, whatever it returns.
int cluster_sum_shard(const Cluster& cl, const ClusterShard& s, uint64_t share_mask, uint32_t with_dv, G1JEntry* sum,
                      uint8_t* flag) {
  const size_t ng = s.ge - s.gb;
  if (!ng) return 0;
  Dev& d = *s.d;
  const uint32_t goff[2] = {0, (uint32_t)ng};
  VaPlan v;
  va_plan(goff, 1, ng, v);
  const size_t na = v.pass_n[0], nb = v.pass_n.size() > 1 ? v.pass_n[1] : 1;
  std::lock_guard<std::mutex> lk(d.mu);
  if (hipSetDevice(d.ord) != hipSuccess) return set_err("hipSetDevice failed");
  DevBufs b;
  G1JEntry *rows, *sa, *sb;
  uint8_t *rows_st, *sa_st, *sb_st;
  uint32_t* dplan;
  if (b.alloc(&rows, ng * sizeof(G1JEntry)) || b.alloc(&rows_st, ng) || b.alloc(&sa, na * sizeof(G1JEntry)) ||
      b.alloc(&sa_st, na) || b.alloc(&sb, nb * sizeof(G1JEntry)) || b.alloc(&sb_st, nb) ||
      b.alloc(&dplan, v.plan.size() * sizeof(uint32_t)))
    return -1;
  HCHK(hipMemcpyAsync(dplan, v.plan.data(), v.plan.size() * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
  TIMED(d, "k_cluster_row_sum", d.stream,
        launch_cluster_row_sum(s.ent, s.st, (uint32_t)ng, cl.n_shares, share_mask, with_dv, rows, rows_st, d.stream));
  G1JEntry* out;
  uint8_t* out_st;
  if (va_reduce(d, v, dplan, false, rows, rows_st, sa, sa_st, sb, sb_st, d.stream, &out, &out_st)) return -1;
  HCHK(hipMemcpyAsync(sum, out, sizeof(G1JEntry), hipMemcpyDeviceToHost, d.stream));  // the one group's sum: index 0
  HCHK(hipMemcpyAsync(flag, out_st, 1, hipMemcpyDeviceToHost, d.stream));
  HCHK(hipStreamSynchronize(d.stream));
  return 0;
}

// A checked hbls_cluster_verify_aggregate: the shards' sums, then the cross-shard tail
int cluster_verify_aggregate(Cluster& cl, uint64_t share_mask, uint32_t with_dv, const uint8_t* sig, const uint8_t* msg,
                             uint32_t msg_len, uint8_t* status) {
  // per shard: its rows' selected keys down to one point and one flag (an empty selection sums nothing)
  const size_t nd = cl.sh.size();
  const uint32_t per_row = cluster_sel_count(share_mask, with_dv);
  std::vector<G1JEntry> hsum(nd);
  std::vector<uint8_t> hflag(nd, 0);
  if (per_row && each_shard("hbls_cluster_verify_aggregate", cl.sh, [&](size_t k) {
        return cluster_sum_shard(cl, cl.sh[k], share_mask, with_dv, &hsum[k], &hflag[k]);
      }))
    return -1;
  // across the shards: their points and flags, packed, to the first non-empty shard's device -- one more
  // k_seg_sum<false> pass there (va_pipeline over Jacobian sums), then FastAggregateVerify's tail
  std::vector<G1JEntry> sums;
  std::vector<uint8_t> flags;
  const ClusterShard* first = nullptr;
  for (size_t k = 0; k < nd; k++) {
    const ClusterShard& s = cl.sh[k];
    if (s.ge == s.gb) continue;
    if (!first) first = &s;
    if (per_row) {
      sums.push_back(hsum[k]);
      flags.push_back(hflag[k]);
    }
  }
  if (!first) first = &cl.sh[0];  // a cluster of no validator: the empty group on the first device
  Dev& d = *first->d;
  const size_t np = sums.size();
  const uint32_t goff[2] = {0, (uint32_t)np};
  MsgTable t;
  t.idx.resize(1);
  t.off.push_back(0);
  t.len.push_back(msg_len);
  t.bytes.assign(msg, msg + msg_len);
  uint8_t st = 0;
  {
    HcLease hcs(d);
    Hc& h = *hcs.h[0];
    std::unique_lock<std::mutex> lk(d.mu);
    if (hipSetDevice(d.ord) != hipSuccess) return set_err("hipSetDevice failed");
    G1JEntry* dsums;
    uint8_t *dflags, *dsig;
    void *pst, *hmp;
    if (upload(d, I_OUT, sums.data(), np, &dsums, &h) || upload(d, I_HM2, flags.data(), np, &dflags, &h) ||
        upload(d, I_SIG, sig, (size_t)96, &dsig, &h) || ensure_buf(h.io[I_STAT], 1, &pst) ||
        ensure_buf(h.io[I_HM], sizeof(MsgEntry), &hmp))
      return -1;
    Ws& w = ws_acquire(d, h.s);
    VaKeys keys;
    keys.sums = dsums;
    keys.sums_st = dflags;
    if (va_pipeline(d, w, keys, np, goff, 1, dsig, (MsgEntry*)hmp, (uint8_t*)pst, h.s,
                    [&]() -> int { MsgEntry* hx; return hash_table(d, t, &hx, true, &h); }))
      return -1;
    if (ws_release(w, h.s)) return -1;
    lk.unlock();  // enqueued: other callers may enqueue while this one waits for its stream
    HCHK(hipMemcpyAsync(&st, pst, 1, hipMemcpyDeviceToHost, h.s));
    HCHK(hipStreamSynchronize(h.s));
  }
  *status = st;
  cl.verify_stats[3] += 1;
  cl.verify_stats[4] += (uint64_t)per_row * cl.n_validators;
  return 0;
}

struct DutyShard {
  Dev* d = nullptr;
  size_t gb = 0, ge = 0;
  const ClusterShard* cs = nullptr;  // a cluster duty: the shard's keys (Duty::cl keeps them alive)
  DutyMsgTable tab;   // the shard's messages (host); ids index hm
  size_t hashed = 0;  // messages resident in hm (a failed add may leave the table ahead of it)
  MsgEntry* hm = nullptr;
  size_t hm_cap = 0;
  HmEntry* store = nullptr;     // (ge - gb) max_stored points
  uint8_t* store_st = nullptr;  // their member statuses: zero, a stored partial was verified
  int64_t* rec_idx = nullptr;
  uint32_t *rec_msg = nullptr, *rec_serial = nullptr, *count = nullptr;
  uint8_t *fired = nullptr, *dvpk = nullptr;
  uint64_t* selctr = nullptr;  // what k_ta_sel_scatter counts (the device's own counters stay hbls_slot_select's)
};
// INVARIANT: no two streams ever touch a duty's device buffers.  Every call on a duty holds `mu`
// from before its first enqueue until its stream (a host-call context's, with the workspace side
// streams joined into it) has drained; the next call, on whatever stream, is ordered behind it by
// that host-side wait alone.  Nothing else in the library knows these buffers.
// INVARIANT (hbls_duty_add_sets): what the host plan hands a kernel is never trusted as an address.
// set_off is validated on the host before anything is enqueued, and k_duty_set_first and the gate
// (dutysel.h duty_admit) still check an item's set id against n_sets before it indexes set_first,
// as k_duty_store checks a touched group against the shard's groups.  hbls_duty_add_sets_first hands the
// verification the groups' and items' set ids as well (VerifyCall::gseg / item_seg): dutyfirst.hip's kernels
// check each against n_seg in the same way.
// INVARIANT (cluster duties): a group or a share index of the caller's never becomes an address into
// the cluster's keys except through cluster.h cluster_key -- in k_cluster_keys for every partial and
// for every fired group's DV key, and on the host where hbls_cluster_stats is counted -- which compares
// the full 64-bit share index and the group against the shard's own range; k_cluster_keys checks the
// key's number against the shard's key count once more.
struct Duty {
  std::mutex mu;
  std::shared_ptr<Cluster> cl;  // a cluster duty (hbls_duty_open_cluster): its keys; the shards are the cluster's
  bool closed = false, broken = false;
  size_t n_groups = 0;
  uint32_t t = 0, max_stored = 0, next_serial = 0;
  std::vector<DutyShard> sh;
  uint64_t stats[6] = {};
  uint64_t set_stats[3] = {};  // hbls_duty_set_stats: sets seen, sets rejected, verified partials of rejected sets
  uint64_t first_stats[2] = {};  // hbls_duty_first_stats: partials through hbls_duty_add_sets_first, those reported UNCHECKED
};
HandleTable<Duty> g_duties;

// take: hbls_duty_close (the handle's last use)
std::shared_ptr<Duty> duty_get(const std::string& who, uint64_t handle, bool take = false) {
  std::shared_ptr<Duty> du = take ? g_duties.take(handle) : g_duties.find(handle);
  if (!du) set_err(who + ": no such duty (never opened, or closed)");
  return du;
}

void duty_free_shard(DutyShard& s) {
  if (!s.d) return;
  std::lock_guard<std::mutex> lk(s.d->mu);
  if (hipSetDevice(s.d->ord) != hipSuccess) return;
  DevBufs own({s.hm, s.store, s.store_st, s.rec_idx, s.rec_msg, s.rec_serial, s.count, s.fired, s.dvpk, s.selctr});  // freed on return
  s = DutyShard{};
}

int duty_alloc_shard(DutyShard& s, const uint8_t* dv_pks, uint32_t max_stored) {
  Dev& d = *s.d;
  std::lock_guard<std::mutex> lk(d.mu);
  if (hipSetDevice(d.ord) != hipSuccess) return set_err("hipSetDevice failed");
  const size_t ng = s.ge - s.gb, slots = std::max<size_t>(ng * max_stored, 1), g1 = std::max<size_t>(ng, 1);
  HCHK(hipMalloc((void**)&s.store, slots * sizeof(HmEntry)));
  HCHK(hipMalloc((void**)&s.store_st, slots));
  HCHK(hipMalloc((void**)&s.rec_idx, slots * sizeof(int64_t)));
  HCHK(hipMalloc((void**)&s.rec_msg, slots * sizeof(uint32_t)));
  HCHK(hipMalloc((void**)&s.rec_serial, slots * sizeof(uint32_t)));
  HCHK(hipMalloc((void**)&s.count, g1 * sizeof(uint32_t)));
  HCHK(hipMalloc((void**)&s.fired, g1));
  if (dv_pks || !ng) HCHK(hipMalloc((void**)&s.dvpk, 48 * g1));  // (a cluster duty keeps none: the DV keys are the cluster's)
  HCHK(hipMalloc((void**)&s.selctr, SEL_COUNTERS * sizeof(uint64_t)));
  HCHK(hipMemset(s.store_st, 0, slots));
  HCHK(hipMemset(s.count, 0, g1 * sizeof(uint32_t)));
  HCHK(hipMemset(s.fired, 0, g1));
  HCHK(hipMemset(s.selctr, 0, SEL_COUNTERS * sizeof(uint64_t)));
  if (ng && dv_pks) HCHK(hipMemcpy(s.dvpk, dv_pks + 48 * s.gb, 48 * ng, hipMemcpyHostToDevice));
  HCHK(hipStreamSynchronize(nullptr));  // complete before any stream's kernel reads them
  return 0;
}

// cl (nullable): a cluster duty -- no dv_pks, and the cluster's shards (devices and ranges as they were
// when it was opened) in place of devs() as it is now
int duty_open(const uint8_t* dv_pks, size_t n_groups, uint32_t threshold, uint32_t max_stored, uint64_t* handle,
              const std::shared_ptr<Cluster>& cl = nullptr) {
  const std::string who = cl ? "hbls_duty_open_cluster" : "hbls_duty_open";
  auto du = std::make_shared<Duty>();
  du->n_groups = n_groups;
  du->t = threshold;
  du->max_stored = max_stored;
  du->cl = cl;
  const std::vector<Dev*> ds = cl ? std::vector<Dev*>() : devs();
  const size_t nd = cl ? cl->sh.size() : slot_shards(ds.size(), n_groups);
  du->sh.resize(nd);
  for (size_t k = 0; k < nd; k++) {
    du->sh[k].d = cl ? cl->sh[k].d : ds[k];
    du->sh[k].gb = cl ? cl->sh[k].gb : n_groups * k / nd;
    du->sh[k].ge = cl ? cl->sh[k].ge : n_groups * (k + 1) / nd;
    du->sh[k].cs = cl ? &cl->sh[k] : nullptr;
    if (duty_alloc_shard(du->sh[k], dv_pks, max_stored)) {
      const Dev& d = *du->sh[k].d;
      const std::string err = g_err;
      for (size_t j = 0; j <= k; j++) duty_free_shard(du->sh[j]);  // nothing is left behind
      return shard_err(who, d, err);
    }
  }
  *handle = g_duties.add(du);
  return 0;
}

// What one shard's add hands back: its fired groups, ascending, with their rows
struct DutyShardOut {
  std::vector<uint32_t> fired, chosen;
  std::vector<uint8_t> ta_out, ta_status, agg_vstatus;
  uint64_t n_stored = 0, n_full = 0, n_new_msgs = 0, resident = 0;
  uint64_t n_named = 0, n_nokey = 0, n_dv = 0;  // a cluster duty: hbls_cluster_stats [3], [4], [5] of this add
};

// hbls_duty_add_sets: the call's sets (hduty.h), every caller index's set id
struct DutySetCall {
  const uint32_t* set_off = nullptr;
  size_t n_sets = 0;
  std::vector<uint32_t> set_of;
  // hbls_duty_add_sets_first: the shards plan set-major (hduty.h group_by_set) and verify segmented
  // (VerifyCall::gseg), which leaves set_first where k_duty_set_first would; the gate and the store are the same
  bool first = false;
};

// What a duty add was called with (include/hipbls.h), checked by duty_add_entry
struct DutyAddArgs {
  const uint8_t *pks, *sigs, *msgs;
  const uint64_t* msg_off;
  const uint32_t *msg_len, *group;
  const int64_t* share_idx;
  size_t n;
  uint8_t *vstatus, *stored;
  uint32_t *first_serial, *fired;
  size_t* n_fired;
  uint32_t* chosen;
  uint8_t *ta_out, *ta_status, *agg_vstatus;
  const char* who;
  const DutySetCall* sets;  // the set entry points (null: hbls_duty_add): the call's sets,
  uint32_t* set_first;      // and their first failures (n_sets entries) to fill
};

// One shard's part of an add: its items (caller indices, increasing).  As with
// hbls_slot_select_batch, the shard's add is one verification: it is not chunked.
//
// verify() enqueues the upload, the hashing and the verification; store() runs gate_(), store_rule_()
// (with the copies), download_() (the one host wait) and, where a group fired, aggregate_fired_() (the
// tail shared with slot_select_core) and download_fired_().  hbls_duty_add runs the two back to back
// as one stream segment under one hold of the device lock.  hbls_duty_add_sets does the same on one
// shard, with k_duty_set_first and k_duty_gate between the verification and the store;
// hbls_duty_add_sets_first likewise, except that the verification itself, run segmented over a
// set-major plan, leaves each set's first failure where k_duty_set_first would (DutySetCall::first).
// On several shards a set's verdict needs every shard's verification, so verify(split)
// ends phase one: it hands its workspace set back, waits for the shard's set_first and returns
// with no device lock held, the caller joins the shards and merges, and store(merged) is phase two.
// INVARIANT (host-call contexts): a context is one of a bounded pool per device that other calls
// block on (hc_acquire), so no call may wait for a second context while it holds one unless every
// such call takes them in one global order.  On the one-segment path a shard takes its context in
// verify() and gives it back at the end of store(), with no other shard waited for in between --
// the lifetime the shard routine always had.  On the two-phase path the contexts are held across
// the join (phase two needs the staging buffers phase one filled), so duty_add takes all of them
// itself before any shard starts, in ascending order of their devices' addresses (lease()), and each
// goes back at the end of its shard's store(): calls that hold a device's context wait only for
// devices later in that order, and one-context holders wait for nothing.
// INVARIANT (workspace sets): none is kept between the phases.  A set cannot be kept without the
// device lock (ws_acquire hands the sets out round-robin and orders their users by free_ev alone),
// so what phase two reads of the verification -- the decompressed signatures k_duty_copy moves -- is
// copied into the context's staging before the set is handed back.
// Members: "the call" is set by duty_add (the constructor); the rest is written by verify_() and the
// steps of store_() and read by the steps behind them.  `lk` is held from the first upload of a phase
// to its last enqueue only -- taken by verify_(), gate_() (phase two) and aggregate_fired_(), dropped by
// verify_() (phase one), store_rule_() and aggregate_fired_() -- and never when verify() / store()
// return; `w` is non-null from the verification's ws_acquire until the ws_release at the end of phase
// one (two phases: verify_()) or of the store's enqueues (one segment: store_rule_()), and stays
// unreleased, as it always did, when an enqueue fails in between; `hcs` is held from lease() or
// verify() until store() returns (or verify() fails); the device pointers are valid while it is.
struct DutyShardAdd {
  // the call
  Duty& du;
  DutyShard& sh;
  Dev& d;
  const DutyAddArgs& a;
  const DutySetCall* const sets;  // null: hbls_duty_add
  const size_t n_sets, t, ng, gmax;
  const std::vector<uint32_t>& items;
  const uint32_t first_serial;
  DutyShardOut& out;
  DutyShardAdd(Duty& du, DutyShard& sh, const DutyAddArgs& a, const std::vector<uint32_t>& items, size_t gmax, DutyShardOut& out)
      : du(du), sh(sh), d(*sh.d), a(a), sets(a.sets), n_sets(sets ? sets->n_sets : 0), t(du.t), ng(sh.ge - sh.gb),
        gmax(gmax), items(items), first_serial(du.next_serial), out(out) {}
  // from verify() to store(), and from step to step of it
  std::unique_ptr<HcLease> hcs;
  DutyShardPlan p;
  std::unique_lock<std::mutex> lk;
  bool split = false;
  size_t m = 0, nm = 0, nnew = 0, nt = 0, np = 0, nf = 0;
  double t_start = 0, t_prep = 0, t_enq1 = 0, t_dev1 = 0, t_enq2 = 0;
  uint32_t *dmidx = nullptr, *dserial = nullptr, *dtgrp = nullptr, *dtoff = nullptr, *dtpos = nullptr, *dsid = nullptr;
  int64_t* dtidx = nullptr;
  void *pst = nullptr, *pstored = nullptr, *pslot = nullptr, *pmslot = nullptr, *pmser = nullptr, *pmidx = nullptr,
       *pfmsg = nullptr, *pfkey = nullptr, *pcopy = nullptr, *pfired = nullptr, *pctr = nullptr, *psetfirst = nullptr,
       *padmit = nullptr;
  void *pser = nullptr, *pfg = nullptr, *ptout = nullptr, *ptst = nullptr, *past = nullptr;  // the fired groups' rows
  const HmEntry* vsig = nullptr;
  DutyStoreArgs st{};             // the storing rule's arguments: the gather reads its per-group outputs
  std::vector<uint32_t> hfired;   // the touched groups that fired (rows of the plan), downloaded
  Ws* w = nullptr;  // the verification's workspace set, until it is handed back
  std::vector<uint32_t> set_first;  // the sets' first failures as this shard saw them (one shard: the call's)

  int verify_(bool split);
  int store_(const uint32_t* merged);
  int gate_(const uint32_t* merged), store_rule_(), download_(), aggregate_fired_(), download_fired_();  // its steps
  // the device lock never outlives the phase (nor, in a shard thread, the thread) that took it
  int verify(bool two_phases) {
    const int rc = verify_(two_phases);
    if ((rc || two_phases) && lk.owns_lock()) lk.unlock();
    if (rc) hcs.reset();
    return rc;
  }
  int store(const uint32_t* merged) {
    const int rc = store_(merged);
    if (lk.owns_lock()) lk.unlock();
    hcs.reset();  // the last download is synchronised (or the shard failed): the context goes back now
    return rc;
  }
  // two phases: the shard's context, taken by duty_add in the global order before any shard starts
  void lease() {
    if (!items.empty()) hcs.reset(new HcLease(d));
  }
};

int DutyShardAdd::verify_(bool two_phases) {
  split = two_phases;
  m = items.size();
  if (sets) set_first.assign(sets->n_sets, DUTY_NONE);
  if (!m) return 0;
  t_start = now_ms();
  if (!hcs) hcs.reset(new HcLease(d));
  Hc& h = *hcs->h[0];
  const bool seg = sets && sets->first;
  duty_plan_shard(a.msgs, a.msg_off, a.msg_len, a.group, a.share_idx, items, sh.gb, sh.ge, first_serial, gmax, sh.tab, p,
                  seg ? sets->set_of.data() : nullptr);
  std::vector<uint32_t> hsid;
  if (sets) duty_plan_sets(sets->set_of, p, hsid);
  nm = sh.tab.size(), nnew = nm - sh.hashed, nt = p.n_touched(), np = p.tpos.size();
  out.n_new_msgs = nnew;
  out.resident = p.resident;
  // the keys: the caller's 48 bytes per partial, or (a cluster duty) each partial's group and share index
  // for k_cluster_keys -- as the plan orders them, like everything the verification reads per item
  const ClusterShard* const cs = sh.cs;
  std::vector<uint8_t> hpk(cs ? 0 : 48 * m), hsig;
  std::vector<uint32_t> hcg;
  std::vector<int64_t> hci;
  gather_plan_order(p.order, cs ? a.group : nullptr, a.share_idx, a.sigs, hcg, hci, hsig);
  if (!cs) {
    for (size_t q = 0; q < m; q++) memcpy(&hpk[48 * q], a.pks + 48ull * p.order[q], 48);
  } else {  // hbls_cluster_stats: the rule the kernel applies, on the host; duty_add counts it once the add has succeeded
    for (size_t q = 0; q < m; q++)
      out.n_named += cluster_key(hcg[q], hci[q], (uint32_t)sh.gb, (uint32_t)ng, du.cl->n_shares) != CLUSTER_NO_KEY ? 1 : 0;
    out.n_nokey = m - out.n_named;
  }
  std::vector<uint64_t> noff(nnew);  // the new messages' offsets, from the first new byte
  const uint64_t nb0 = nnew ? sh.tab.t.off[sh.hashed] : 0;
  for (size_t j = 0; j < nnew; j++) noff[j] = sh.tab.t.off[sh.hashed + j] - nb0;
  t_prep = now_ms();
  lk = std::unique_lock<std::mutex>(d.mu);
  if (hipSetDevice(d.ord) != hipSuccess) return set_err("hipSetDevice failed");
  hipStream_t s = h.s;
  if (nm > sh.hm_cap) {  // grow geometrically, keeping the resident entries (hash and lines)
    const size_t cap = std::max<size_t>(std::max<size_t>(nm, 2 * sh.hm_cap), 16);
    MsgEntry* nh;
    HCHK(hipMalloc((void**)&nh, cap * sizeof(MsgEntry)));
    if (sh.hashed) HCHK(hipMemcpyAsync(nh, sh.hm, sh.hashed * sizeof(MsgEntry), hipMemcpyDeviceToDevice, s));
    HCHK(hipStreamSynchronize(s));
    if (sh.hm) HCHK(hipFree(sh.hm));
    sh.hm = nh;
    sh.hm_cap = cap;
  }
  uint8_t *dpk = nullptr, *dsig, *dmsg;
  uint64_t* doff;
  uint32_t *dlen, *dvgoff, *darr = nullptr, *dgseg = nullptr, *dcg = nullptr;
  int64_t* dci = nullptr;
  if ((!cs && upload(d, I_PK, hpk.data(), hpk.size(), &dpk, &h)) || upload(d, I_SIG, hsig.data(), hsig.size(), &dsig, &h))
    return -1;
  PinnedUploads up;
  if (cs) {
    up.add(I_DCGRP, hcg.data(), m, &dcg);
    up.add(I_DCSHARE, hci.data(), m, &dci);
  }
  up.add(I_MSG, sh.tab.t.bytes.data() + nb0, sh.tab.t.bytes.size() - (nnew ? nb0 : sh.tab.t.bytes.size()), &dmsg);
  up.add(I_OFF, noff.data(), nnew, &doff);
  up.add(I_LEN, sh.tab.t.len.data() + sh.hashed, nnew, &dlen);
  up.add(I_MIDX, p.midx.data(), m, &dmidx);
  up.add(I_VGOFF, p.vgoff.data(), p.vgoff.size(), &dvgoff);
  up.add(I_DSERIAL, p.serial.data(), m, &dserial);
  up.add(I_DTGRP, p.tgroup.data(), nt, &dtgrp);
  up.add(I_DTOFF, p.toff.data(), p.toff.size(), &dtoff);
  up.add(I_DTPOS, p.tpos.data(), np, &dtpos);
  up.add(I_DTIDX, p.tidx.data(), np, &dtidx);
  if (sets) {
    up.add(I_DSETID, hsid.data(), m, &dsid);
    up.add(I_DARR, p.order.data(), m, &darr);
  }
  if (seg) up.add(I_DGSEG, p.vgset.data(), p.vgset.size(), &dgseg);
  if (sets && (ensure_buf(h.io[I_DSETFIRST], n_sets * sizeof(uint32_t), &psetfirst) || ensure_buf(h.io[I_DADMIT], m, &padmit)))
    return -1;
  if (upload_pinned(d, h, up) || ensure_buf(h.io[I_STAT], m, &pst) || ensure_buf(h.io[I_DSTORED], m, &pstored) ||
      ensure_buf(h.io[I_DSLOT], m * sizeof(uint32_t), &pslot) || ensure_buf(h.io[I_DMSLOT], nt * t * sizeof(uint32_t), &pmslot) ||
      ensure_buf(h.io[I_DMSER], nt * t * sizeof(uint32_t), &pmser) || ensure_buf(h.io[I_DMIDX], nt * t * sizeof(int64_t), &pmidx) ||
      ensure_buf(h.io[I_DFMSG], nt * sizeof(uint32_t), &pfmsg) || ensure_buf(h.io[I_DFKEY], nt * sizeof(uint32_t), &pfkey) ||
      ensure_buf(h.io[I_DCOPY], m * sizeof(uint2), &pcopy) || ensure_buf(h.io[I_DFIRED], nt * sizeof(uint32_t), &pfired) ||
      ensure_buf(h.io[I_DCTR], DUTY_CTRS * sizeof(uint32_t), &pctr))
    return -1;
  // phase 1: hash the messages new to the shard (with their lines: the entries stay), verify the set
  Ws& w = ws_acquire(d, s);
  this->w = &w;
  HCHK(hipEventRecord(w.ev_fork, s));
  hipStream_t shs = w.side[2];
  HCHK(hipStreamWaitEvent(shs, w.ev_fork, 0));
  if (nnew && hash_messages(d, dmsg, doff, dlen, nnew, sh.hm + sh.hashed, shs, true)) return -1;
  HCHK(hipEventRecord(w.ev_side[2], shs));
  VerifyCall vc;
  vc.pks = dpk;
  vc.sigs = dsig;
  vc.msg_idx = dmidx;
  vc.hm = sh.hm;
  vc.n = m;
  vc.grp_off = dvgoff;
  vc.n_groups = p.n_vgroups();
  vc.status = (uint8_t*)pst;
  vc.s = s;
  vc.device_entry = true;
  vc.hm_ready = w.ev_side[2];
  ClusterKeysArgs ck{};
  if (cs) {
    ck = cluster_keys_args(*cs, du.cl->n_shares, dcg, dci, false);
    vc.cluster = &ck;
    vc.cluster_wide = cs->wide;
  }
  if (seg) {  // one first failure per set: the verification itself leaves set_first (preset by it)
    vc.gseg = dgseg;
    vc.n_seg = (uint32_t)n_sets;
    vc.item_seg = dsid;
    vc.item_arrival = darr;
    vc.seg_first_out = (uint32_t*)psetfirst;
  }
  if (verify_pipeline(d, w, vc)) return -1;
  HCHK(hipStreamWaitEvent(s, w.ev_side[2], 0));
  vsig = vc.vsig;
  if (sets && !seg) {
    HCHK(hipMemsetAsync(psetfirst, 0xff, std::max<size_t>(n_sets, 1) * sizeof(uint32_t), s));
    TIMED(d, "k_duty_set_first", s,
          launch_duty_set_first((const uint8_t*)pst, dsid, darr, (uint32_t)m, (uint32_t*)psetfirst, (uint32_t)n_sets, s));
    HCHK(hipGetLastError());
  }
  if (!split) return 0;
  // end of phase one: the decompressed signatures leave the workspace set, the set goes back, and the
  // shard's verdicts per set come to the host
  void* pv;
  if (ensure_buf(h.io[I_DVSIG], m * sizeof(HmEntry), &pv)) return -1;
  HCHK(hipMemcpyAsync(pv, vsig, m * sizeof(HmEntry), hipMemcpyDeviceToDevice, s));
  vsig = (const HmEntry*)pv;
  if (ws_release(w, s)) return -1;
  this->w = nullptr;
  lk.unlock();
  if (n_sets) HCHK(hipMemcpyAsync(set_first.data(), psetfirst, n_sets * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HCHK(hipStreamSynchronize(s));
  sh.hashed = nm;
  return 0;
}

// The steps of store(), in order; hcs is held throughout; a failing step leaves lk as it is (store() drops it)
int DutyShardAdd::store_(const uint32_t* merged) {
  if (!m) return 0;
  if (gate_(merged) || store_rule_() || download_()) return -1;
  t_enq2 = t_dev1;
  if (nf && (aggregate_fired_() || download_fired_())) return -1;
  if (host_timing())
    fprintf(stderr, "hbls duty_add shard groups %zu..%zu n=%zu touched=%zu new msgs=%zu fired=%zu: plan %.2f ms, "
            "enqueue verify+store %.2f, device %.2f, enqueue aggregate+verify %.2f, device %.2f\n", sh.gb, sh.ge, m, nt,
            nnew, nf, t_prep - t_start, t_enq1 - t_prep, t_dev1 - t_enq1, t_enq2 - t_dev1, now_ms() - t_enq2);
  return 0;
}

// Phase two's upload of the call's verdicts per set, and the gate of a set add.  One segment: lk and w
// are held since verify_().  Two phases: neither is; takes lk.  Leaves lk held, w as it was.
int DutyShardAdd::gate_(const uint32_t* merged) {
  Hc& h = *hcs->h[0];
  hipStream_t s = h.s;
  if (split) {  // phase two: every shard's store sees the call's verdicts per set
    lk.lock();
    if (hipSetDevice(d.ord) != hipSuccess) return set_err("hipSetDevice failed");
    PinnedUploads upm;
    uint32_t* dm;
    upm.add(I_DSETFIRST, merged, n_sets, &dm);
    if (upload_pinned(d, h, upm)) return -1;
    psetfirst = dm;
  }
  st.vstatus = (const uint8_t*)pst;  // what the storing rule reads as the items' statuses
  if (sets) {
    TIMED(d, "k_duty_gate", s,
          launch_duty_gate((const uint8_t*)pst, dsid, (uint32_t)m, (const uint32_t*)psetfirst, (uint32_t)n_sets,
                           (uint8_t*)padmit, s));
    st.vstatus = (const uint8_t*)padmit;
  }
  return 0;
}

// store: the rule per touched group, then the stored partials' points out of the workspace.  Needs lk;
// hands w back if it is still held (one segment), then drops lk: leaves neither.
int DutyShardAdd::store_rule_() {
  hipStream_t s = hcs->h[0]->s;
  HCHK(hipMemsetAsync(pstored, 0, m, s));
  HCHK(hipMemsetAsync(pctr, 0, DUTY_CTRS * sizeof(uint32_t), s));
  st.rec_idx = sh.rec_idx;
  st.rec_msg = sh.rec_msg;
  st.rec_serial = sh.rec_serial;
  st.count = sh.count;
  st.fired = sh.fired;
  st.n_groups = (uint32_t)ng;
  st.max_stored = du.max_stored;
  st.t = du.t;
  st.msg_idx = dmidx;
  st.serial = dserial;
  st.n = (uint32_t)m;
  st.tgroup = dtgrp;
  st.toff = dtoff;
  st.tpos = dtpos;
  st.tidx = dtidx;
  st.n_touched = (uint32_t)nt;
  st.n_pos = (uint32_t)np;
  st.stored = (uint8_t*)pstored;
  st.slot = (uint32_t*)pslot;
  st.mslot = (uint32_t*)pmslot;
  st.mserial = (uint32_t*)pmser;
  st.midx = (int64_t*)pmidx;
  st.fmsg = (uint32_t*)pfmsg;
  st.fkey = (uint32_t*)pfkey;
  st.copies = (uint2*)pcopy;
  st.fired_u = (uint32_t*)pfired;
  st.ctr = (uint32_t*)pctr;
  TIMED(d, "k_duty_store", s, launch_duty_store(st, s));
  TIMED(d, "k_duty_copy", s,
        launch_duty_copy(vsig, (uint32_t)m, st.copies, st.ctr + DUTY_CTR_COPIES, (uint32_t)m, sh.store,
                         (uint32_t)(ng * du.max_stored), s));
  HCHK(hipGetLastError());
  if (w) {
    if (ws_release(*w, s)) return -1;
    w = nullptr;
  }
  lk.unlock();  // enqueued: other callers may enqueue while this one waits for its stream
  t_enq1 = now_ms();
  return 0;
}

// The items' verdicts and stored flags to the caller, nf and hfired to the host, behind the stream's end.
// Needs and leaves no lock and no workspace set.
int DutyShardAdd::download_() {
  hipStream_t s = hcs->h[0]->s;
  std::vector<uint8_t> hst(m), hstored(m);
  hfired.assign(nt, 0);
  uint32_t hctr[DUTY_CTRS] = {};
  if (sets && !split && n_sets)  // one shard: the sets' verdicts come back with the items'
    HCHK(hipMemcpyAsync(set_first.data(), psetfirst, n_sets * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HCHK(hipMemcpyAsync(hst.data(), pst, m, hipMemcpyDeviceToHost, s));
  HCHK(hipMemcpyAsync(hstored.data(), pstored, m, hipMemcpyDeviceToHost, s));
  HCHK(hipMemcpyAsync(hctr, pctr, sizeof(hctr), hipMemcpyDeviceToHost, s));
  if (nt) HCHK(hipMemcpyAsync(hfired.data(), pfired, nt * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HCHK(hipStreamSynchronize(s));
  sh.hashed = nm;
  t_dev1 = now_ms();
  for (size_t q = 0; q < m; q++) {
    a.vstatus[p.order[q]] = hst[q];
    a.stored[p.order[q]] = hstored[q];
    out.n_stored += hstored[q] ? 1 : 0;
  }
  out.n_full = hctr[DUTY_CTR_FULL];
  nf = hctr[DUTY_CTR_FIRED];
  if (nf > nt) return set_err(std::string(a.who) + ": the fired list is longer than the touched groups");
  return 0;
}

// The fired groups, ascending: their members are in the store.  k_duty_gather fills the candidates;
// behind it the shared tail, as phases 3 and 4 of slot_select_core.  Needs neither lk nor a workspace
// set; takes lk and a set of its own, hands the set back, then drops lk: leaves neither.
int DutyShardAdd::aggregate_fired_() {
  Hc& h = *hcs->h[0];
  hipStream_t s = h.s;
  std::sort(hfired.begin(), hfired.begin() + nf);
  for (size_t k = 0; k < nf; k++)
    if (hfired[k] >= nt) return set_err(std::string(a.who) + ": a fired row names no touched group");
  lk.lock();
  if (hipSetDevice(d.ord) != hipSuccess) return set_err("hipSetDevice failed");
  uint32_t* dfrow;
  PinnedUploads up2;
  up2.add(I_DFROW, hfired.data(), nf, &dfrow);
  void *pmem, *pdv = nullptr;  // (a cluster duty gathers no DV key bytes: k_cluster_keys resolves them by fired group id)
  if (upload_pinned(d, h, up2) || ensure_buf(h.io[I_CAND], nf * t * sizeof(uint32_t), &pmem) ||
      ensure_buf(h.io[I_CHOSEN], nf * t * sizeof(uint32_t), &pser) || ensure_buf(h.io[I_DFGRP], nf * sizeof(uint32_t), &pfg) ||
      (!sh.cs && ensure_buf(h.io[I_DVPK], 48 * nf, &pdv)) || ensure_buf(h.io[I_TAOUT], 96 * nf, &ptout) ||
      ensure_buf(h.io[I_TAST], nf, &ptst) || ensure_buf(h.io[I_AGGST], nf, &past))
    return -1;
  Ws& w2 = ws_acquire(d, s);
  SelWs x;
  if (sel_ws(w2, nf, t, s, x)) return -1;
  TaSelectArgs& sa = x.sa;
  sa.chosen = (uint32_t*)pmem;
  DutyGatherArgs ga{};
  ga.n_fired = (uint32_t)nf;
  ga.n_touched = (uint32_t)nt;
  ga.n_groups = (uint32_t)ng;
  ga.max_stored = du.max_stored;
  ga.t = du.t;
  ga.group_base = (uint32_t)sh.gb;
  ga.frow = dfrow;
  ga.tgroup = dtgrp;
  ga.mslot = st.mslot;
  ga.mserial = st.mserial;
  ga.midx = st.midx;
  ga.fmsg = st.fmsg;
  ga.fkey = st.fkey;
  ga.dv_pks = sh.cs ? nullptr : sh.dvpk;
  ga.chosen = sa.chosen;
  ga.cidx = sa.cidx;
  ga.key = sa.key;
  ga.state = sa.state;
  ga.gmsg = sa.gmsg;
  ga.hist = sa.hist;
  ga.serials = (uint32_t*)pser;
  ga.fired_g = (uint32_t*)pfg;
  ga.dv_out = (uint8_t*)pdv;
  TIMED(d, "k_duty_gather", s, launch_duty_gather(ga, s));
  if (sel_aggregate(d, w2, x, sh.store, sh.store_st, (uint8_t*)ptout, (uint8_t*)ptst, sh.selctr, s)) return -1;
  VerifyCall v2;  // the aggregates under the DV keys gathered by group id; the messages' lines are resident
  v2.pks = (const uint8_t*)pdv;
  v2.hm = sh.hm;
  ClusterKeysArgs ck{};
  if (sh.cs) {  // a cluster duty: the DV keys from the cluster by fired group id (no bytes were gathered: pdv is null)
    ck = cluster_keys_args(*sh.cs, du.cl->n_shares, (const uint32_t*)pfg, nullptr, false);
    v2.cluster = &ck;
    v2.cluster_wide = sh.cs->wide;
    out.n_dv = nf;
  }
  if (sel_verify(d, w2, x, v2, (const uint8_t*)ptst, (uint8_t*)past, s)) return -1;
  if (ws_release(w2, s)) return -1;
  lk.unlock();
  t_enq2 = now_ms();
  return 0;
}

// The fired groups' rows to the shard's output.  No lock, no workspace set; waits for the stream.
int DutyShardAdd::download_fired_() {
  hipStream_t s = hcs->h[0]->s;
  out.fired.resize(nf);
  out.chosen.resize(nf * t);
  out.ta_out.resize(96 * nf);
  out.ta_status.resize(nf);
  out.agg_vstatus.resize(nf);
  HCHK(hipMemcpyAsync(out.fired.data(), pfg, nf * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HCHK(hipMemcpyAsync(out.chosen.data(), pser, nf * t * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HCHK(hipMemcpyAsync(out.ta_out.data(), ptout, 96 * nf, hipMemcpyDeviceToHost, s));
  HCHK(hipMemcpyAsync(out.ta_status.data(), ptst, nf, hipMemcpyDeviceToHost, s));
  HCHK(hipMemcpyAsync(out.agg_vstatus.data(), past, nf, hipMemcpyDeviceToHost, s));
  HCHK(hipStreamSynchronize(s));
  return 0;
}

// A checked, non-empty add (duty_add_entry) over the duty's shards
int duty_add(Duty& du, const DutyAddArgs& a) {
  const DutySetCall* const sets = a.sets;
  const size_t n = a.n, nd = du.sh.size(), t = du.t, n_sets = sets ? sets->n_sets : 0;
  const std::string who = a.who;
  const size_t gmax = call_gmax(n, g_single_max.load(), g_fe_batch_min.load(), g_gmax.load());
  std::vector<std::vector<uint32_t>> items;
  duty_route(a.group, n, du.n_groups, nd, items);
  std::vector<DutyShardOut> outs(nd);
  std::vector<DutyShardAdd> adds;
  adds.reserve(nd);
  for (size_t k = 0; k < nd; k++) adds.emplace_back(du, du.sh[k], a, items[k], gmax, outs[k]);
  // every shard runs fn (run_shards: concurrently, all joined before this returns)
  auto each = [&](const std::function<int(size_t)>& fn) {
    const int rc = each_shard(who, du.sh, fn);
    if (rc) du.broken = true;  // a shard may have stored what another did not verify: the duty's state is no longer one stream's
    return rc;
  };
  std::vector<uint32_t> merged(n_sets, DUTY_NONE);
  if (!sets || nd == 1) {  // one stream segment per shard
    if (each([&](size_t k) { return adds[k].verify(false) ? -1 : adds[k].store(nullptr); })) return -1;
    if (sets) merged = adds[0].set_first;
  } else {
    // a set's verdict needs every shard's verification: phase one everywhere, the shards joined (none
    // parked, no device lock and no workspace set held), the element-wise min, then phase two everywhere.  A failure in
    // phase one leaves nothing stored anywhere.
    // the shards' contexts first, in the one global order (DutyShardAdd's invariant)
    std::vector<size_t> ord(nd);
    std::iota(ord.begin(), ord.end(), size_t(0));
    std::sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return std::less<Dev*>()(du.sh[x].d, du.sh[y].d); });
    for (size_t k : ord) adds[k].lease();
    if (each([&](size_t k) { return adds[k].verify(true); })) return -1;
    for (size_t k = 0; k < nd; k++) duty_merge_set_first(merged.data(), adds[k].set_first.data(), n_sets);
    if (each([&](size_t k) { return adds[k].store(merged.data()); })) return -1;
  }
  if (sets) {
    uint64_t rejected = 0, lost = 0;
    for (size_t k = 0; k < n_sets; k++) {
      const uint32_t f = merged[k], b = sets->set_off[k], e = sets->set_off[k + 1];
      if (f == DUTY_NONE) continue;
      if (f < b || f >= e) {
        du.broken = true;
        return set_err(who + ": a set's first failure lies outside the set");
      }
      rejected++;
      for (uint32_t i = b; i < e; i++) lost += a.vstatus[i] == HBLS_OK ? 1 : 0;
    }
    if (n_sets) memcpy(a.set_first, merged.data(), n_sets * sizeof(uint32_t));
    du.set_stats[0] += n_sets;
    du.set_stats[1] += rejected;
    du.set_stats[2] += lost;
    if (sets->first) {
      du.first_stats[0] += n;
      for (size_t i = 0; i < n; i++) du.first_stats[1] += a.vstatus[i] == HBLS_UNCHECKED ? 1 : 0;
    }
  }
  size_t nf = 0;  // the shards own ascending ranges of the groups: their lists concatenate in order
  for (size_t k = 0; k < nd; k++) {
    const DutyShardOut& o = outs[k];
    const size_t f = o.fired.size();
    if (f) {
      memcpy(a.fired + nf, o.fired.data(), f * sizeof(uint32_t));
      memcpy(a.chosen + nf * t, o.chosen.data(), f * t * sizeof(uint32_t));
      memcpy(a.ta_out + 96 * nf, o.ta_out.data(), 96 * f);
      memcpy(a.ta_status + nf, o.ta_status.data(), f);
      memcpy(a.agg_vstatus + nf, o.agg_vstatus.data(), f);
      nf += f;
    }
    du.stats[1] += o.n_stored;
    du.stats[2] += o.n_new_msgs;
    du.stats[3] += o.resident;
    du.stats[5] += o.n_full;
    if (du.cl) {  // counted here, behind every shard's last download: a failed add counts nothing
      du.cl->stats[3] += o.n_named;
      du.cl->stats[4] += o.n_nokey;
      du.cl->stats[5] += o.n_dv;
    }
  }
  du.stats[0] += n;
  du.stats[4] += nf;
  du.next_serial += (uint32_t)n;
  *a.n_fired = nf;
  return 0;
}

int duty_state(Duty& du, uint32_t* stored_count, uint8_t* fired_flag) {
  for (DutyShard& s : du.sh) {
    const size_t ng = s.ge - s.gb;
    if (!ng) continue;
    std::lock_guard<std::mutex> lk(s.d->mu);
    if (hipSetDevice(s.d->ord) != hipSuccess) return set_err("hipSetDevice failed");
    // every add has drained its stream (the duty's invariant): a plain copy sees the final records
    HCHK(hipMemcpy(stored_count + s.gb, s.count, ng * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HCHK(hipMemcpy(fired_flag + s.gb, s.fired, ng, hipMemcpyDeviceToHost));
  }
  return 0;
}

// hbls_duty_stats, hbls_duty_set_stats and hbls_duty_first_stats: the first n of one of the duty's counter arrays
template <size_t N>
int duty_counters(const std::string& who, uint64_t duty, uint64_t (Duty::*ctr)[N], uint64_t* out, size_t n) {
  if (ensure_init()) return -1;
  std::shared_ptr<Duty> du = duty_get(who, duty);
  if (!du || counters_args(who, out, n, N)) return -1;
  std::lock_guard<std::mutex> l(du->mu);
  if (du->closed) return set_err(who + ": the duty is closed");
  counters_copy((*du).*ctr, out, n);
  return 0;
}

// A checked hbls_duty_open / hbls_duty_open_cluster begins: the handle's place, the threshold, max_stored
int duty_open_check(const std::string& who, const uint64_t* duty, uint32_t threshold, uint32_t max_stored) {
  if (!duty) return set_err(who + ": duty is required");
  if (threshold < 1 || threshold > (uint32_t)TA_SMALL_MAX)
    return set_err(who + ": threshold must be in 1.." + std::to_string(TA_SMALL_MAX));
  if (max_stored < 1 || max_stored > DUTY_MAX_STORED)
    return set_err(who + ": max_stored must be in 1.." + std::to_string(DUTY_MAX_STORED));
  return 0;
}

// hbls_key_learn_stats, hbls_key_wide_stats and hbls_subgroup_batch_stats: for each device of the mask (at
// most max_devices), under its lock and behind everything enqueued so far, its counter struct C (ctr; with
// `optional`, zeros while it is not allocated) as the row fill(dev, counters) of out, `stride` counters long
template <class C, size_t stride, class Fill>
int device_counters(const std::string& who, DevBuf Dev::*ctr, bool optional, uint64_t* out, size_t max_devices,
                    size_t* n_devices, Fill fill) {
  if (ensure_init()) return -1;
  if (!out || !n_devices) return set_err(who + ": null arguments");
  size_t k = 0;
  for (Dev* d : devs()) {
    if (k == max_devices) break;
    std::lock_guard<std::mutex> lk(d->mu);
    HCHK(hipSetDevice(d->ord));
    C c{};
    if (!optional || (d->*ctr).p) {
      if (drain_lib_streams(*d)) return -1;
      HCHK(hipMemcpy(&c, (d->*ctr).p, sizeof(c), hipMemcpyDeviceToHost));
    }
    const std::array<uint64_t, stride> row = fill(*d, c);
    std::copy(row.begin(), row.end(), out + stride * k++);
  }
  *n_devices = k;
  return 0;
}

// Signing roots (roots.hip).  mode 0: data = 128-byte SSZ AttestationData; 1: data = 32-byte
// object roots.  Host buffers; dom_idx nullable.
int roots_host(int mode, const uint8_t* data, size_t n, const uint8_t* domains, size_t n_domains, const uint32_t* dom_idx,
               uint8_t* roots) {
  if (n_domains == 0) return set_err("signing roots: no domain");
  if (dom_idx)
    for (size_t i = 0; i < n; i++)
      if (dom_idx[i] >= n_domains) return set_err("signing roots: domain index out of range");
  const size_t item = mode == 0 ? 128 : 32;
  return for_each_device(n, [&](Dev& d, size_t b, size_t e) -> int {
    const size_t m = e - b;
    uint8_t *dd, *ddom;
    uint32_t* didx = nullptr;
    if (upload(d, I_SIG, data + item * b, m * item, &dd) || upload(d, I_PK, domains, n_domains * 32, &ddom)) return -1;
    if (dom_idx && upload(d, I_MIDX, dom_idx + b, m, &didx)) return -1;
    void* out;
    if (ensure_buf(d.io[I_OUT], m * 32, &out)) return -1;
    if (mode == 0)
      TIMED(d, "k_attestation_roots", d.stream,
            launch_attestation_roots(dd, (uint32_t)m, ddom, (uint32_t)n_domains, didx, (uint8_t*)out, d.stream));
    else
      TIMED(d, "k_signing_roots", d.stream,
            launch_signing_roots(dd, (uint32_t)m, ddom, (uint32_t)n_domains, didx, (uint8_t*)out, d.stream));
    HCHK(hipMemcpyAsync(roots + 32 * b, out, m * 32, hipMemcpyDeviceToHost, d.stream));
    HCHK(hipStreamSynchronize(d.stream));
    return 0;
  });
}

// ---------------------------------------------------------------------------------------
// RCCL: one communicator per process (one GPU each) for the exchange of slot results
// ---------------------------------------------------------------------------------------
ncclComm_t g_comm = nullptr;
int g_comm_ranks = 0;

#define NCHK(expr)                                                                        \
  do {                                                                                    \
    ncclResult_t _r = (expr);                                                             \
    if (_r != ncclSuccess) return set_err(std::string(#expr) + ": " + ncclGetErrorString(_r)); \
  } while (0)

}  // namespace

// ---------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------
extern "C" {

int hbls_init(uint32_t device_mask) { return init_mask(device_mask); }

const char* hbls_last_error(void) { return g_err.c_str(); }

int hbls_available(void) { return ensure_init() == 0 ? 1 : 0; }

#ifndef HBLS_BUILD_ID
#define HBLS_BUILD_ID "hbls-build:unversioned"
#endif
const char* hbls_build_id(void) { return HBLS_BUILD_ID; }

int hbls_device_count(void) { return ensure_init() ? -1 : (int)devs().size(); }

size_t hbls_hm_entry_bytes(void) { return sizeof(MsgEntry); }

int hbls_verify_batch(const uint8_t* pks, const uint8_t* sigs, const uint8_t* msgs, const uint64_t* msg_off,
                      const uint32_t* msg_len, size_t n, uint8_t* status) {
  if (ensure_init()) return -1;
  if (n == 0) return 0;
  return verify_coalesced(pks, sigs, msgs, msg_off, msg_len, n, status);
}

int hbls_verify_batch_first_error(const uint8_t* pks, const uint8_t* sigs, const uint8_t* msgs, const uint64_t* msg_off,
                                  const uint32_t* msg_len, size_t n, int64_t* first, uint8_t* first_status,
                                  uint8_t* status) {
  if (ensure_init()) return -1;
  if (!first) return set_err("verify first error: no output for the index");
  return verify_first_host(pks, sigs, msgs, msg_off, msg_len, n, first, first_status, status);
}

int hbls_threshold_aggregate_batch(const uint8_t* sigs, const int64_t* idx, const uint32_t* grp_off, size_t n_groups,
                                   uint8_t* out, uint8_t* status) {
  if (ensure_init()) return -1;
  if (n_groups == 0) return 0;
  return group_op_host(sigs, idx, grp_off, n_groups, 0, out, status);
}

int hbls_aggregate_batch(const uint8_t* sigs, const uint32_t* grp_off, size_t n_groups, uint8_t* out,
                         uint8_t* status) {
  if (ensure_init()) return -1;
  if (n_groups == 0) return 0;
  return group_op_host(sigs, nullptr, grp_off, n_groups, 1, out, status);
}

int hbls_verify_aggregate_batch(const uint8_t* pks, const uint32_t* grp_off, const uint8_t* sigs,
                                const uint8_t* msgs, const uint64_t* msg_off, const uint32_t* msg_len,
                                size_t n_groups, uint8_t* status) {
  if (ensure_init()) return -1;
  if (n_groups == 0) return 0;
  if (check_offsets(grp_off, n_groups)) return -1;
  return for_each_device_hc(n_groups, [&](Dev& d, Hc& h, size_t gb, size_t ge, std::unique_lock<std::mutex>& lk) -> int {
    const size_t ng = ge - gb, pb = grp_off[gb], np = grp_off[ge] - pb;
    if (ng == 0) return 0;
    MsgTable t;  // one hash per group (messages need not be distinct)
    t.idx.resize(ng);
    for (size_t g = gb; g < ge; g++) {
      t.off.push_back(t.bytes.size());
      t.len.push_back(msg_len[g]);
      t.bytes.insert(t.bytes.end(), msgs + msg_off[g], msgs + msg_off[g] + msg_len[g]);
    }
    std::vector<uint32_t> goff(ng + 1);
    for (size_t g = 0; g <= ng; g++) goff[g] = grp_off[gb + g] - (uint32_t)pb;
    uint8_t *dpk, *dsig;
    if (upload(d, I_PK, pks + 48 * pb, np * 48, &dpk, &h) || upload(d, I_SIG, sigs + 96 * gb, ng * 96, &dsig, &h))
      return -1;
    void* p;
    if (ensure_buf(h.io[I_STAT], ng, &p)) return -1;
    Ws& w = ws_acquire(d, h.s);
    uint8_t* dst = (uint8_t*)p;
    void* hmp;  // the message table's buffer (hash_table fills the same one on the call's stream)
    if (ensure_buf(h.io[I_HM], ng * sizeof(MsgEntry), &hmp)) return -1;
    MsgEntry* hm = (MsgEntry*)hmp;
    VaKeys keys;
    keys.dpk = dpk;
    if (va_pipeline(d, w, keys, np, goff.data(), ng, dsig, hm, dst, h.s,
                    [&]() -> int { MsgEntry* hx; return hash_table(d, t, &hx, true, &h); }))
      return -1;
    if (ws_release(w, h.s)) return -1;
    lk.unlock();  // enqueued: other callers may enqueue while this one waits for its stream
    HCHK(hipMemcpyAsync(status + gb, dst, ng, hipMemcpyDeviceToHost, h.s));
    HCHK(hipStreamSynchronize(h.s));
    return 0;
  });
}

int hbls_attestation_signing_roots(const uint8_t* data, size_t n, const uint8_t* domains, size_t n_domains,
                                   const uint32_t* dom_idx, uint8_t* roots) {
  if (ensure_init()) return -1;
  if (n == 0) return 0;
  return roots_host(0, data, n, domains, n_domains, dom_idx, roots);
}

int hbls_signing_roots(const uint8_t* object_roots, size_t n, const uint8_t* domains, size_t n_domains,
                       const uint32_t* dom_idx, uint8_t* roots) {
  if (ensure_init()) return -1;
  if (n == 0) return 0;
  return roots_host(1, object_roots, n, domains, n_domains, dom_idx, roots);
}

int hbls_duty_signing_roots(int kind, const uint8_t* data, const uint64_t* off, const uint32_t* len, size_t n,
                            const uint8_t* domains, size_t n_domains, const uint32_t* dom_idx, uint8_t* roots,
                            uint8_t* status) {
  if (ensure_init()) return -1;
  if (n == 0) return 0;
  if (kind < 1 || kind > 9) return set_err("duty signing roots: unknown kind");
  if (n_domains == 0) return set_err("signing roots: no domain");
  if (dom_idx)
    for (size_t i = 0; i < n; i++)
      if (dom_idx[i] >= n_domains) return set_err("signing roots: domain index out of range");
  return for_each_device(n, [&](Dev& d, size_t b, size_t e) -> int {
    const size_t m = e - b;
    // the shard's objects packed: their bytes from the first object's offset on, offsets rebased
    uint64_t lo = ~0ull, hi = 0;
    for (size_t i = b; i < e; i++) {
      lo = std::min(lo, off[i]);
      hi = std::max(hi, off[i] + len[i]);
    }
    std::vector<uint64_t> roff(m);
    for (size_t i = 0; i < m; i++) roff[i] = off[b + i] - lo;
    uint8_t *dd, *ddom;
    uint64_t* doff;
    uint32_t *dlen, *didx = nullptr;
    if (upload(d, I_SIG, data + lo, hi - lo, &dd) || upload(d, I_PK, domains, n_domains * 32, &ddom) ||
        upload(d, I_OFF, roff.data(), m, &doff) || upload(d, I_LEN, len + b, m, &dlen))
      return -1;
    if (dom_idx && upload(d, I_MIDX, dom_idx + b, m, &didx)) return -1;
    void *out, *st;
    if (ensure_buf(d.io[I_OUT], m * 32, &out) || ensure_buf(d.io[I_STAT], m, &st)) return -1;
    TIMED(d, "k_duty_roots", d.stream,
          launch_duty_roots(kind, dd, doff, dlen, (uint32_t)m, ddom, (uint32_t)n_domains, didx, (uint8_t*)out,
                            (uint8_t*)st, d.stream));
    HCHK(hipMemcpyAsync(roots + 32 * b, out, m * 32, hipMemcpyDeviceToHost, d.stream));
    HCHK(hipMemcpyAsync(status + b, st, m, hipMemcpyDeviceToHost, d.stream));
    HCHK(hipStreamSynchronize(d.stream));
    return 0;
  });
}

int hbls_sign_batch(const uint8_t* sks, const uint8_t* msgs, const uint64_t* msg_off, const uint32_t* msg_len,
                    size_t n, uint8_t* sigs, uint8_t* status) {
  if (ensure_init()) return -1;
  if (n == 0) return 0;
  return for_each_device(n, [&](Dev& d, size_t b, size_t e) -> int {
    const size_t m = e - b;
    std::vector<size_t> items(m);
    std::iota(items.begin(), items.end(), b);
    MsgTable t;
    dedup_messages(msgs, msg_off, msg_len, m, items.data(), t);
    MsgEntry* hm;
    if (hash_table(d, t, &hm, false)) return -1;
    uint8_t* dsk;
    uint32_t* didx;
    if (upload(d, I_SK, sks + 32 * b, m * 32, &dsk) || upload(d, I_MIDX, t.idx.data(), m, &didx)) return -1;
    void *dout, *dst;
    if (ensure_buf(d.io[I_OUT], m * 96, &dout) || ensure_buf(d.io[I_STAT], m, &dst)) return -1;
    LAUNCH(k_sign, m, d.stream, dsk, didx, hm, (uint32_t)m, (uint8_t*)dout, (uint8_t*)dst);
    HCHK(hipMemcpyAsync(sigs + 96 * b, dout, m * 96, hipMemcpyDeviceToHost, d.stream));
    HCHK(hipMemcpyAsync(status + b, dst, m, hipMemcpyDeviceToHost, d.stream));
    HCHK(hipStreamSynchronize(d.stream));
    return 0;
  });
}

int hbls_secret_to_public_key_batch(const uint8_t* sks, size_t n, uint8_t* pks, uint8_t* status) {
  if (ensure_init()) return -1;
  if (n == 0) return 0;
  return for_each_device(n, [&](Dev& d, size_t b, size_t e) -> int {
    const size_t m = e - b;
    uint8_t* dsk;
    if (upload(d, I_SK, sks + 32 * b, m * 32, &dsk)) return -1;
    void *dout, *dst;
    if (ensure_buf(d.io[I_OUT], m * 48, &dout) || ensure_buf(d.io[I_STAT], m, &dst)) return -1;
    LAUNCH(k_sk_to_pk, m, d.stream, dsk, (uint32_t)m, (uint8_t*)dout, (uint8_t*)dst);
    HCHK(hipMemcpyAsync(pks + 48 * b, dout, m * 48, hipMemcpyDeviceToHost, d.stream));
    HCHK(hipMemcpyAsync(status + b, dst, m, hipMemcpyDeviceToHost, d.stream));
    HCHK(hipStreamSynchronize(d.stream));
    return 0;
  });
}

int hbls_threshold_split(const uint8_t* secret, const uint8_t* coeffs, uint32_t total, uint32_t threshold,
                         uint8_t* shares, uint8_t* status) {
  if (ensure_init()) return -1;
  if (total == 0 || threshold == 0) return 0;
  std::vector<uint8_t> poly(32ull * threshold);
  memcpy(poly.data(), secret, 32);
  if (threshold > 1) memcpy(poly.data() + 32, coeffs, 32ull * (threshold - 1));
  return for_each_device(1, [&](Dev& d, size_t, size_t) -> int {
    uint8_t* dpoly;
    if (upload(d, I_SK, poly.data(), poly.size(), &dpoly)) return -1;
    void *dout, *dst;
    if (ensure_buf(d.io[I_OUT], 32ull * total, &dout) || ensure_buf(d.io[I_STAT], total, &dst)) return -1;
    LAUNCH(k_split, total, d.stream, dpoly, threshold, total, (uint8_t*)dout, (uint8_t*)dst);
    HCHK(hipMemcpyAsync(shares, dout, 32ull * total, hipMemcpyDeviceToHost, d.stream));
    HCHK(hipMemcpyAsync(status, dst, total, hipMemcpyDeviceToHost, d.stream));
    HCHK(hipStreamSynchronize(d.stream));
    return 0;
  });
}

int hbls_recover_secret(const uint8_t* shares, const int64_t* idx, size_t k, uint8_t* out, uint8_t* status) {
  if (ensure_init()) return -1;
  return for_each_device(1, [&](Dev& d, size_t, size_t) -> int {
    uint8_t* dsh;
    int64_t* didx;
    std::vector<uint8_t> dummy(32);
    if (upload(d, I_SK, k ? shares : dummy.data(), k ? 32 * k : 32, &dsh)) return -1;
    std::vector<int64_t> di(k ? k : 1, 0);
    if (k) memcpy(di.data(), idx, 8 * k);
    if (upload(d, I_IDX, di.data(), di.size(), &didx)) return -1;
    void *dout, *dst;
    if (ensure_buf(d.io[I_OUT], 32, &dout) || ensure_buf(d.io[I_STAT], 1, &dst)) return -1;
    hipLaunchKernelGGL(k_recover, dim3(1), dim3(64), 0, d.stream, dsh, didx, (uint32_t)k, (uint8_t*)dout,
                       (uint8_t*)dst);
    HCHK(hipGetLastError());
    HCHK(hipMemcpyAsync(out, dout, 32, hipMemcpyDeviceToHost, d.stream));
    HCHK(hipMemcpyAsync(status, dst, 1, hipMemcpyDeviceToHost, d.stream));
    HCHK(hipStreamSynchronize(d.stream));
    return 0;
  });
}

// ---- device-buffer entry points (slot pipeline) ----
int hbls_hash_to_g2_device(const uint8_t* msgs, const uint64_t* msg_off, const uint32_t* msg_len, size_t n_msgs,
                           void* hm, void* stream) {
  Dev* d;
  hipStream_t s = (hipStream_t)stream;
  if (dev_of_stream(s, &d)) return -1;
  std::lock_guard<std::mutex> lk(d->mu);
  return hash_messages(*d, msgs, msg_off, msg_len, n_msgs, (MsgEntry*)hm, s);
}

int hbls_verify_device(const uint8_t* pks, const uint8_t* sigs, const uint32_t* msg_idx, const void* hm, size_t n,
                       const uint32_t* vgrp_off, size_t n_vgroups, uint8_t* status, void* stream) {
  Dev* d;
  hipStream_t s = (hipStream_t)stream;
  if (dev_of_stream(s, &d)) return -1;
  if (n == 0) return 0;
  std::lock_guard<std::mutex> lk(d->mu);
  Ws& w = ws_acquire(*d, s);
  VerifyCall vc;
  vc.pks = pks;
  vc.sigs = sigs;
  vc.msg_idx = msg_idx;
  vc.hm = (const MsgEntry*)hm;
  vc.n = n;
  vc.grp_off = vgrp_off;
  vc.n_groups = n_vgroups;
  vc.status = status;
  vc.s = s;
  vc.device_entry = true;
  if (verify_pipeline(*d, w, vc)) return -1;
  return ws_release(w, s);
}

int hbls_verify_device_first_error(const uint8_t* pks, const uint8_t* sigs, const uint32_t* msg_idx, const void* hm,
                                   size_t n, const uint32_t* vgrp_off, size_t n_vgroups, uint8_t* status,
                                   uint32_t* first, void* stream) {
  Dev* d;
  hipStream_t s = (hipStream_t)stream;
  if (dev_of_stream(s, &d)) return -1;
  if (!first) return set_err("verify first error: no output for the index");
  if (n == 0) {
    HCHK(hipMemsetAsync(first, 0xff, sizeof(uint32_t), s));
    return 0;
  }
  if (n >= 0xffffffffull) return set_err("verify first error: too many items");
  std::lock_guard<std::mutex> lk(d->mu);
  Ws& w = ws_acquire(*d, s);
  VerifyCall vc;
  vc.pks = pks;
  vc.sigs = sigs;
  vc.msg_idx = msg_idx;
  vc.hm = (const MsgEntry*)hm;
  vc.n = n;
  vc.grp_off = vgrp_off;
  vc.n_groups = n_vgroups;
  vc.status = status;
  vc.s = s;
  vc.device_entry = true;
  vc.first_out = first;
  if (verify_pipeline(*d, w, vc)) return -1;
  return ws_release(w, s);
}

size_t hbls_pk_entry_bytes(void) { return sizeof(G1AEntry); }

int hbls_pubkey_cache_add(const uint8_t* pks, size_t n) {
  if (ensure_init()) return -1;
  std::lock_guard<std::mutex> al(g_kc_add_mu);
  std::vector<uint8_t> fresh;
  std::unordered_map<std::string, uint32_t> add;
  {
    std::lock_guard<std::mutex> lk(g_kc_mu);
    for (size_t k = 0; k < n; k++) {
      std::string key((const char*)pks + 48 * k, 48);
      if (g_kc_map.count(key) || add.count(key)) continue;
      add.emplace(key, (uint32_t)(g_kc_n + add.size()));
      fresh.insert(fresh.end(), pks + 48 * k, pks + 48 * k + 48);
    }
  }
  const size_t m = add.size();
  if (m == 0) return 0;
  if (g_kc_n + m > 0xffffffffull) return set_err("pubkey cache full");
  for (Dev* dp : devs()) {  // the device work under each Dev::mu in turn, g_kc_mu not held
    std::lock_guard<std::mutex> dl(dp->mu);
    if (kc_fill(*dp, fresh.data(), g_kc_n, m)) return -1;
  }
  g_kc_keys.insert(g_kc_keys.end(), fresh.begin(), fresh.end());
  std::lock_guard<std::mutex> lk(g_kc_mu);  // publish: lookups see the entries only now
  for (auto& kv : add) g_kc_map.emplace(kv.first, kv.second);
  g_kc_n += m;
  return 0;
}

size_t hbls_sig_cache(size_t entries) {
  if (ensure_init()) return 0;
  while (entries & (entries - 1)) entries &= entries - 1;
  entries = std::min<size_t>(entries, size_t(1) << 30);
  const size_t old = g_sc_cap.exchange(entries);
  for (Dev* d : devs()) {  // drop the contents: the next put allocates at the new capacity
    std::lock_guard<std::mutex> lk(d->mu);
    d->sc_filled = 0;
    d->sc_cap = 0;
  }
  return old;
}

int hbls_pubkey_cache_clear(void) {
  std::lock_guard<std::mutex> al(g_kc_add_mu);
  for (Dev* dp : devs()) {  // no verification enqueued after this sees the old entries
    std::lock_guard<std::mutex> dl(dp->mu);
    dp->kc_n = 0;
    dp->kc_tcap = 0;  // the next fill builds a fresh index
    if (kl_reset(*dp, false)) return -1;  // the learned keys too
  }
  std::lock_guard<std::mutex> lk(g_kc_mu);
  g_kc_map.clear();
  g_kc_n = 0;
  g_kc_keys.clear();
  return 0;
}

size_t hbls_pubkey_cache_size(void) {
  std::lock_guard<std::mutex> lk(g_kc_mu);
  return g_kc_n;
}

int hbls_key_learn_stats(uint64_t* out, size_t max_devices, size_t* n_devices) {
  return device_counters<KeyLearnCtr, 4>("hbls_key_learn_stats", &Dev::kl_ctr, true, out, max_devices, n_devices,
                                         [](const Dev& d, const KeyLearnCtr& c) -> std::array<uint64_t, 4> {
                                           return {d.kl_cap ? std::min<uint64_t>(c.size, d.kl_cap) : 0, g_key_learn.load(), c.hits, c.misses};
                                         });
}

// The ladder tables of the learned keys, per device of the mask and cumulative: out[5 k + 0] tables
// built, + 1 / + 2 chunks of the chunked combination's key side combined through tables / without,
// + 3 / + 4 per-item key-side ladders through tables / without.  Waits like hbls_key_learn_stats.
int hbls_key_wide_stats(uint64_t* out, size_t max_devices, size_t* n_devices) {
  return device_counters<KeyLearnCtr, 5>("hbls_key_wide_stats", &Dev::kl_ctr, true, out, max_devices, n_devices,
                                         [](const Dev&, const KeyLearnCtr& c) -> std::array<uint64_t, 5> {
                                           return {c.wide_built, c.wide_chunks, c.narrow_chunks, c.wide_items, c.narrow_items};
                                         });
}

// The batched subgroup test, per device of the mask and cumulative: out[4 k + 0] batched tests run,
// + 1 batched tests that failed, + 2 signatures that went through the per-item ladders of calls
// large enough for the test, + 3 calls that skipped the test by the adaptive history.  Waits like
// hbls_key_wide_stats; its counters are allocated with the device, so there is no unallocated case.
int hbls_subgroup_batch_stats(uint64_t* out, size_t max_devices, size_t* n_devices) {
  return device_counters<SubgCtr, 4>("hbls_subgroup_batch_stats", &Dev::sg_ctr, false, out, max_devices, n_devices,
                                     [](const Dev&, const SubgCtr& c) -> std::array<uint64_t, 4> {
                                       return {c.run, c.failed, c.laddered, c.skipped};
                                     });
}

// Test switch of the in-process multi-device split: every device of the mask is driven through
// `copies` contexts (streams, workspaces, host thread), so host-buffer calls shard over them as
// over several GPUs (for_each_device) on a one-GPU box.  Call while no other call is in flight.
int hbls_debug_split(uint32_t copies) {
  if (ensure_init()) return -1;
  if (copies == 0 || copies > 16) return set_err("hbls_debug_split: copies must be in 1..16");
  std::lock_guard<std::mutex> il(g_init_mu);
  std::lock_guard<std::mutex> al(g_kc_add_mu);
  std::vector<Dev*> devs;
  g_split_pool.resize(g_base_devs.size());
  for (size_t bi = 0; bi < g_base_devs.size(); bi++) {
    Dev* b = g_base_devs[bi];
    std::vector<Dev*>& pool = g_split_pool[bi];
    devs.push_back(b);
    for (uint32_t c = 1; c < copies; c++) {
      if (pool.size() < c) {
        Dev* d;
        if (dev_create(b->ord, &d)) return -1;
        pool.push_back(d);
      }
      Dev* d = pool[c - 1];
      d->timing = b->timing;
      d->serial = b->serial;
      std::lock_guard<std::mutex> dl(d->mu);
      if (hipSetDevice(d->ord) != hipSuccess) return set_err("hipSetDevice failed");
      if (g_kc_n && kc_fill(*d, g_kc_keys.data(), 0, g_kc_n)) return -1;  // the same key cache
      devs.push_back(d);
    }
  }
  std::lock_guard<std::mutex> l(g_devs_mu);
  g_devs = devs;
  return 0;
}

int hbls_decompress_pubkeys_device(const uint8_t* pks, size_t n, void* table, uint8_t* status, void* stream) {
  Dev* d;
  hipStream_t s = (hipStream_t)stream;
  if (dev_of_stream(s, &d)) return -1;
  if (n == 0) return 0;
  if (n > 0xffffffffull) return set_err("decompress pubkeys: too many keys");
  std::lock_guard<std::mutex> lk(d->mu);
  TIMED(*d, "k_dec_pk", s, launch_dec_pk(pks, (uint32_t)n, (G1AEntry*)table, status, s));
  return 0;
}

int hbls_attestation_signing_roots_device(const uint8_t* data, size_t n, const uint8_t* domains, size_t n_domains,
                                          const uint32_t* dom_idx, uint8_t* roots, void* stream) {
  Dev* d;
  hipStream_t s = (hipStream_t)stream;
  if (dev_of_stream(s, &d)) return -1;
  if (n == 0) return 0;
  if (n_domains == 0) return set_err("signing roots: no domain");
  if (n > 0xffffffffull) return set_err("signing roots: too many items");
  std::lock_guard<std::mutex> lk(d->mu);
  TIMED(*d, "k_attestation_roots", s,
        launch_attestation_roots(data, (uint32_t)n, domains, (uint32_t)n_domains, dom_idx, roots, s));
  return 0;
}

int hbls_verify_aggregate_device(const uint8_t* pks, const uint32_t* grp_off, size_t n_groups, const uint8_t* sigs,
                                 const void* hm, uint8_t* status, void* stream) {
  Dev* d;
  hipStream_t s = (hipStream_t)stream;
  if (dev_of_stream(s, &d)) return -1;
  if (n_groups == 0) return 0;
  if (check_offsets(grp_off, n_groups)) return -1;
  std::vector<uint32_t> goff(n_groups + 1);
  for (size_t g = 0; g <= n_groups; g++) goff[g] = grp_off[g] - grp_off[0];
  std::lock_guard<std::mutex> lk(d->mu);
  Ws& w = ws_acquire(*d, s);
  VaKeys keys;
  keys.dpk = pks + 48ull * grp_off[0];
  if (va_pipeline(*d, w, keys, goff[n_groups], goff.data(), n_groups, sigs, (const MsgEntry*)hm, status, s, nullptr))
    return -1;
  return ws_release(w, s);
}

int hbls_threshold_aggregate_device(const uint8_t* sigs, const int64_t* idx, const uint32_t* grp_off, size_t n_groups,
                                    size_t n_partials, uint8_t* out, uint8_t* status, void* stream) {
  Dev* d;
  hipStream_t s = (hipStream_t)stream;
  if (dev_of_stream(s, &d)) return -1;
  std::lock_guard<std::mutex> lk(d->mu);
  Ws& w = ws_acquire(*d, s);
  HmEntry* pts;
  uint8_t* mst0;
  if (wsbuf(w, W_TAPTS, n_partials, &pts) || wsbuf(w, W_TADST, n_partials, &mst0)) return -1;
  if (n_partials) TIMED(*d, "k_dec_sig_pt", s, launch_dec_sig_pt(sigs, (uint32_t)n_partials, pts, mst0, s));
  if (ta_tail(*d, w, pts, nullptr, mst0, idx, grp_off, n_groups, n_partials, 0, out, status, nullptr, s)) return -1;
  return ws_release(w, s);
}

int hbls_slot_device(const hbls_slot* a, void* stream) {
  Dev* d;
  hipStream_t s = (hipStream_t)stream;
  if (dev_of_stream(s, &d)) return -1;
  if (!a) return set_err("hbls_slot_device: null arguments");
  if (a->n_groups && !a->ta_src && !a->ta_sigs) return set_err("hbls_slot_device: ta_src or ta_sigs is required");
  if (a->dv_pks && a->n_vgroups != a->n_groups)
    return set_err("hbls_slot_device: the folded post-aggregate verification needs one verification group per "
                   "aggregation group");
  std::lock_guard<std::mutex> lk(d->mu);
  Ws& w = ws_acquire(*d, s);
  // The slot starts writing the caller's hm at once, on a side stream: the staged hashing keeps
  // its hand-over values in hm's line area (hashsplit.hip).  A caller that prepared its buffers on
  // the device's default stream (a zero fill of hm, say) and passes a non-blocking stream has not
  // ordered that work before this call; a blocking stream would have.  The call therefore runs
  // behind what the default stream holds now: one event, nothing to wait for when it is idle.
  if (s) {
    HCHK(hipEventRecord(w.ev_dflt, nullptr));
    HCHK(hipStreamWaitEvent(s, w.ev_dflt, 0));
  }
  HCHK(hipEventRecord(w.ev_fork, s));
  // messages: hash + Miller lines (side 2)
  hipStream_t sh = w.side[2];
  HCHK(hipStreamWaitEvent(sh, w.ev_fork, 0));
  const bool defer = defer_lines(a->n_vgroups, a->n_msgs);
  if (hash_messages(*d, a->msgs, a->msg_off, a->msg_len, a->n_msgs, (MsgEntry*)a->hm, sh, !defer)) return -1;
  HCHK(hipEventRecord(w.ev_side[2], sh));
  TaFold fold{};
  fold.ta_sigs = a->ta_sigs;
  fold.ta_src = a->ta_src;
  fold.ta_idx = a->ta_idx;
  fold.grp_off = a->grp_off;
  fold.n_groups = a->n_groups;
  fold.n_partials = a->n_ta_partials;
  fold.ta_out = a->ta_out;
  fold.ta_status = a->ta_status;
  fold.dv_pks = a->dv_pks;
  fold.agg_status = a->agg_vstatus;
  if ((a->pk_table != nullptr) != (a->pk_table_st != nullptr) ||
      (a->dv_pk_table != nullptr) != (a->dv_pk_table_st != nullptr))
    return set_err("hbls_slot_device: a key table needs its status array");
  fold.pk_table = (const G1AEntry*)a->pk_table;
  fold.pk_table_st = a->pk_table_st;
  fold.dv_pk_table = (const G1AEntry*)a->dv_pk_table;
  fold.dv_pk_table_st = a->dv_pk_table_st;
  VerifyCall vc;
  vc.pks = a->pks;
  vc.sigs = a->sigs;
  vc.msg_idx = a->msg_idx;
  vc.hm = (const MsgEntry*)a->hm;
  vc.n = a->n;
  vc.grp_off = a->vgrp_off;
  vc.n_groups = a->n_vgroups;
  vc.status = a->vstatus;
  vc.s = s;
  vc.device_entry = true;
  vc.hm_ready = w.ev_side[2];
  vc.fold = &fold;
  vc.defer_hm = (MsgEntry*)a->hm;
  vc.defer_msgs = defer ? a->n_msgs : 0;
  if (verify_pipeline(*d, w, vc)) return -1;
  HCHK(hipStreamWaitEvent(s, w.ev_side[2], 0));
  return ws_release(w, s);
}

// hbls_slot_device with verified-member selection: slot_select_core with ta_select
int hbls_slot_select_device(const hbls_slot* a, uint32_t threshold, uint32_t* chosen, uint32_t* ta_count,
                            void* stream) {
  Dev* d;
  hipStream_t s = (hipStream_t)stream;
  if (dev_of_stream(s, &d)) return -1;
  if (!a) return set_err("hbls_slot_select_device: null arguments");
  if (threshold == 0 || threshold > (uint32_t)TA_SMALL_MAX)
    return set_err("hbls_slot_select_device: threshold must be in 1.." + std::to_string(TA_SMALL_MAX));
  if (a->ta_sigs) return set_err("hbls_slot_select_device: ta_sigs must be NULL (the candidates are verified partials)");
  const size_t ng = a->n_groups, t = threshold;
  if (ng && (!a->ta_src || !a->ta_idx || !a->grp_off || !chosen || !ta_count || !a->ta_out || !a->ta_status))
    return set_err("hbls_slot_select_device: ta_src, ta_idx, grp_off, chosen, ta_count, ta_out and ta_status are required");
  if (ng && (!a->dv_pks || !a->agg_vstatus)) return set_err("hbls_slot_select_device: dv_pks and agg_vstatus are required");
  if (a->n >= 0xffffffffull || ng * t >= 0xffffffffull || a->n_ta_partials >= 0xffffffffull)
    return set_err("hbls_slot_select_device: too many items");
  if ((a->pk_table != nullptr) != (a->pk_table_st != nullptr) ||
      (a->dv_pk_table != nullptr) != (a->dv_pk_table_st != nullptr))
    return set_err("hbls_slot_select_device: a key table needs its status array");
  std::lock_guard<std::mutex> lk(d->mu);
  return slot_select_core(*d, s, *a, threshold, chosen, ta_count, TASEL_MODE_FIRST, true);
}

int hbls_slot_select_batch(const uint8_t* pks, const uint8_t* sigs, const uint8_t* msgs, const uint64_t* msg_off,
                           const uint32_t* msg_len, size_t n, const uint32_t* cand, const int64_t* cand_idx,
                           const uint32_t* grp_off, size_t n_groups, const uint8_t* dv_pks, uint32_t threshold,
                           uint8_t* vstatus, uint32_t* chosen, uint32_t* ta_count, uint8_t* ta_out, uint8_t* ta_status,
                           uint8_t* agg_vstatus) {
  if (ensure_init()) return -1;
  if (threshold == 0 || threshold > (uint32_t)TA_SMALL_MAX)
    return set_err("hbls_slot_select_batch: threshold must be in 1.." + std::to_string(TA_SMALL_MAX));
  if (n >= 0xffffffffull || n_groups >= 0xffffffffull || n_groups * threshold >= 0xffffffffull)
    return set_err("hbls_slot_select_batch: too many items");
  if (n && (!pks || !sigs || !msg_off || !msg_len || !vstatus))
    return set_err("hbls_slot_select_batch: pks, sigs, msg_off, msg_len and vstatus are required");
  if (msgs_missing(msgs, msg_len, n)) return set_err("hbls_slot_select_batch: msgs is required");
  if (n_groups && (!grp_off || !dv_pks || !chosen || !ta_count || !ta_out || !ta_status || !agg_vstatus))
    return set_err("hbls_slot_select_batch: grp_off, dv_pks, chosen, ta_count, ta_out, ta_status and agg_vstatus are required");
  static const uint32_t no_groups[1] = {0};
  if (!n_groups) grp_off = no_groups;
  for (size_t g = 0; g < n_groups; g++)
    if (grp_off[g + 1] < grp_off[g]) return set_err("hbls_slot_select_batch: grp_off must be non-decreasing");
  if (grp_off[n_groups] > grp_off[0] && (!cand || !cand_idx))
    return set_err("hbls_slot_select_batch: cand and cand_idx are required");
  if (n == 0 && n_groups == 0) return 0;
  return slot_select_host(pks, sigs, msgs, msg_off, msg_len, n, cand, cand_idx, grp_off, n_groups, dv_pks, threshold,
                          vstatus, chosen, ta_count, ta_out, ta_status, agg_vstatus);
}

// Cumulative per-process counters of hbls_slot_select_device over the devices of the mask, reset by
// reading: out[0] groups seen, out[1] groups with fewer than `threshold` members, out[2] groups whose
// members are not their first `threshold` candidates, out[3] groups the small-scalar path aggregated
// (n <= 4).  Waits for the devices' work.
int hbls_slot_select_stats(uint64_t* out, size_t n) {
  if (ensure_init()) return -1;
  if (!out || n > (size_t)SEL_COUNTERS) return set_err("hbls_slot_select_stats: out is null or n above 4");
  for (size_t k = 0; k < n; k++) out[k] = 0;
  for (Dev* d : devs()) {
    std::lock_guard<std::mutex> lk(d->mu);
    if (!d->sel_ctr.p) continue;
    HCHK(hipSetDevice(d->ord));
    // the counting kernels run on the callers' streams, which the library does not know: the device
    HCHK(hipDeviceSynchronize());
    uint64_t c[SEL_COUNTERS];
    HCHK(hipMemcpy(c, d->sel_ctr.p, sizeof(c), hipMemcpyDeviceToHost));
    HCHK(hipMemset(d->sel_ctr.p, 0, sizeof(c)));
    HCHK(hipDeviceSynchronize());
    for (size_t k = 0; k < n; k++) out[k] += c[k];
  }
  return 0;
}

int hbls_duty_open(const uint8_t* dv_pks, size_t n_groups, uint32_t threshold, uint32_t max_stored, uint64_t* duty) {
  if (ensure_init() || duty_open_check("hbls_duty_open", duty, threshold, max_stored)) return -1;
  if (n_groups && !dv_pks) return set_err("hbls_duty_open: dv_pks is required");
  if (n_groups >= 0xffffffffull / DUTY_MAX_STORED) return set_err("hbls_duty_open: too many groups");
  return duty_open(dv_pks, n_groups, threshold, max_stored, duty);
}

// hbls_duty_add, hbls_duty_add_sets and hbls_duty_add_sets_first: one argument check, in the order the
// first failing one is reported in, one call.  sets: null for hbls_duty_add (its set ids are filled here)
static int duty_add_entry(uint64_t duty, DutyAddArgs a, DutySetCall* sets) {
  const std::string who = a.who;
  const size_t n = a.n;
  if (ensure_init()) return -1;
  std::shared_ptr<Duty> du = duty_get(who, duty);
  if (!du) return -1;
  std::lock_guard<std::mutex> l(du->mu);
  if (du->closed) return set_err(who + ": the duty is closed");
  if (du->broken) return set_err(who + ": an earlier add failed on a device; close the duty");
  if (!a.first_serial || !a.n_fired) return set_err(who + ": first_serial and n_fired are required");
  if (n >= 0xffffffffull - du->next_serial) return set_err(who + ": the duty would reach 2^32 - 1 partials");
  if (sets) {
    if (sets->n_sets >= 0xffffffffull) return set_err(who + ": too many sets");
    if (sets->n_sets && !a.set_first) return set_err(who + ": set_first is required");
    if (const char* bad = duty_check_sets(sets->set_off, sets->n_sets, n)) return set_err(who + ": " + bad);
  }
  if (du->cl) {  // a cluster duty resolves the keys itself: a caller that passes some mixes the two kinds of duty
    if (a.pks) return set_err(who + ": pks must be NULL on a cluster duty (the keys are the cluster's)");
    if (n && (!a.sigs || !a.msg_off || !a.msg_len || !a.group || !a.share_idx || !a.vstatus || !a.stored))
      return set_err(who + ": sigs, msg_off, msg_len, group, share_idx, vstatus and stored are required");
  } else if (n && (!a.pks || !a.sigs || !a.msg_off || !a.msg_len || !a.group || !a.share_idx || !a.vstatus || !a.stored))
    return set_err(who + ": pks, sigs, msg_off, msg_len, group, share_idx, vstatus and stored are required");
  if (msgs_missing(a.msgs, a.msg_len, n)) return set_err(who + ": msgs is required");
  if (std::min(n, du->n_groups) && (!a.fired || !a.chosen || !a.ta_out || !a.ta_status || !a.agg_vstatus))
    return set_err(who + ": fired, chosen, ta_out, ta_status and agg_vstatus are required");
  *a.first_serial = du->next_serial;
  *a.n_fired = 0;
  if (!n) {
    if (sets) {  // empty sets only: seen, none rejected
      for (size_t k = 0; k < sets->n_sets; k++) a.set_first[k] = DUTY_NONE;
      du->set_stats[0] += sets->n_sets;
    }
    return 0;
  }
  if (sets) duty_set_ids(sets->set_off, sets->n_sets, n, sets->set_of);
  a.sets = sets;
  return duty_add(*du, a);
}

int hbls_duty_add(uint64_t duty, const uint8_t* pks, const uint8_t* sigs, const uint8_t* msgs, const uint64_t* msg_off,
                  const uint32_t* msg_len, const uint32_t* group, const int64_t* share_idx, size_t n, uint8_t* vstatus,
                  uint8_t* stored, uint32_t* first_serial, uint32_t* fired, size_t* n_fired, uint32_t* chosen,
                  uint8_t* ta_out, uint8_t* ta_status, uint8_t* agg_vstatus) {
  return duty_add_entry(duty, {pks, sigs, msgs, msg_off, msg_len, group, share_idx, n, vstatus, stored, first_serial, fired,
                               n_fired, chosen, ta_out, ta_status, agg_vstatus, "hbls_duty_add"}, nullptr);
}

int hbls_duty_add_sets(uint64_t duty, const uint8_t* pks, const uint8_t* sigs, const uint8_t* msgs, const uint64_t* msg_off,
                       const uint32_t* msg_len, const uint32_t* group, const int64_t* share_idx, size_t n,
                       const uint32_t* set_off, size_t n_sets, uint8_t* vstatus, uint8_t* stored, uint32_t* first_serial,
                       uint32_t* set_first, uint32_t* fired, size_t* n_fired, uint32_t* chosen, uint8_t* ta_out,
                       uint8_t* ta_status, uint8_t* agg_vstatus) {
  DutySetCall sc{set_off, n_sets, {}, false};
  return duty_add_entry(duty, {pks, sigs, msgs, msg_off, msg_len, group, share_idx, n, vstatus, stored, first_serial, fired,
                               n_fired, chosen, ta_out, ta_status, agg_vstatus, "hbls_duty_add_sets", nullptr, set_first}, &sc);
}

int hbls_duty_add_sets_first(uint64_t duty, const uint8_t* pks, const uint8_t* sigs, const uint8_t* msgs,
                             const uint64_t* msg_off, const uint32_t* msg_len, const uint32_t* group,
                             const int64_t* share_idx, size_t n, const uint32_t* set_off, size_t n_sets, uint8_t* vstatus,
                             uint8_t* stored, uint32_t* first_serial, uint32_t* set_first, uint32_t* fired, size_t* n_fired,
                             uint32_t* chosen, uint8_t* ta_out, uint8_t* ta_status, uint8_t* agg_vstatus) {
  DutySetCall sc{set_off, n_sets, {}, true};
  return duty_add_entry(duty, {pks, sigs, msgs, msg_off, msg_len, group, share_idx, n, vstatus, stored, first_serial, fired,
                               n_fired, chosen, ta_out, ta_status, agg_vstatus, "hbls_duty_add_sets_first", nullptr, set_first}, &sc);
}

int hbls_duty_first_stats(uint64_t duty, uint64_t* out, size_t n) {
  return duty_counters("hbls_duty_first_stats", duty, &Duty::first_stats, out, n);
}

int hbls_duty_set_stats(uint64_t duty, uint64_t* out, size_t n) {
  return duty_counters("hbls_duty_set_stats", duty, &Duty::set_stats, out, n);
}

int hbls_duty_state(uint64_t duty, uint32_t* stored_count, uint8_t* fired_flag) {
  if (ensure_init()) return -1;
  std::shared_ptr<Duty> du = duty_get("hbls_duty_state", duty);
  if (!du) return -1;
  std::lock_guard<std::mutex> l(du->mu);
  if (du->closed) return set_err("hbls_duty_state: the duty is closed");
  if (du->n_groups && (!stored_count || !fired_flag)) return set_err("hbls_duty_state: stored_count and fired_flag are required");
  return duty_state(*du, stored_count, fired_flag);
}

int hbls_duty_stats(uint64_t duty, uint64_t* out, size_t n) {
  return duty_counters("hbls_duty_stats", duty, &Duty::stats, out, n);
}

int hbls_duty_close(uint64_t duty) {
  if (ensure_init()) return -1;
  std::shared_ptr<Duty> du = duty_get("hbls_duty_close", duty, true);
  if (!du) return -1;
  std::lock_guard<std::mutex> l(du->mu);  // behind the duty's call in flight, if any
  du->closed = true;
  for (DutyShard& s : du->sh) duty_free_shard(s);
  du->cl.reset();  // a cluster duty: the last duty of a closed cluster frees the keys (no device lock is held here)
  return 0;
}

int hbls_cluster_open(const uint8_t* dv_pks, const uint8_t* pubshares, size_t n_validators, uint32_t n_shares,
                      uint32_t ladder_tables, uint8_t* key_status, uint64_t* cluster) {
  if (ensure_init()) return -1;
  if (!cluster) return set_err("hbls_cluster_open: cluster is required");
  if (n_shares < 1 || n_shares > CLUSTER_MAX_SHARES)
    return set_err("hbls_cluster_open: n_shares must be in 1.." + std::to_string(CLUSTER_MAX_SHARES));
  if (ladder_tables > 1) return set_err("hbls_cluster_open: ladder_tables must be 0 or 1");
  if (n_validators && (!dv_pks || !pubshares)) return set_err("hbls_cluster_open: dv_pks and pubshares are required");
  // n_validators (1 + n_shares) < 2^32 - 1: a key's number is a uint32 entry number of the ladder-table
  // path (KeyWideRef::ent), and KEY_WIDE_NONE is no key's
  if (n_validators > 0xfffffffeull / (1 + (uint64_t)n_shares)) return set_err("hbls_cluster_open: too many keys");
  return cluster_open(dv_pks, pubshares, n_validators, n_shares, ladder_tables != 0, key_status, cluster);
}

int hbls_cluster_close(uint64_t cluster) {
  if (ensure_init()) return -1;
  return cluster_get("hbls_cluster_close", cluster, true) ? 0 : -1;  // (the keys go here unless a duty still holds them)
}

int hbls_cluster_stats(uint64_t cluster, uint64_t* out, size_t n) {
  return cluster_counters("hbls_cluster_stats", cluster, &Cluster::stats, out, n);
}

int hbls_cluster_check(uint64_t cluster, uint32_t threshold, uint8_t* row_status, uint64_t* row_windows, size_t* n_bad) {
  if (ensure_init()) return -1;
  std::shared_ptr<Cluster> cl = cluster_get("hbls_cluster_check", cluster);
  if (!cl) return -1;
  LockPlan plan;
  if (!lock_plan(cl->n_shares, threshold, plan))
    return set_err("hbls_cluster_check: threshold must be in 1.." + std::to_string(cl->n_shares) + " (the cluster's n_shares)");
  if (cl->n_validators && !row_status) return set_err("hbls_cluster_check: row_status is required");
  return cluster_check(*cl, plan, row_status, row_windows, n_bad);
}

int hbls_cluster_check_stats(uint64_t cluster, uint64_t* out, size_t n) {
  return cluster_counters("hbls_cluster_check_stats", cluster, &Cluster::check_stats, out, n);
}

int hbls_cluster_verify_batch(uint64_t cluster, const uint32_t* group, const int64_t* key_idx, const uint8_t* sigs,
                              const uint8_t* msgs, const uint64_t* msg_off, const uint32_t* msg_len, size_t n,
                              uint8_t* status) {
  if (ensure_init()) return -1;
  std::shared_ptr<Cluster> cl = cluster_get("hbls_cluster_verify_batch", cluster);
  if (!cl) return -1;
  if (n >= 0xffffffffull) return set_err("hbls_cluster_verify_batch: too many items");
  if (n && (!group || !key_idx || !sigs || !msg_off || !msg_len || !status))
    return set_err("hbls_cluster_verify_batch: group, key_idx, sigs, msg_off, msg_len and status are required");
  if (msgs_missing(msgs, msg_len, n))
    return set_err("hbls_cluster_verify_batch: msgs is required (an item has a message of non-zero length)");
  return cluster_verify_batch(*cl, {group, key_idx, sigs, msgs, msg_off, msg_len, n, status});
}

int hbls_cluster_verify_aggregate(uint64_t cluster, uint64_t share_mask, uint32_t with_dv, const uint8_t* sig,
                                  const uint8_t* msg, uint32_t msg_len, uint8_t* status) {
  if (ensure_init()) return -1;
  std::shared_ptr<Cluster> cl = cluster_get("hbls_cluster_verify_aggregate", cluster);
  if (!cl) return -1;
  if (!cluster_sel_valid(share_mask, with_dv, cl->n_shares))
    return set_err("hbls_cluster_verify_aggregate: share_mask has a bit at or above the cluster's n_shares (" +
                   std::to_string(cl->n_shares) + "), or with_dv is above 1");
  if (!sig || !status || (msg_len && !msg)) return set_err("hbls_cluster_verify_aggregate: sig, status and msg are required");
  return cluster_verify_aggregate(*cl, share_mask, with_dv, sig, msg, msg_len, status);
}

int hbls_cluster_verify_stats(uint64_t cluster, uint64_t* out, size_t n) {
  return cluster_counters("hbls_cluster_verify_stats", cluster, &Cluster::verify_stats, out, n);
}

int hbls_duty_open_cluster(uint64_t cluster, uint32_t threshold, uint32_t max_stored, uint64_t* duty) {
  if (ensure_init() || duty_open_check("hbls_duty_open_cluster", duty, threshold, max_stored)) return -1;
  std::shared_ptr<Cluster> cl = cluster_get("hbls_duty_open_cluster", cluster);
  if (!cl) return -1;
  if (cl->n_validators >= 0xffffffffull / DUTY_MAX_STORED) return set_err("hbls_duty_open_cluster: too many groups");
  return duty_open(nullptr, cl->n_validators, threshold, max_stored, duty, cl);
}

int hbls_timing(int enable) {
  if (ensure_init()) return -1;
  for (Dev* d : devs()) {
    std::lock_guard<std::mutex> lk(d->mu);
    d->timing = enable != 0;
    d->serial = enable == 2;
    d->tev_used = 0;
  }
  return 0;
}

// Launch durations recorded since hbls_timing(1), in launch order over the devices of the mask:
// names[i] (kernel name, static storage) and ms[i].
int hbls_timing_read(const char** names, float* ms, size_t max_n, size_t* n_out) {
  if (ensure_init()) return -1;
  size_t k = 0;
  for (Dev* d : devs()) {
    std::lock_guard<std::mutex> lk(d->mu);
    HCHK(hipSetDevice(d->ord));
    for (size_t i = 0; i < d->tev_used && k < max_n; i++, k++) {
      HCHK(hipEventSynchronize(d->tev[i].b));
      HCHK(hipEventElapsedTime(&ms[k], d->tev[i].a, d->tev[i].b));
      if (names) names[k] = d->tev[i].name;
    }
  }
  *n_out = k;
  return 0;
}

int hbls_stats(uint64_t* out, size_t n) {
  for (size_t k = 0; k < n && k < 8; k++) out[k] = g_stats[k].load();
  return stats_on() ? 0 : set_err("statistics are collected only with HBLS_STATS=1");
}

size_t hbls_fe_batch(size_t min_groups) { return g_fe_batch_min.exchange(min_groups); }
int hbls_adaptive(int on) { return g_adaptive.exchange(on != 0) ? 1 : 0; }
// the latency-path layouts by name (tests switch between them within one process)
int hbls_tune(const char* name, size_t value, size_t* previous) {
  if (ensure_init()) return -1;
  if (!name) return set_err("hbls_tune: no name");
  static const std::pair<const char*, std::atomic<size_t>*> knobs[] = {
      {"HBLS_HASH_PAIR_MAX", &g_hash_pair_max}, {"HBLS_HASH_ONE_LANE", &g_hash_one_lane},
      {"HBLS_HASH_SPLIT", &g_hash_split},       {"HBLS_FE18_MAX", &g_fe18_max},
      {"HBLS_TA_PAIR_MAX", &g_ta_pair_max},     {"HBLS_DEC_PAIR_MAX", &g_dec_pair_max},
      // chunking of large verifications (tests run them at small sizes: several chunks per call)
      {"HBLS_GROUP_CHUNK", &g_gcap},            {"HBLS_FALLBACK_CHUNK", &g_fbcap},
      {"HBLS_GROUP_MAX", &g_gmax}};
  if (strcmp(name, "HBLS_KEY_LEARN") == 0) {  // a new capacity starts from an empty table (0: freed)
    value = std::min(value, KEY_LEARN_MAX);
    const size_t old = g_key_learn.exchange(value);
    if (previous) *previous = old;
    if (old != value)
      for (Dev* d : devs()) {
        std::lock_guard<std::mutex> lk(d->mu);
        if (kl_reset(*d, value == 0)) return -1;
      }
    return 0;
  }
  if (strcmp(name, "HBLS_KEY_WIDE") == 0) {  // likewise: the tables are built as keys are learned (0: freed)
    value = std::min(value, KEY_LEARN_MAX);
    const size_t old = g_key_wide.exchange(value);
    if (previous) *previous = old;
    if (old != value)
      for (Dev* d : devs()) {
        std::lock_guard<std::mutex> lk(d->mu);
        if (kl_reset(*d, false)) return -1;
        if (value == 0 && d->kl_wide.p) {
          HCHK(hipSetDevice(d->ord));
          HCHK(hipFree(d->kl_wide.p));
          d->kl_wide = DevBuf{};
        }
      }
    return 0;
  }
  for (const auto& k : knobs)
    if (strcmp(k.first, name) == 0) {
      const size_t old = k.second->exchange(value);
      if (previous) *previous = old;
      return 0;
    }
  return set_err(std::string("hbls_tune: unknown setting ") + name);
}
size_t hbls_dec_pair_max(size_t items) {
  if (ensure_init()) return 0;
  return g_dec_pair_max.exchange(items);
}
size_t hbls_single_max(size_t items) {
  if (ensure_init()) return 0;
  return g_single_max.exchange(items);
}
size_t hbls_slot_msm(size_t min_items) {
  // a new setting starts from a clean history (tests count the slot-wide checks that ran)
  for (Dev* d : devs()) {
    std::lock_guard<std::mutex> lk(d->mu);
    for (; d->res_tail != d->res_head; d->res_tail++) (void)hipEventSynchronize(d->res_ev[d->res_tail % N_RES]);
    d->attack = false;
  }
  return g_slot_msm_min.exchange(min_items);
}
size_t hbls_subgroup_batch(size_t min_items) {
  // a new setting starts from a clean history (tests count the batched tests that ran)
  for (Dev* d : devs()) {
    std::lock_guard<std::mutex> lk(d->mu);
    for (; d->sres_tail != d->sres_head; d->sres_tail++) (void)hipEventSynchronize(d->sres_ev[d->sres_tail % N_RES]);
    d->subg_failed = false;
  }
  return g_subg_batch_min.exchange(min_items);
}
size_t hbls_ta_joint(size_t members) { return g_ta_joint.exchange(std::min<size_t>(members, 8)); }
size_t hbls_rlc_lanes(size_t lanes) { return g_rlc_lanes.exchange(lanes ? lanes : 65536); }

int hbls_sync(void* stream) {
  HCHK(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}

int hbls_status_bitmap(const uint8_t* status, size_t n, uint8_t* bits, void* stream) {
  Dev* d;
  hipStream_t s = (hipStream_t)stream;
  if (dev_of_stream(s, &d)) return -1;
  if (n > 0xffffffffull) return set_err("status bitmap: too many items");
  LAUNCH(k_status_bitmap, n, s, status, (uint32_t)n, bits);
  return 0;
}

// ---- RCCL exchange between processes (one GPU each) ----
size_t hbls_comm_id_bytes(void) { return sizeof(ncclUniqueId); }

int hbls_comm_unique_id(uint8_t* id) {
  ncclUniqueId u;
  NCHK(ncclGetUniqueId(&u));
  memcpy(id, &u, sizeof(u));
  return 0;
}

int hbls_comm_init(int nranks, int rank, const uint8_t* id) {
  if (ensure_init()) return -1;
  const std::vector<Dev*> ds = devs();
  if (ds.size() != 1) return set_err("hbls_comm_init: one device per process");
  if (g_comm) return g_comm_ranks == nranks ? 0 : set_err("communicator already initialised");
  HCHK(hipSetDevice(ds[0]->ord));
  ncclUniqueId u;
  memcpy(&u, id, sizeof(u));
  NCHK(ncclCommInitRank(&g_comm, nranks, u, rank));
  g_comm_ranks = nranks;
  return 0;
}

int hbls_allgather_device(const void* send, void* recv, size_t bytes, void* stream) {
  if (!g_comm) return set_err("hbls_allgather_device: no communicator (hbls_comm_init)");
  NCHK(ncclAllGather(send, recv, bytes, ncclUint8, g_comm, (hipStream_t)stream));
  return 0;
}

int hbls_comm_size(void) {
  if (!g_comm) return 0;
  int n = 0;
  if (ncclCommCount(g_comm, &n) != ncclSuccess) return -1;
  return n;
}

int hbls_comm_destroy(void) {
  if (g_comm) NCHK(ncclCommDestroy(g_comm));
  g_comm = nullptr;
  g_comm_ranks = 0;
  return 0;
}

}  // extern "C"
