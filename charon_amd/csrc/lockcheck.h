// The rule of hbls_cluster_check: do a validator's pubshares interpolate to its DV key.  Row g of a
// cluster is P_0 (the DV key, node 0) followed by P_1 .. P_n (the pubshares, nodes 1 .. n): n + 1
// points of G1 (cyclic, of prime order r far above n) on the consecutive nodes 0 .. n.  The row lies on
// a polynomial of degree < t in the exponent iff every t-th forward difference vanishes,
//     D_k = sum_{i = 0 .. t} (-1)^(t - i) C(t, i) P_{k + i} = O        for k = 0 .. n - t,
// W = n - t + 1 windows: the sequences on n + 1 consecutive nodes with every D_k = O form a space of
// dimension exactly t, which the polynomials of degree < t fill (no false accept), and the difference
// operator annihilates those (no false reject).  The scalars are signed binomials: C(64, 32) < 2^63, so
// for every allowed t <= 64 they fit a signed 64-bit word, and no Fr arithmetic is needed anywhere.
//
// ONE function holds the coefficients and the plan built on them.  No HIP in here: lockcheck.hip's
// launcher hands the plan to k_lock_check as its argument, hipbls.hip validates a call's threshold
// with it, and the CPU harness tests/native/lockcheckhost.cpp compiles the same functions for
// tests/test_lock_check_host.py.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LOCKCHECK_HD __host__ __device__ inline
#else
#define LOCKCHECK_HD inline
#endif

namespace hb {

constexpr uint32_t LOCK_MAX_T = 64;  // cluster.h CLUSTER_MAX_SHARES: a threshold is at most n_shares

// c[i] = (-1)^(t - i) C(t, i) for i = 0 .. t (c: t + 1 words).  False, with nothing written, unless
// 1 <= t <= LOCK_MAX_T.  Pascal's rule in place: every intermediate value is a binomial of a row
// <= t, so nothing exceeds C(64, 32).
LOCKCHECK_HD bool lock_coeffs(uint32_t t, int64_t* c) {
  if (t < 1 || t > LOCK_MAX_T) return false;
  c[0] = 1;
  for (uint32_t row = 1; row <= t; row++) {
    c[row] = 1;
    for (uint32_t i = row - 1; i >= 1; i--) c[i] += c[i - 1];
  }
  for (uint32_t i = 0; i <= t; i++)
    if ((t - i) & 1) c[i] = -c[i];
  return true;
}

// The common bit length of a threshold's coefficients: that of the largest magnitude, C(t, t / 2);
// 0 when the threshold is refused.
LOCKCHECK_HD uint32_t lock_bits(uint32_t t) {
  int64_t c[LOCK_MAX_T + 1];
  if (!lock_coeffs(t, c)) return 0;
  uint64_t m = (uint64_t)(c[t / 2] < 0 ? -c[t / 2] : c[t / 2]);
  uint32_t b = 0;
  for (; m; m >>= 1) b++;
  return b;
}

// What k_lock_check consumes, the same for every lane of a launch (so the coefficient bits are
// wave-uniform): lane = row * windows + k computes D_k of its row from the row's entries k .. k + t.
struct LockPlan {
  uint32_t n_shares;  // a row holds 1 + n_shares keys
  uint32_t t;
  uint32_t windows;   // n_shares - t + 1 <= 64: a row's verdicts fit one 64-bit mask
  uint32_t bits;      // lock_bits(t): the bit planes of the joint ladder
  int64_t c[LOCK_MAX_T + 1];
};

// The plan of (n_shares, t).  False, with nothing written, unless 1 <= t <= n_shares <= LOCK_MAX_T.
LOCKCHECK_HD bool lock_plan(uint32_t n_shares, uint32_t t, LockPlan& p) {
  if (t < 1 || t > n_shares || n_shares > LOCK_MAX_T) return false;
  p.n_shares = n_shares;
  p.t = t;
  p.windows = n_shares - t + 1;
  p.bits = lock_bits(t);
  for (uint32_t i = 0; i <= LOCK_MAX_T; i++) p.c[i] = 0;
  return lock_coeffs(t, p.c);
}

}  // namespace hb
