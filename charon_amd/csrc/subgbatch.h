// The batched G2 subgroup test of large calls (msm.hip k_subg_*): the digits of an item, and the
// map between a window value and its base-13 digits.  Host and device (tests/native/subgcheck.cpp
// compiles it with g++).
//
// Every checked signature enters SG_WINDOWS bucket sums; a window value d < 13^4 is read as
// SG_DIGITS base-13 digits, so the 5 x 4 = 20 weighted sums S_(w,j) = sum_d digit_j(d) B_(w,d) are
// 20 random combinations sum_i c_i Q_i with every coefficient c_i in [0, 12].  psi - [x] is a
// homomorphism of E'(Fp2) with kernel G2, so S_(w,j) is in G2 exactly when sum_i c_i T_i = 0 for the
// items' components T_i in the cofactor group; the smallest prime of the cofactor is 13 > 12, so a
// nonzero T_i passes a test for at most one value of its digit.
#pragma once
#include "sha256.h"

namespace hb {

constexpr uint32_t SG_BASE = 13, SG_DIGITS = 4, SG_WINDOWS = 5;
constexpr uint32_t SG_RANGE = SG_BASE * SG_BASE * SG_BASE * SG_BASE;  // 28 561 window values
constexpr uint32_t SG_KEYS = SG_WINDOWS * SG_RANGE;                   // buckets (window, value); value 0 unused
constexpr uint32_t SG_SUMS = SG_WINDOWS * SG_DIGITS;                  // the weighted sums tested
constexpr uint32_t SG_CLASSES = SG_SUMS * (SG_BASE - 1);              // (window, digit place, digit value 1..12)
constexpr uint32_t SG_CLASS_SIZE = SG_RANGE / SG_BASE;                // window values with one digit fixed
// the domain word of the digits' hash block: rlc_coeffs / rlc_digits (vbatch.hip) hash key || item
// with word 9 = 0x80000000 (the padding bit right behind the item); here word 9 is this constant
// and the padding follows it, so the block is one no coefficient is ever drawn from
constexpr uint32_t SG_DOMAIN = 0x53554247u;  // "SUBG"

// a uniform 32-bit word to a window value: floor(u * 13^4 / 2^32); each value has at most
// ceil(2^32 / 13^4) preimages
HD uint32_t sg_window(uint32_t u) { return (uint32_t)(((uint64_t)u * SG_RANGE) >> 32); }

// digit j (0 = least significant) of a window value
HD uint32_t sg_digit(uint32_t d, uint32_t j) {
  HB_NOUNROLL for (uint32_t k = 0; k < j; k++) d /= SG_BASE;
  return d % SG_BASE;
}

// the m-th (m < SG_CLASS_SIZE) window value whose digit j is c: m's three base-13 digits around c
HD uint32_t sg_class_member(uint32_t j, uint32_t c, uint32_t m) {
  uint32_t pw = 1;
  HB_NOUNROLL for (uint32_t k = 0; k < j; k++) pw *= SG_BASE;
  const uint32_t lo = m % pw, hi = m / pw;
  return lo + c * pw + hi * pw * SG_BASE;
}

// the SG_WINDOWS window values of entry `item` under the call's key (8 words)
HD void sg_windows(const uint32_t* key, uint32_t item, uint32_t* d) {
  uint32_t w[16];
  HB_UNROLL for (int j = 0; j < 8; j++) w[j] = key[j];
  w[8] = item;
  w[9] = SG_DOMAIN;
  w[10] = 0x80000000u;
  HB_UNROLL for (int j = 11; j < 15; j++) w[j] = 0;
  w[15] = 40 * 8;
  Sha256State st = sha256_init();
  sha256_compress(st, w);
  HB_UNROLL for (uint32_t k = 0; k < SG_WINDOWS; k++) d[k] = sg_window(st.h[k]);
}

}  // namespace hb
