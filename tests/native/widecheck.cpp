// TEST-ONLY harness (tests/test_key_wide_host.py): the ladder tables of learned keys compiled for
// the host CPU, as hostcheck.cpp does for the rest of the kernels' arithmetic -- ec28.h's table
// builder (vbatch.hip k_pk_wide) and both ladders through the tables (k_rlc_msm<1, 2>'s chunk
// ladder, k_rlc<1>'s one-item form), beside the per-slot table and 32-step chunk ladder they
// replace.  Points go in and out compressed; the test compares with the Python oracle's group law.
// The product library never loads this; it is not a fallback.
#include "../../charon_amd/csrc/ops.h"
#include "../../charon_amd/csrc/rlc.h"
#include <string.h>

using namespace hb;

namespace {
struct Pair {
  uint32_t x, y;
};
constexpr int MAX_K = 64;
}  // namespace

extern "C" {

const char* wc_build_id() { return WC_BUILD_ID; }

// the 15 entries of the key's table, compressed (48 bytes each, entry d - 1 at out[48 (d - 1)])
int wc_table(const uint8_t* pk48, uint8_t* out) {
  G1A p;
  if (g1_decompress(p, pk48, false)) return 1;
  G1WidePt t[KEY_WIDE_PTS];
  g1_wide_build(p, t);
  for (uint32_t d = 0; d < KEY_WIDE_PTS; d++) g1_compress(out + 48 * d, G1A{t[d].x, t[d].y, false});
  return 0;
}

// sum over k items of [a_i + b_i lambda] pk_i through the tables (one table per item, in item
// order: entry number i), compressed
int wc_chunk_wide(int k, const uint8_t* pks, const uint32_t* ab, uint8_t* out48) {
  static G1WidePt wide[MAX_K * KEY_WIDE_PTS];
  uint32_t ent[MAX_K];
  Pair coef[MAX_K];
  if (k < 1 || k > MAX_K) return 1;
  for (int i = 0; i < k; i++) {
    G1A p;
    if (g1_decompress(p, pks + 48 * i, false)) return 1;  // (no subgroup check: the test gives points of G1)
    g1_wide_build(p, wide + KEY_WIDE_PTS * i);
    ent[i] = (uint32_t)i;
    coef[i] = {ab[2 * i], ab[2 * i + 1]};
  }
  g1_compress(out48, jac_to_aff(g1l_msm_ladder_wide(wide, ent, coef, 0, (uint32_t)k)));
  return 0;
}

// the same sum through the per-slot table and the 32-step ladder (vbatch.hip rlc_tab_g1's points:
// P, phi(P), P + phi(P) affine)
int wc_chunk_narrow(int k, const uint8_t* pks, const uint32_t* ab, uint8_t* out48) {
  static G1J tab[3 * MAX_K];
  Pair coef[MAX_K];
  if (k < 1 || k > MAX_K) return 1;
  for (int i = 0; i < k; i++) {
    G1A p;
    if (g1_decompress(p, pks + 48 * i, false)) return 1;  // (no subgroup check: the test gives points of G1)
    const G1A p2 = {fp_mul(p.x, fp_from_const(G1_BETA)), p.y, false};
    const G1A p3 = jac_to_aff(jac_add_aff(jac_from_aff(p), p2));
    tab[3 * i] = jac_from_aff(p);
    tab[3 * i + 1] = jac_from_aff(p2);
    tab[3 * i + 2] = jac_from_aff(p3);
    coef[i] = {ab[2 * i], ab[2 * i + 1]};
  }
  g1_compress(out48, jac_to_aff(g1l_msm_ladder(tab, coef, 0, (uint32_t)k)));
  return 0;
}

// [a + b lambda] pk through its table, the one-item ladder
int wc_item_wide(const uint8_t* pk48, uint32_t a, uint32_t b, uint8_t* out48) {
  G1A p;
  if (g1_decompress(p, pk48, false)) return 1;
  G1WidePt t[KEY_WIDE_PTS];
  g1_wide_build(p, t);
  g1_compress(out48, jac_to_aff(g1l_mul_wide(t, a, b)));
  return 0;
}

}  // extern "C"
