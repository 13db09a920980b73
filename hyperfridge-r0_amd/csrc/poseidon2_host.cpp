// Poseidon2 on the host (BabyBear, t=24, x^7, 4+21+4 rounds): the tables a context uploads (fill_p2), the round-by-round permutation
// the transcript and the verifier use, and the sponge laid out for the in-circuit hash.  Host only and free of the HIP runtime, so the
// sanitizer checks compile it as it is (tools/fuzz/run_p2_dot_check.sh).
#include "../../include/r0hip_poseidon2_consts.h"
#include "internal.hpp"
#include "poseidon2_dot_schedule.hpp"

namespace r0h {

bool fill_p2(P2Consts& k, const uint32_t* rc, const uint32_t* diag) {
  int fr = 0, pr = 0;
  for (int r = 0; r < P2_ROUNDS; r++) {
    bool full = r < P2_HALF_FULL || r >= P2_HALF_FULL + P2_PARTIAL;
    if (full) {
      for (int i = 0; i < P2_CELLS; i++) k.rc_full[fr][i] = enc(rc[r * P2_CELLS + i]);
      fr++;
    } else {
      k.rc_partial[pr++] = enc(rc[r * P2_CELLS]);
    }
  }
  for (int i = 0; i < P2_CELLS; i++) {
    k.diag[i] = enc(diag[i]);
    k.diag_canon[i] = diag[i];
    k.diag_shoup[i] = shoup_companion(diag[i]);
  }
  // tables of the deferred partial rounds: powers of the diagonal and their lane sums (canonical arithmetic, then encoded)
  uint32_t pw[P2_PARTIAL + 1][P2_CELLS], kappa[P2_PARTIAL + 1];
  for (int e = 0; e <= P2_PARTIAL; e++) {
    uint64_t ks = 0;
    for (int i = 1; i < P2_CELLS; i++) {
      pw[e][i] = e == 0 ? 1u : (uint32_t)((uint64_t)pw[e - 1][i] * diag[i] % P);
      ks += pw[e][i];
    }
    kappa[e] = (uint32_t)(ks % P);
  }
  uint32_t* w = k.part_sigma;
  for (int r = 1; r < P2_PARTIAL; r++) {
    for (int i = 1; i < P2_CELLS; i++) *w++ = enc(pw[r][i]);
    for (int j = 0; j < r; j++) *w++ = enc(kappa[r - 1 - j]);
  }
  w = k.part_final;
  for (int i = 1; i < P2_CELLS; i++)
    for (int e = P2_PARTIAL; e >= 0; e--) *w++ = enc(pw[e][i]);
  // the schedule compiled into the kernels against the words that now stand in the table, not against the diagonal they came from
  return p2_dot_schedule_covers(P2_DOT_TIGHT, k.part_sigma, k.part_final);
}
const P2Consts& p2_default() {
  static const P2Consts k = [] { P2Consts t; fill_p2(t, R0H_P2_ROUND_CONSTANTS, R0H_P2_INT_DIAG_M1); return t; }();
  return k;
}

static inline uint32_t sbox7(uint32_t x) {
  uint32_t x2 = mul(x, x), x4 = mul(x2, x2);
  return mul(mul(x4, x2), x);
}
static void m_ext_host(uint32_t* c) {
  uint32_t col[4] = {0, 0, 0, 0};
  for (int k = 0; k < P2_CELLS; k += 4) {
    uint32_t a = c[k], b = c[k + 1], d = c[k + 2], e = c[k + 3];
    uint32_t t0 = add(a, b), t1 = add(d, e);
    uint32_t t2 = add(add(b, b), t1), t3 = add(add(e, e), t0);
    uint32_t t4 = add(add(add(t1, t1), add(t1, t1)), t3), t5 = add(add(add(t0, t0), add(t0, t0)), t2);
    c[k] = add(t3, t5); c[k + 1] = t5; c[k + 2] = add(t2, t4); c[k + 3] = t4;
    for (int j = 0; j < 4; j++) col[j] = add(col[j], c[k + j]);
  }
  for (int i = 0; i < P2_CELLS; i++) c[i] = add(c[i], col[i & 3]);
}
void p2_mix_host(const P2Consts& k, uint32_t* c) {
  m_ext_host(c);
  for (int r = 0; r < P2_HALF_FULL; r++) {
    for (int i = 0; i < P2_CELLS; i++) c[i] = sbox7(add(c[i], k.rc_full[r][i]));
    m_ext_host(c);
  }
  for (int r = 0; r < P2_PARTIAL; r++) {
    c[0] = sbox7(add(c[0], k.rc_partial[r]));
    uint32_t sum = 0;
    for (int i = 0; i < P2_CELLS; i++) sum = add(sum, c[i]);
    for (int i = 0; i < P2_CELLS; i++) c[i] = add(sum, mul(k.diag[i], c[i]));
  }
  for (int r = P2_HALF_FULL; r < 2 * P2_HALF_FULL; r++) {
    for (int i = 0; i < P2_CELLS; i++) c[i] = sbox7(add(c[i], k.rc_full[r][i]));
    m_ext_host(c);
  }
}
// The sponge below (p2_hash_elems_host) laid out row by row for the recursion circuit's in-circuit hash (include/r0hip_circuit.h SPONGE,
// tools/sponge_component.py): 30 rows per permutation -- absorb + external layer, then one round per row -- in 65 columns of `stride`
// words: st[24] the state after the row's step, aux[24] the cubes (x + rc)^3 of the lanes the round's S-box touches, in[16] the words
// absorbed on a permutation's first row, act = 1.  Only rows [0, *rows_used) are written; the caller clears the rest.
void p2_sponge_rows_host(const P2Consts& k, const uint32_t* words, size_t n_words, uint32_t* cols, size_t stride, size_t* rows_used) {
  constexpr int ROWS = 1 + 2 * P2_HALF_FULL + P2_PARTIAL;  // one permutation: the absorbing row, then a row per round
  const size_t n_perm = n_words ? (n_words + P2_RATE - 1) / P2_RATE : 1;
  uint32_t st[P2_CELLS] = {0};
  // a permutation's rows are made in a small block [column][row of the permutation] and go out column by column: 65 runs of 30
  // consecutive words instead of 1,950 single words a stride apart
  uint32_t blk[65][ROWS];
  for (size_t q = 0; q < n_perm; q++) {
    memset(blk, 0, sizeof blk);
    int row = 0;
    auto put_state = [&] {
      for (int j = 0; j < P2_CELLS; j++) blk[j][row] = st[j];
      blk[64][row] = ONE;
    };
    for (size_t j = 0; j < P2_RATE; j++) {
      st[j] = q * P2_RATE + j < n_words ? words[q * P2_RATE + j] : 0u;
      blk[48 + j][0] = st[j];
    }
    m_ext_host(st);
    put_state();
    row++;
    for (int r = 0; r < 2 * P2_HALF_FULL + P2_PARTIAL; r++, row++) {
      const bool full = r < P2_HALF_FULL || r >= P2_HALF_FULL + P2_PARTIAL;
      const uint32_t* rc = full ? k.rc_full[r < P2_HALF_FULL ? r : r - P2_PARTIAL] : &k.rc_partial[r - P2_HALF_FULL];
      for (int j = 0; j < (full ? P2_CELLS : 1); j++) {
        const uint32_t t = add(st[j], rc[j]), cube = mul(mul(t, t), t);
        st[j] = mul(mul(cube, cube), t);
        blk[24 + j][row] = cube;
      }
      if (full) m_ext_host(st);
      else {
        uint32_t sum = 0;
        for (int i = 0; i < P2_CELLS; i++) sum = add(sum, st[i]);
        for (int i = 0; i < P2_CELLS; i++) st[i] = add(sum, mul(k.diag[i], st[i]));
      }
      put_state();
    }
    for (int c = 0; c < 65; c++) memcpy(cols + (size_t)c * stride + q * ROWS, blk[c], sizeof blk[c]);
  }
  *rows_used = n_perm * ROWS;
}
// One pass of the sponge chain: the digest, and -- with `states` -- what every permutation starts from, 24 words each: the state after
// the absorb and before the external layer.  A permutation's 30 rows (p2_sponge_rows_host) depend on nothing else, so whoever wants
// the rows as well as the digest runs the sequential part once (r0h_lift / r0h_join: sponge_plant_states expands them on the device).
void p2_sponge_chain_host(const P2Consts& k, const uint32_t* elems, size_t n, uint32_t digest[8], std::vector<uint32_t>* states) {
  const size_t n_perm = n ? (n + P2_RATE - 1) / P2_RATE : 1;
  if (states) states->resize(n_perm * P2_CELLS);
  uint32_t st[P2_CELLS] = {0};
  for (size_t q = 0; q < n_perm; q++) {
    for (size_t j = 0; j < P2_RATE; j++) st[j] = q * P2_RATE + j < n ? elems[q * P2_RATE + j] : 0u;  // the last block is zero-padded
    if (states) memcpy(states->data() + q * P2_CELLS, st, sizeof st);
    p2_mix_host(k, st);
  }
  memcpy(digest, st, 32);
}
void p2_hash_elems_host(const P2Consts& k, const uint32_t* elems, size_t n, uint32_t digest[8]) { p2_sponge_chain_host(k, elems, n, digest, nullptr); }

}  // namespace r0h
