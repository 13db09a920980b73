// When the lazily accumulated dot products of the deferred partial rounds (poseidon2_device.hpp: dot_mac, dot_finish) bring the
// accumulator's high word below p: one 64-bit mask per dot product, derived at compile time from the diagonal that is compiled in.
// Plain C++17, no device code: the kernels read the masks as constants, fill_p2 (poseidon2_host.cpp) walks the table it has filled against them,
// tools/fuzz/p2_dot_check.cpp prints them.
//
// The 43 dot products, in the order p2_partial_rounds evaluates them:
//   rows 0..19   part_sigma, round r = row + 1: 23 + r terms
//   rows 20..42  part_final, lane i = row - 19: 22 terms
// Bit idx of a row's mask: correct before term idx is added.  Bit P2_DOT_END: correct before reduce64.
//
// The rule.  Every a_i is a canonical word, every k_i a fixed word of the table, so an exact bound B on the accumulator follows the
// terms: B = (p - 1) k_0 after the first; before term i, if B + (p - 1) k_i could reach 2p 2^32 the high word is corrected first --
// it is below 2p there, which is what makes one conditional subtraction enough -- and B = p 2^32 - 1; at the end a correction is due
// only if B could reach 4 p^2, reduce64's precondition.  2p 2^32 < 2^64, so the accumulator never wraps.  With every k_i = p - 1 the
// rule asks for a correction before every second term from the fifth on: that, with a correction at every end, is P2DotSafe, the
// schedule that holds for any canonical table (550 corrections per permutation).
#pragma once
#include <stdint.h>

#include "../../include/r0hip_poseidon2_consts.h"
#include "fp.hpp"

namespace r0h {

constexpr int P2_DOT_SIGMA_ROWS = R0H_P2_ROUNDS_PARTIAL - 1, P2_DOT_ROWS = P2_DOT_SIGMA_ROWS + R0H_P2_CELLS - 1;  // 20 + 23
constexpr int P2_DOT_END = 63;
constexpr int P2_DOT_MAX_TERMS = R0H_P2_CELLS - 1 + P2_DOT_SIGMA_ROWS;  // the last part_sigma row: 43
constexpr uint64_t P2_DOT_FIX_LIMIT = ((uint64_t)2 * P) << 32;           // a correction needs the accumulator below 2p 2^32
constexpr uint64_t P2_DOT_FIXED = ((uint64_t)P << 32) - 1;               // ... and leaves it at most here
constexpr uint64_t P2_DOT_END_LIMIT = (uint64_t)4 * P * P;               // reduce64 needs its argument below 4 p^2

constexpr int p2_dot_terms(int row) { return row < P2_DOT_SIGMA_ROWS ? R0H_P2_CELLS + row : R0H_P2_ROUNDS_PARTIAL + 1; }

struct P2DotSchedule {
  uint64_t mask[P2_DOT_ROWS];
};
// the constant words of the 43 rows, as fill_p2 lays them out in P2Consts::part_sigma and part_final (Montgomery form)
struct P2DotTable {
  uint32_t k[P2_DOT_ROWS][P2_DOT_MAX_TERMS];
};

constexpr uint64_t p2_dot_row_mask(const uint32_t* k, int terms) {
  uint64_t mask = 0, bound = (uint64_t)(P - 1) * k[0];
  for (int i = 1; i < terms; i++) {
    const uint64_t term = (uint64_t)(P - 1) * k[i];
    if (bound >= P2_DOT_FIX_LIMIT - term) {  // bound + term >= 2p 2^32, without leaving 64 bits
      mask |= (uint64_t)1 << i;
      bound = P2_DOT_FIXED;
    }
    bound += term;
  }
  if (bound >= P2_DOT_END_LIMIT) mask |= (uint64_t)1 << P2_DOT_END;
  return mask;
}

constexpr uint32_t p2_dot_enc(uint32_t canonical) { return (uint32_t)((((uint64_t)canonical % P) << 32) % P); }  // the word enc() returns
constexpr P2DotTable p2_dot_table(const uint32_t* diag_m1) {
  uint32_t pw[R0H_P2_ROUNDS_PARTIAL + 1][R0H_P2_CELLS] = {}, kappa[R0H_P2_ROUNDS_PARTIAL + 1] = {};
  for (int e = 0; e <= R0H_P2_ROUNDS_PARTIAL; e++) {
    uint64_t ks = 0;
    for (int i = 1; i < R0H_P2_CELLS; i++) {
      pw[e][i] = e == 0 ? 1u : (uint32_t)((uint64_t)pw[e - 1][i] * diag_m1[i] % P);
      ks += pw[e][i];
    }
    kappa[e] = (uint32_t)(ks % P);
  }
  P2DotTable t = {};
  for (int r = 1; r < R0H_P2_ROUNDS_PARTIAL; r++) {
    for (int i = 1; i < R0H_P2_CELLS; i++) t.k[r - 1][i - 1] = p2_dot_enc(pw[r][i]);
    for (int j = 0; j < r; j++) t.k[r - 1][R0H_P2_CELLS - 1 + j] = p2_dot_enc(kappa[r - 1 - j]);
  }
  for (int i = 1; i < R0H_P2_CELLS; i++)
    for (int q = 0; q <= R0H_P2_ROUNDS_PARTIAL; q++) t.k[P2_DOT_SIGMA_ROWS + i - 1][q] = p2_dot_enc(pw[R0H_P2_ROUNDS_PARTIAL - q][i]);
  return t;
}
constexpr P2DotSchedule p2_dot_schedule(const P2DotTable& t) {
  P2DotSchedule s = {};
  for (int row = 0; row < P2_DOT_ROWS; row++) s.mask[row] = p2_dot_row_mask(t.k[row], p2_dot_terms(row));
  return s;
}
// the conservative schedule: the first four products fit as they are (4 p^2 < 2^64), then a correction before every second
// term keeps the total below p 2^32 + 2 p^2, and one more at the end
constexpr P2DotSchedule p2_dot_schedule_safe() {
  P2DotSchedule s = {};
  for (int row = 0; row < P2_DOT_ROWS; row++) {
    for (int i = 4; i < p2_dot_terms(row); i += 2) s.mask[row] |= (uint64_t)1 << i;
    s.mask[row] |= (uint64_t)1 << P2_DOT_END;
  }
  return s;
}
constexpr int p2_dot_corrections(const P2DotSchedule& s) {
  int n = 0;
  for (int row = 0; row < P2_DOT_ROWS; row++)
    for (int b = 0; b < 64; b++) n += (int)((s.mask[row] >> b) & 1);
  return n;
}

// The schedule of the compiled-in diagonal, and the one any canonical table is safe under.
constexpr P2DotSchedule P2_DOT_TIGHT = p2_dot_schedule(p2_dot_table(R0H_P2_INT_DIAG_M1));
constexpr P2DotSchedule P2_DOT_SAFE = p2_dot_schedule_safe();
static_assert(p2_dot_corrections(P2_DOT_SAFE) == 550, "the safe schedule: before every second term from the fifth on, and at every end");
static_assert(p2_dot_corrections(P2_DOT_TIGHT) < p2_dot_corrections(P2_DOT_SAFE), "the compiled-in diagonal allows fewer corrections");

// The policy p2_partial_rounds is compiled for (one instantiation of every Poseidon2 kernel each: hash_suite_device.hpp).
struct P2DotTight {
  static constexpr uint64_t mask(int row) { return P2_DOT_TIGHT.mask[row]; }
};
struct P2DotSafe {
  static constexpr uint64_t mask(int row) { return P2_DOT_SAFE.mask[row]; }
};

#if !defined(__HIP_DEVICE_COMPILE__)
// Whether a schedule covers the tables part_sigma / part_final of a P2Consts as they are laid out in memory: walked in exact 128-bit
// integers with every operand at p - 1, the accumulator stays below 2^64 throughout, is below 2p 2^32 wherever it is corrected and
// below 4 p^2 when reduce64 takes it.
inline bool p2_dot_schedule_covers(const P2DotSchedule& s, const uint32_t* part_sigma, const uint32_t* part_final) {
  typedef unsigned __int128 u128;
  const uint32_t* k = part_sigma;
  for (int row = 0; row < P2_DOT_ROWS; row++) {
    if (row == P2_DOT_SIGMA_ROWS) k = part_final;
    const int terms = p2_dot_terms(row);
    u128 bound = 0;
    for (int i = 0; i < terms; i++) {
      if (i && ((s.mask[row] >> i) & 1)) {
        if (bound >= (u128)P2_DOT_FIX_LIMIT) return false;
        if (bound > (u128)P2_DOT_FIXED) bound = P2_DOT_FIXED;
      }
      bound += (u128)(P - 1) * k[i];
      if (bound >> 64) return false;
    }
    if ((s.mask[row] >> P2_DOT_END) & 1) {
      if (bound >= (u128)P2_DOT_FIX_LIMIT) return false;
      if (bound > (u128)P2_DOT_FIXED) bound = P2_DOT_FIXED;
    }
    if (bound >= (u128)P2_DOT_END_LIMIT) return false;
    k += terms;
  }
  return true;
}
#endif

}  // namespace r0h
