// The lazily accumulated dot products of the Poseidon2 partial rounds (csrc/poseidon2_device.hpp: dot_fix, dot_mac, dot_finish,
// p2_partial_rounds) compiled for the host with R0H_DOT_CHECK: every bound their correction schedules rely on is asserted in 128-bit
// arithmetic as the code runs -- no accumulator reaches 2^64, the high word is below 2p at each correction, reduce64 is handed less
// than 4 p^2.  Driven with
//   * every operand of every dot product at p - 1, fed to the dot routines directly (the exact worst case; no preimage reaches it
//     through the full rounds), and at zero: the tight schedule on the compiled-in table, the safe one on that table, on a table the
//     tight one does not cover, and on rows whose every word is p - 1;
//   * the tight schedule on rows of p - 1, where the checks must fire (they are compiled in and alive);
//   * random states through p2_partial_rounds and the whole permutation under both schedules, against the round-by-round form
//     (p2_mix_host, and its partial rounds restated here).
// Built with -fsanitize=address,undefined by tools/fuzz/run_p2_dot_check.sh; needs no GPU.
//   p2_dot_check            run the checks
//   p2_dot_check --masks    print the compiled schedules, one "tight|safe <row> <mask in hex>" per line
#define R0H_DOT_CHECK
#include <stdio.h>
#include <stdlib.h>

#include <random>

#include "poseidon2_device.hpp"

using namespace r0h;

static bool expect_failure = false;
static long failures = 0;
void r0h::r0h_dot_check_failed(const char* what, uint64_t acc) {
  failures++;
  if (expect_failure) return;
  fprintf(stderr, "p2_dot_check: %s (accumulator %016llx)\n", what, (unsigned long long)acc);
  abort();
}

typedef unsigned __int128 u128;

// one dot product of the schedule's row ROW over the words k, every operand `a`: what the routines return against the exact sum
template <class S, int ROW>
static void one_row(const uint32_t* k, uint32_t a) {
  constexpr int terms = p2_dot_terms(ROW);
  uint64_t acc;
  u128 exact = 0;
  for (int i = 0; i < terms; i++) {
    dot_mac<S, ROW>(acc, a, k[i], i);
    exact += (u128)a * k[i];
  }
  const uint32_t got = dot_finish<S, ROW>(acc);
  const uint32_t want = mul((uint32_t)(exact % P), 1u);  // the sum times 2^-32: the Montgomery reduction of the exact total
  if (expect_failure) return;
  if (got != want) {
    fprintf(stderr, "p2_dot_check: row %d, operands %u: %u, the exact sum gives %u\n", ROW, a, got, want);
    abort();
  }
}
template <class S, int... ROW>
static void all_rows(const uint32_t* part_sigma, const uint32_t* part_final, uint32_t a, std::integer_sequence<int, ROW...>) {
  (one_row<S, ROW>(ROW < P2_DOT_SIGMA_ROWS ? part_sigma + ROW * (P2_CELLS - 1) + ROW * (ROW + 1) / 2 : part_final + (ROW - P2_DOT_SIGMA_ROWS) * (P2_PARTIAL + 1), a), ...);
}
template <class S>
static void worst_and_zero(const P2Consts& k) {
  all_rows<S>(k.part_sigma, k.part_final, P - 1, std::make_integer_sequence<int, P2_DOT_ROWS>{});
  all_rows<S>(k.part_sigma, k.part_final, 0u, std::make_integer_sequence<int, P2_DOT_ROWS>{});
}

// the partial rounds of p2_mix_host, round by round
static void partial_rounds_plain(const P2Consts& k, uint32_t* c) {
  for (int r = 0; r < P2_PARTIAL; r++) {
    const uint32_t x = add(c[0], k.rc_partial[r]), x2 = mul(x, x), x4 = mul(x2, x2);
    c[0] = mul(mul(x4, x2), x);
    uint32_t sum = 0;
    for (int i = 0; i < P2_CELLS; i++) sum = add(sum, c[i]);
    for (int i = 0; i < P2_CELLS; i++) c[i] = add(sum, mul(k.diag[i], c[i]));
  }
}
template <class S>
static void random_states(const P2Consts& k, int n, uint32_t seed) {
  std::mt19937 rng(seed);
  for (int t = 0; t < n; t++) {
    uint32_t c[P2_CELLS], want[P2_CELLS], whole[P2_CELLS], whole_want[P2_CELLS];
    for (int i = 0; i < P2_CELLS; i++) {
      const uint32_t v = t == 0 ? P - 1 : t == 1 ? 0u : (uint32_t)(rng() % P);
      c[i] = want[i] = whole[i] = whole_want[i] = v;
    }
    p2_partial_rounds<S>(c, &k);
    partial_rounds_plain(k, want);
    p2_mix<0, S>(whole, &k);
    p2_mix_host(k, whole_want);
    if (memcmp(c, want, sizeof c) != 0 || memcmp(whole, whole_want, sizeof whole) != 0) {
      fprintf(stderr, "p2_dot_check: state %d of seed %u: the deferred partial rounds differ from the round-by-round form\n", t, seed);
      abort();
    }
  }
}

int main(int argc, char** argv) {
  if (argc > 1 && strcmp(argv[1], "--masks") == 0) {
    for (int row = 0; row < P2_DOT_ROWS; row++) printf("tight %d %016llx\n", row, (unsigned long long)P2_DOT_TIGHT.mask[row]);
    for (int row = 0; row < P2_DOT_ROWS; row++) printf("safe %d %016llx\n", row, (unsigned long long)P2_DOT_SAFE.mask[row]);
    return 0;
  }
  const P2Consts& def = p2_default();
  uint32_t minus_one[P2_CELLS];
  for (int i = 0; i < P2_CELLS; i++) minus_one[i] = P - 1;
  P2Consts uncovered, top;
  const bool default_tight = p2_dot_schedule_covers(P2_DOT_TIGHT, def.part_sigma, def.part_final);
  const bool uncovered_tight = fill_p2(uncovered, R0H_P2_ROUND_CONSTANTS, minus_one);  // every D_i = -1
  top = def;
  for (uint32_t& w : top.part_sigma) w = P - 1;
  for (uint32_t& w : top.part_final) w = P - 1;
  if (!default_tight || uncovered_tight || p2_dot_schedule_covers(P2_DOT_TIGHT, top.part_sigma, top.part_final) ||
      !p2_dot_schedule_covers(P2_DOT_SAFE, def.part_sigma, def.part_final) || !p2_dot_schedule_covers(P2_DOT_SAFE, uncovered.part_sigma, uncovered.part_final) ||
      !p2_dot_schedule_covers(P2_DOT_SAFE, top.part_sigma, top.part_final)) {
    fprintf(stderr, "p2_dot_check: the walk of the tables: the tight schedule must cover the compiled-in table alone, the safe one all three\n");
    return 1;
  }
  worst_and_zero<P2DotTight>(def);
  worst_and_zero<P2DotSafe>(def);
  worst_and_zero<P2DotSafe>(uncovered);
  worst_and_zero<P2DotSafe>(top);
  expect_failure = true;  // the tight schedule where it does not hold: the checks must see it
  worst_and_zero<P2DotTight>(top);
  expect_failure = false;
  if (failures == 0) {
    fprintf(stderr, "p2_dot_check: the tight schedule on rows of p - 1 raised no bound: the checks are not compiled in\n");
    return 1;
  }
  random_states<P2DotTight>(def, 3000, 1);
  random_states<P2DotSafe>(def, 1000, 2);
  random_states<P2DotSafe>(uncovered, 1000, 3);
  printf("p2 dot check: no report (%d + %d corrections per permutation; %ld bounds raised where they had to be)\n", p2_dot_corrections(P2_DOT_TIGHT),
         p2_dot_corrections(P2_DOT_SAFE), failures);
  return 0;
}
