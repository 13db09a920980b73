// Device-side Poseidon2 permutation (BabyBear, t=24, x^7, 4+21+4 rounds) over a state held in 24 VGPRs of one lane.
// Reached by the Merkle kernels through P2Device (hash_suite_device.hpp); shared with sponge.hip and tools/microbench/p2_rounds_bench.hip (per-round cycle counts).
#pragma once
#include <utility>

#include "internal.hpp"
#include "poseidon2_dot_schedule.hpp"

namespace r0h {

// x^7 with lazily reduced intermediates (bounds in units of p, x < 1):
//   x2 = x*x        < 0.47 + 1 = 1.47        x3 = x2*x < 0.69 + 1 = 1.69      x4 = x2*x2 < 1.02 + 1 = 2.02 (t + 2^32 p < 2^64 holds)
//   x4' = x4 - p if that does not wrap (< 1.02)                               x7 = x3*x4' < 0.81 + 1, then one reduction
// Two conditional subtractions fewer than four full products; the result is the same canonical word.  (A signed-Montgomery
// chain -- v_mad_i64_i32 / v_mul_hi_i32, no corrections until the end -- measured 19 % slower: tools/microbench/p2_rounds_bench.)
R0H_HD uint32_t sbox7(uint32_t x) {
  uint32_t x2 = mul_lazy(x, x);
  uint32_t x3 = mul_lazy(x2, x);
  uint32_t x4 = reduce1(mul_lazy(x2, x2));
  return reduce1(mul_lazy(x3, x4));
}

// One modular add inside a larger asm statement: r = a + b mod p (x: scratch).  r may be a or b.
#define R0H_ASM_ADD(r, a, b, x) "v_add_u32 " r ", " a ", " b "\n\tv_subrev_co_u32 " x ", vcc, 0x78000001, " r "\n\tv_cndmask_b32 " r ", " x ", " r ", vcc\n\t"
// External linear layer: circ(2 M4, M4, .., M4) with M4 = [[2,3,1,1],[1,2,3,1],[1,1,2,3],[3,1,1,2]] -- 124 modular adds (the
// first block's outputs seed the column sums; the plain form below is the restatement).
// Written as seven asm statements (one per block of four cells incl. its share of the column sums, one for the final 24 adds):
// hipcc puts an `s_nop 0` between an asm statement and the next instruction touching a register that statement wrote (it assumes
// a dst-forwarding hazard on gfx950 for anything inside asm), so the one-statement-per-add form carried a nop with every add:
// the kernel is VALU-throughput bound, so the nops themselves cost next to nothing, but the statement form needs 98 instead of 139
// VGPRs (four waves per SIMD instead of three) and measures 0.45 % faster on hash_rows in an A/B on one box
// (profiles/r02/poseidon2_variants.md).  Same canonical words: every add is reduced, only the statement boundaries moved.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(R0H_MEXT_PLAIN)
// M4 on one block of four cells and its share of the column sums.  FIRST: the block's outputs ARE the sums so far (nothing is
// added to zero); the second block then writes its sums to fresh registers (the first block's outputs stay live as cells).
#define R0H_ASM_M4(T0, T1, T2, T3, U, X, A, B, D, E, O0, O1, O2, O3) \
  R0H_ASM_ADD(T0, A, B, X)    /* t0 = a + b */ \
  R0H_ASM_ADD(T1, D, E, X)    /* t1 = d + e */ \
  R0H_ASM_ADD(U, B, B, X)     /* u = 2b */ \
  R0H_ASM_ADD(T2, U, T1, X)   /* t2 = 2b + t1 */ \
  R0H_ASM_ADD(U, E, E, X)     /* u = 2e */ \
  R0H_ASM_ADD(T3, U, T0, X)   /* t3 = 2e + t0 */ \
  R0H_ASM_ADD(T1, T1, T1, X)  /* 2 t1 */ \
  R0H_ASM_ADD(T1, T1, T1, X)  /* 4 t1 */ \
  R0H_ASM_ADD(O3, T1, T3, X)  /* o3 = t4 = 4 t1 + t3 */ \
  R0H_ASM_ADD(T0, T0, T0, X)  /* 2 t0 */ \
  R0H_ASM_ADD(T0, T0, T0, X)  /* 4 t0 */ \
  R0H_ASM_ADD(O1, T0, T2, X)  /* o1 = t5 = 4 t0 + t2 */ \
  R0H_ASM_ADD(O0, T3, O1, X)  /* o0 = t3 + t5 */ \
  R0H_ASM_ADD(O2, T2, O3, X)  /* o2 = t2 + t4 */
template <bool FIRST>
__device__ __forceinline__ void m4_block(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t& s0, uint32_t& s1, uint32_t& s2, uint32_t& s3) {
  uint32_t o0, o1, o2, o3, t0, t1, t2, t3, u, x;
  if (FIRST) {
    // %0-3 o, %4-9 t0 t1 t2 t3 u x, %10-13 a b d e
    asm(R0H_ASM_M4("%4", "%5", "%6", "%7", "%8", "%9", "%10", "%11", "%12", "%13", "%0", "%1", "%2", "%3")
        : "=&v"(o0), "=&v"(o1), "=&v"(o2), "=&v"(o3), "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3), "=&v"(u), "=&v"(x)
        : "v"(c0), "v"(c1), "v"(c2), "v"(c3)
        : "vcc");
    s0 = o0; s1 = o1; s2 = o2; s3 = o3;
  } else {
    // %0-3 o, %4-7 s (out), %8-13 t0 t1 t2 t3 u x, %14-17 a b d e, %18-21 s (in)
    uint32_t n0, n1, n2, n3;
    asm(R0H_ASM_M4("%8", "%9", "%10", "%11", "%12", "%13", "%14", "%15", "%16", "%17", "%0", "%1", "%2", "%3")
        R0H_ASM_ADD("%4", "%18", "%0", "%13") R0H_ASM_ADD("%5", "%19", "%1", "%13") R0H_ASM_ADD("%6", "%20", "%2", "%13") R0H_ASM_ADD("%7", "%21", "%3", "%13")
        : "=&v"(o0), "=&v"(o1), "=&v"(o2), "=&v"(o3), "=&v"(n0), "=&v"(n1), "=&v"(n2), "=&v"(n3), "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3), "=&v"(u), "=&v"(x)
        : "v"(c0), "v"(c1), "v"(c2), "v"(c3), "v"(s0), "v"(s1), "v"(s2), "v"(s3)
        : "vcc");
    s0 = n0; s1 = n1; s2 = n2; s3 = n3;
  }
  c0 = o0; c1 = o1; c2 = o2; c3 = o3;
}
// c[k..k+3] += (s0, s1, s2, s3) for the blocks [0, N) of four cells, one statement
template <int N>
__device__ __forceinline__ void add_sums(uint32_t (&c)[P2_CELLS], uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3);
template <>
__device__ __forceinline__ void add_sums<2>(uint32_t (&c)[P2_CELLS], uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3) {
  uint32_t x;
  // %0-7 cells (in/out), %8 scratch, %9-12 column sums
  asm(R0H_ASM_ADD("%0", "%0", "%9", "%8") R0H_ASM_ADD("%1", "%1", "%10", "%8") R0H_ASM_ADD("%2", "%2", "%11", "%8") R0H_ASM_ADD("%3", "%3", "%12", "%8")
      R0H_ASM_ADD("%4", "%4", "%9", "%8") R0H_ASM_ADD("%5", "%5", "%10", "%8") R0H_ASM_ADD("%6", "%6", "%11", "%8") R0H_ASM_ADD("%7", "%7", "%12", "%8")
      : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(c[4]), "+v"(c[5]), "+v"(c[6]), "+v"(c[7]), "=&v"(x)
      : "v"(s0), "v"(s1), "v"(s2), "v"(s3)
      : "vcc");
}
template <>
__device__ __forceinline__ void add_sums<4>(uint32_t (&c)[P2_CELLS], uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3) {
  uint32_t x;
  // %0-15 cells (in/out), %16 scratch, %17-20 column sums
  asm(R0H_ASM_ADD("%0", "%0", "%17", "%16") R0H_ASM_ADD("%1", "%1", "%18", "%16") R0H_ASM_ADD("%2", "%2", "%19", "%16") R0H_ASM_ADD("%3", "%3", "%20", "%16")
      R0H_ASM_ADD("%4", "%4", "%17", "%16") R0H_ASM_ADD("%5", "%5", "%18", "%16") R0H_ASM_ADD("%6", "%6", "%19", "%16") R0H_ASM_ADD("%7", "%7", "%20", "%16")
      R0H_ASM_ADD("%8", "%8", "%17", "%16") R0H_ASM_ADD("%9", "%9", "%18", "%16") R0H_ASM_ADD("%10", "%10", "%19", "%16") R0H_ASM_ADD("%11", "%11", "%20", "%16")
      R0H_ASM_ADD("%12", "%12", "%17", "%16") R0H_ASM_ADD("%13", "%13", "%18", "%16") R0H_ASM_ADD("%14", "%14", "%19", "%16") R0H_ASM_ADD("%15", "%15", "%20", "%16")
      : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(c[4]), "+v"(c[5]), "+v"(c[6]), "+v"(c[7]), "+v"(c[8]), "+v"(c[9]), "+v"(c[10]), "+v"(c[11]),
        "+v"(c[12]), "+v"(c[13]), "+v"(c[14]), "+v"(c[15]), "=&v"(x)
      : "v"(s0), "v"(s1), "v"(s2), "v"(s3)
      : "vcc");
}
template <>
__device__ __forceinline__ void add_sums<6>(uint32_t (&c)[P2_CELLS], uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3) {
  uint32_t x;
  // %0-23 cells (in/out), %24 scratch, %25-28 column sums
  asm(R0H_ASM_ADD("%0", "%0", "%25", "%24") R0H_ASM_ADD("%1", "%1", "%26", "%24") R0H_ASM_ADD("%2", "%2", "%27", "%24") R0H_ASM_ADD("%3", "%3", "%28", "%24")
      R0H_ASM_ADD("%4", "%4", "%25", "%24") R0H_ASM_ADD("%5", "%5", "%26", "%24") R0H_ASM_ADD("%6", "%6", "%27", "%24") R0H_ASM_ADD("%7", "%7", "%28", "%24")
      R0H_ASM_ADD("%8", "%8", "%25", "%24") R0H_ASM_ADD("%9", "%9", "%26", "%24") R0H_ASM_ADD("%10", "%10", "%27", "%24") R0H_ASM_ADD("%11", "%11", "%28", "%24")
      R0H_ASM_ADD("%12", "%12", "%25", "%24") R0H_ASM_ADD("%13", "%13", "%26", "%24") R0H_ASM_ADD("%14", "%14", "%27", "%24") R0H_ASM_ADD("%15", "%15", "%28", "%24")
      R0H_ASM_ADD("%16", "%16", "%25", "%24") R0H_ASM_ADD("%17", "%17", "%26", "%24") R0H_ASM_ADD("%18", "%18", "%27", "%24") R0H_ASM_ADD("%19", "%19", "%28", "%24")
      R0H_ASM_ADD("%20", "%20", "%25", "%24") R0H_ASM_ADD("%21", "%21", "%26", "%24") R0H_ASM_ADD("%22", "%22", "%27", "%24") R0H_ASM_ADD("%23", "%23", "%28", "%24")
      : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(c[4]), "+v"(c[5]), "+v"(c[6]), "+v"(c[7]), "+v"(c[8]), "+v"(c[9]), "+v"(c[10]), "+v"(c[11]),
        "+v"(c[12]), "+v"(c[13]), "+v"(c[14]), "+v"(c[15]), "+v"(c[16]), "+v"(c[17]), "+v"(c[18]), "+v"(c[19]), "+v"(c[20]), "+v"(c[21]), "+v"(c[22]), "+v"(c[23]),
        "=&v"(x)
      : "v"(s0), "v"(s1), "v"(s2), "v"(s3)
      : "vcc");
}
// The layer as a whole.  ZERO_CAP: the capacity cells c[16..23] are zero on entry, so their two M4 blocks are zero and they leave
// as the column sums.  DIGEST_ONLY: only c[0..7] are read afterwards (the cells c[8..23] are left without their column sums).
template <bool ZERO_CAP = false, bool DIGEST_ONLY = false>
__device__ __forceinline__ void m_ext(uint32_t (&c)[P2_CELLS]) {
  uint32_t s0, s1, s2, s3;
  m4_block<true>(c[0], c[1], c[2], c[3], s0, s1, s2, s3);
#pragma unroll
  for (int k = 4; k < (ZERO_CAP ? P2_RATE : P2_CELLS); k += 4) m4_block<false>(c[k], c[k + 1], c[k + 2], c[k + 3], s0, s1, s2, s3);
  if (DIGEST_ONLY) {
    add_sums<2>(c, s0, s1, s2, s3);
  } else if (ZERO_CAP) {
    add_sums<4>(c, s0, s1, s2, s3);
    c[16] = c[20] = s0; c[17] = c[21] = s1; c[18] = c[22] = s2; c[19] = c[23] = s3;
  } else {
    add_sums<6>(c, s0, s1, s2, s3);
  }
}
#else
template <bool ZERO_CAP = false, bool DIGEST_ONLY = false>  // (the plain form takes no advantage of either)
__device__ __forceinline__ void m_ext(uint32_t (&c)[P2_CELLS]) {
  uint32_t s0, s1, s2, s3;
#pragma unroll
  for (int k = 0; k < P2_CELLS; k += 4) {
    uint32_t a = c[k], b = c[k + 1], d = c[k + 2], e = c[k + 3];
    uint32_t t0 = add(a, b), t1 = add(d, e);
    uint32_t t2 = add(add(b, b), t1), t3 = add(add(e, e), t0);
    uint32_t t1x2 = add(t1, t1), t0x2 = add(t0, t0);
    uint32_t t4 = add(add(t1x2, t1x2), t3), t5 = add(add(t0x2, t0x2), t2);
    c[k] = add(t3, t5); c[k + 1] = t5; c[k + 2] = add(t2, t4); c[k + 3] = t4;
    if (k == 0) { s0 = c[0]; s1 = c[1]; s2 = c[2]; s3 = c[3]; }
    else { s0 = add(s0, c[k]); s1 = add(s1, c[k + 1]); s2 = add(s2, c[k + 2]); s3 = add(s3, c[k + 3]); }
  }
#pragma unroll
  for (int k = 0; k < P2_CELLS; k += 4) {
    c[k] = add(c[k], s0); c[k + 1] = add(c[k + 1], s1); c[k + 2] = add(c[k + 2], s2); c[k + 3] = add(c[k + 3], s3);
  }
}
#endif

// c[1] + ... + c[23] mod p for reduced words, as a balanced tree
R0H_HD uint32_t sum_lanes_1_to_23(const uint32_t (&c)[P2_CELLS]) {
  uint32_t s1[12];
R0H_UNROLL
  for (int i = 0; i < 11; i++) s1[i] = add(c[2 * i + 2], c[2 * i + 3]);
  s1[11] = c[1];
  uint32_t s2[6];
R0H_UNROLL
  for (int i = 0; i < 6; i++) s2[i] = add(s1[2 * i], s1[2 * i + 1]);
  return add(add(add(s2[0], s2[1]), add(s2[2], s2[3])), add(s2[4], s2[5]));
}

// digest_only (wave-uniform; a constant folds away): the round is a hash's last, only c[0..7] are read after it
__device__ __forceinline__ void p2_full_round(uint32_t (&c)[P2_CELLS], const uint32_t* __restrict__ rc, bool digest_only = false) {
#pragma unroll
  for (int i = 0; i < P2_CELLS; i++) c[i] = sbox7(add(c[i], rc[i]));
  if (digest_only) m_ext<false, true>(c);
  else m_ext(c);
}

// Lazily accumulated dot product mod p: 64-bit accumulator, products of reduced words.  The accumulator's high word is brought
// below p (dot_fix: one conditional subtraction, which needs it below 2p, i.e. the accumulator below 2p 2^32 < 2^64) where the
// schedule S says so, and once more before reduce64 if S asks for it (poseidon2_dot_schedule.hpp).  Two schedules:
//   P2DotSafe   holds for every canonical table: the first four products fit as they are (4 p^2 < 2^64), from then on a correction
//               before every second product keeps the total below p 2^32 + 2 p^2, and one at the end: 550 per permutation.
//   P2DotTight  from an exact bound over the words of the compiled-in table, which are about p/2 on average: 258 per permutation.
//               Every correction subtracts p 2^32 from a value that is reduced mod p afterwards, so the words are the same.
// fill_p2 (poseidon2_host.cpp) checks the tight schedule against the table a context loads, and the launches choose the instantiation from that.
// ~11 SIMD cycles per term against ~34 for a reduced product plus a modular add (tools/microbench/dot_bench.hip).
// ROW (the dot product, in the schedule's numbering) is a template argument, so a row's mask is an immediate; `idx` (the term's
// position) is compile-time after unrolling.  (Masks looked up by a loop variable are loads from a table until the loops are
// unrolled, and with them in the body the loops are not unrolled.)  The functions from here to p2_partial_rounds also compile for
// the host (tools/fuzz/p2_dot_check.cpp); with R0H_DOT_CHECK defined there, every bound the schedule relies on is asserted in 128-bit
// arithmetic as the code runs.
#if defined(R0H_DOT_CHECK) && !defined(__HIP_DEVICE_COMPILE__)
void r0h_dot_check_failed(const char* what, uint64_t acc);  // defined by the checking program
#define R0H_DOT_REQUIRE(cond, what, acc) do { if (!(cond)) r0h_dot_check_failed(what, acc); } while (0)
#else
#define R0H_DOT_REQUIRE(cond, what, acc) do { } while (0)
#endif
R0H_HD void dot_fix(uint64_t& acc) {
  uint32_t hi = (uint32_t)(acc >> 32);
  R0H_DOT_REQUIRE(hi < 2 * (uint64_t)P, "a correction finds the high word at or above 2p", acc);
#if defined(__HIP_DEVICE_COMPILE__)
  // reduce1 on the high word IN PLACE: the word is a read-write operand and only the scratch is early-clobber, so the register
  // coalescer keeps it in the accumulator pair.  reduce1 itself returns an early-clobber output, which cost a v_mov_b32 back into
  // the pair after every correction; same two full-rate instructions, same word.
  uint32_t x;
  asm("v_subrev_co_u32 %1, vcc, 0x78000001, %0\n\tv_cndmask_b32 %0, %1, %0, vcc" : "+v"(hi), "=&v"(x) : : "vcc");
#else
  hi = reduce1(hi);
#endif
  acc = ((uint64_t)hi << 32) | (uint32_t)acc;
#if defined(__HIP_DEVICE_COMPILE__)
  // opaque re-pack: seen as (hi << 32) + lo, the optimiser re-associates the following multiply-adds into separate 64-bit
  // additions and moves instead of one v_mad_u64_u32 on the accumulator pair
  asm("" : "+v"(acc));
#endif
}
template <class S, int ROW>
R0H_HD void dot_mac(uint64_t& acc, uint32_t a, uint32_t b, int idx) {
  constexpr uint64_t mask = S::mask(ROW);
  if (idx == 0) { acc = (uint64_t)a * b; return; }
  if ((mask >> idx) & 1) dot_fix(acc);
  R0H_DOT_REQUIRE((((unsigned __int128)acc + (unsigned __int128)a * b) >> 64) == 0, "the accumulator reaches 2^64", acc);
  acc += (uint64_t)a * b;
}
template <class S, int ROW>
R0H_HD uint32_t dot_finish(uint64_t acc) {
  constexpr uint64_t mask = S::mask(ROW);
  if ((mask >> P2_DOT_END) & 1) dot_fix(acc);
  R0H_DOT_REQUIRE(acc < P2_DOT_END_LIMIT, "reduce64 is handed 4 p^2 or more", acc);
  return reduce64(acc);
}

// The 21 partial rounds with the linear layer of lanes 1..23 deferred.  Only lane 0 is non-linear, so with u_i the lanes at
// entry, D_i = mu_i - 1 and sum_r the state sum of round r, lane i after round r is  D_i^r u_i + sum_{j<r} D_i^{r-1-j} sum_j.
// Per round that leaves the S-box of lane 0 and ONE dot product for the sum of the other lanes,
//   sigma_r = sum_i D_i^r u_i + sum_{j<r} kappa_{r-1-j} sum_j      (kappa_k = sum_i D_i^k),
// and the lanes themselves are materialised once at the end (22 terms each): 1176 lazily accumulated terms in all, instead
// of 21 x 24 reduced constant products and 21 x 48 modular adds.  Same canonical words as the round-by-round form.
// Round R and lane I are template arguments for the schedule's sake (above); `row` walks part_sigma as the rounds go.
template <class S, int R>
R0H_HD void p2_partial_round(const uint32_t (&c)[P2_CELLS], uint32_t (&sums)[P2_PARTIAL], uint32_t& s0, uint32_t& sigma,
                             const uint32_t*& row, const P2Consts* __restrict__ k) {
  if (R > 0) {
    constexpr int ROW = R > 0 ? R - 1 : 0;
    uint64_t acc;
R0H_UNROLL
    for (int i = 0; i < P2_CELLS - 1; i++) dot_mac<S, ROW>(acc, c[i + 1], row[i], i);
R0H_UNROLL
    for (int j = 0; j < R; j++) dot_mac<S, ROW>(acc, sums[j], row[P2_CELLS - 1 + j], P2_CELLS - 1 + j);
    sigma = dot_finish<S, ROW>(acc);
    row += P2_CELLS - 1 + R;
  }
  const uint32_t y = sbox7(add(s0, k->rc_partial[R]));
  sums[R] = add(y, sigma);
  s0 = add(sums[R], mul_const(y, k->diag_canon[0], k->diag_shoup[0]));
}
template <class S, int I>
R0H_HD void p2_partial_lane(uint32_t (&c)[P2_CELLS], const uint32_t (&sums)[P2_PARTIAL], const uint32_t* f) {
  constexpr int ROW = P2_DOT_SIGMA_ROWS + I - 1;
  uint64_t acc;
  dot_mac<S, ROW>(acc, c[I], f[0], 0);
R0H_UNROLL
  for (int q = 0; q < P2_PARTIAL; q++) dot_mac<S, ROW>(acc, sums[q], f[1 + q], 1 + q);
  c[I] = dot_finish<S, ROW>(acc);
}
template <class S, int... R, int... I>
R0H_HD void p2_partial_rounds_seq(uint32_t (&c)[P2_CELLS], const P2Consts* __restrict__ k, std::integer_sequence<int, R...>,
                                  std::integer_sequence<int, I...>) {
  // table offsets go through an opaque zero: with constant offsets, loop-invariant code motion precomputes one 64-bit address
  // per table row outside the caller's loop and spills hundreds of SGPRs
  uint32_t zero;
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("s_mov_b32 %0, 0" : "=s"(zero));
#else
  zero = 0;
#endif
  uint32_t sums[P2_PARTIAL];
  uint32_t s0 = c[0];
  uint32_t sigma = sum_lanes_1_to_23(c);
  const uint32_t* row = k->part_sigma + zero;
  (p2_partial_round<S, R>(c, sums, s0, sigma, row, k), ...);
  c[0] = s0;
  (p2_partial_lane<S, I + 1>(c, sums, k->part_final + zero + I * (P2_PARTIAL + 1)), ...);
}
// S has no default, here and in p2_mix_ends, p2_mix, p2_hash_row: P2DotTight is valid only for a table fill_p2 has found it to cover,
// so whoever takes it says so (with_suite does, by r0h_ctx::p2_tight).
template <class S>
R0H_HD void p2_partial_rounds(uint32_t (&c)[P2_CELLS], const P2Consts* __restrict__ k) {
  p2_partial_rounds_seq<S>(c, k, std::make_integer_sequence<int, P2_PARTIAL>{}, std::make_integer_sequence<int, P2_CELLS - 1>{});
}

// The permutation, with what the sponge knows about its ends (both wave-uniform; compile-time constants fold away):
//   zero_cap     the capacity cells c[16..23] are zero on entry (a hash's first block): the first linear layer skips their blocks
//   digest_only  only c[0..7] are read afterwards (a hash's last block): the last linear layer leaves c[8..23] unfinished
// The canonical words that are read are those of the plain permutation.  One body serves every block of hash_rows: the two
// shorter layers sit beside the full ones behind scalar branches, the rounds themselves are not duplicated.
template <class S>
__device__ __forceinline__ void p2_mix_ends(uint32_t (&c)[P2_CELLS], const P2Consts* __restrict__ k, bool zero_cap, bool digest_only) {
  if (zero_cap) m_ext<true, false>(c);
  else m_ext(c);
#pragma unroll 1
  for (int r = 0; r < P2_HALF_FULL; r++) p2_full_round(c, k->rc_full[r]);
  p2_partial_rounds<S>(c, k);
#pragma unroll 1
  for (int r = P2_HALF_FULL; r < 2 * P2_HALF_FULL; r++) {
    p2_full_round(c, k->rc_full[r], digest_only && r == 2 * P2_HALF_FULL - 1);
  }
}
constexpr int P2_ZERO_CAP = 1, P2_DIGEST_ONLY = 2;
template <int ENDS, class S>
__device__ __forceinline__ void p2_mix(uint32_t (&c)[P2_CELLS], const P2Consts* __restrict__ k) {
  p2_mix_ends<S>(c, k, (ENDS & P2_ZERO_CAP) != 0, (ENDS & P2_DIGEST_ONLY) != 0);
}

// The row sponge: c[0..7] = digest of the `cols` words src[0], src[rows], src[2 * rows], .. (one row of a column-major matrix), absorbed
// in rate blocks.  P2Device::row (hash_suite_device.hpp): what hash_rows_kernel computes per lane,
// merkle_open_top_kernel per leaf and merkle_climb_kernel per opening.
template <class S>
__device__ __forceinline__ void p2_hash_row(uint32_t (&c)[P2_CELLS], const uint32_t* src, uint32_t rows, uint32_t cols,
                                            const P2Consts* __restrict__ k) {
#pragma unroll
  for (int i = 0; i < P2_CELLS; i++) c[i] = 0;
  const uint32_t blocks = cols ? (cols + P2_RATE - 1) / P2_RATE : 1u;  // the last one may be partial, zero-padded (all zeros for cols == 0)
  // One permutation body for every block: the first enters with a zero capacity, only the digest is read from the last.  One
  // form of the loads too, each behind a scalar test of its column (two bodies, or a full and a padded form of the loads side by
  // side, cost registers and 0.2-0.6 % of the kernel: profiles/r11/poseidon2_trims.md).
  // (prefetching the next rate block into registers was measured: no gain, the kernel is VALU-issue bound)
  for (uint32_t blk = 0; blk < blocks; blk++) {
    const uint32_t have = cols - blk * P2_RATE;  // columns left, this block's included
#pragma unroll
    for (int i = 0; i < P2_RATE; i++) c[i] = (uint32_t)i < have ? src[(size_t)(blk * P2_RATE + i) * rows] : 0u;
    p2_mix_ends<S>(c, k, blk == 0, blk + 1 == blocks);
  }
}

// One permutation spread over 24 lanes of a 32-lane half-wave, one state cell per lane (`c`: lane l's cell, l = lane within the half;
// lanes 24..31 carry don't-cares): S-boxes run in parallel, the external layer exchanges within quads and across the six quads by
// shuffles, the internal layer is a 5-step shuffle all-reduce.  32x the instructions of the one-lane form and about a seventh of its
// latency: for chains of single permutations -- the upper Merkle levels (hash_fold_lanes_kernel, merkle.hip) and the transcript's
// generator (P2Transcript, hash_suite_device.hpp).  Every lane of the half-wave must call it.  The plain round-by-round permutation, the
// same canonical words as p2_mix.  (Cross-lane: compiled by hipcc only, not by the host builds of this header.)
#if defined(__HIPCC__)
__device__ __forceinline__ uint32_t half_shfl(uint32_t v, uint32_t src_in_half) {
  return __shfl(v, (int)((threadIdx.x & 32u) | src_in_half), 64);
}
__device__ __forceinline__ uint32_t m_ext_lanes(uint32_t x, uint32_t l) {
  const uint32_t q = l & ~3u;
  uint32_t a = half_shfl(x, q), b = half_shfl(x, q | 1), d = half_shfl(x, q | 2), e = half_shfl(x, q | 3);
  uint32_t t0 = add(a, b), t1 = add(d, e);
  uint32_t t2 = add(add(b, b), t1), t3 = add(add(e, e), t0);
  uint32_t t1x2 = add(t1, t1), t0x2 = add(t0, t0);
  uint32_t t4 = add(add(t1x2, t1x2), t3), t5 = add(add(t0x2, t0x2), t2);
  uint32_t t6 = add(t3, t5), t7 = add(t2, t4);
  const uint32_t j = l & 3u;
  uint32_t y = j == 0 ? t6 : (j == 1 ? t5 : (j == 2 ? t7 : t4));
  // column sums over the six quads: pair neighbours, then add the two other pairs (lanes 24..31 carry don't-cares)
  uint32_t t = add(y, half_shfl(y, l ^ 4u));
  uint32_t s = add(t, add(half_shfl(t, (l + 8u) % 24u), half_shfl(t, (l + 16u) % 24u)));
  return add(y, s);
}
__device__ __forceinline__ uint32_t p2_mix_lanes(uint32_t c, uint32_t l, const P2Consts* __restrict__ k) {
  const bool cell = l < 24u;
  const uint32_t li = cell ? l : 0u;
  const uint32_t dg = k->diag_canon[li], ds = k->diag_shoup[li];
  c = m_ext_lanes(c, l);
  for (int r = 0; r < P2_HALF_FULL; r++) c = m_ext_lanes(sbox7(add(c, k->rc_full[r][li])), l);
  for (int r = 0; r < P2_PARTIAL; r++) {
    if (l == 0) c = sbox7(add(c, k->rc_partial[r]));
    uint32_t sum = cell ? c : 0u;
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) sum = add(sum, half_shfl(sum, l ^ (uint32_t)off));
    c = add(sum, mul_const(c, dg, ds));
  }
  for (int r = P2_HALF_FULL; r < 2 * P2_HALF_FULL; r++) c = m_ext_lanes(sbox7(add(c, k->rc_full[r][li])), l);
  return c;
}
#endif

}  // namespace r0h
