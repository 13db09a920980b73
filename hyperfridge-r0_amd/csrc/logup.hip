// The log-derivative accumulation (blob section LOGUP, include/r0hip_circuit.h): the ACCUM group of a circuit whose argument is a sum
// of fractions numerator / (challenge-weighted linear forms of the row) -- lookups into the CODE group's tables, memory tuples,
// session tuples.  Stands where risc0-circuit-rv32im 4.0.4's `step_accum` + the hal's `prefix_products` stand (SURVEY.md 8(a) a10:
// "lookup/permutation argument ... log-derivative"); the fractions themselves come from the blob (tools/trace_circuit.py).
//
// Three device steps, all streams over columns (consecutive lanes own consecutive rows, every column access is a 256-byte line):
//   1. multiplicities: the lookups of a table are walked from a flat list of (numerator, value) forms (logup_lookup_list) by a grid of
//      one workgroup per CU, each striding over the rows with an LDS histogram of half the table's value range -- one launch per (table,
//      half), every in-table lookup an LDS atomic whatever its value; global memory sees each workgroup's flush alone, non-zero bins as
//      contiguous runs.  Zero, by far the most frequent value (idle slots), is counted by subtraction from the slots that are not gated
//      off (a numerator of 0); the counts become the table's multiplicity column in DATA (before DATA is committed);
//   2. terms: one thread per row evaluates the row's fractions accumulator by accumulator, sum_f n_f / d_f = N / D, with ONE
//      extension-field inversion per batch of up to four accumulators (fp4_batch_div), and leaves the running sum WITHIN the row in the
//      ACCUM columns;
//   3. the row totals are scanned (r0h_prefix_sums) and added back: the chain runs through the rows.
// The term interpreter reads a flat tape of the fractions (uniform across the wave: scalar loads) built per launch on the host, public
// inputs folded into the coefficients.  The accumulators with a public total are evaluated and scanned for their totals
// (r0h_logup_totals); a session keeps those scanned terms for the accumulation of the same segment (LogupKept, circuit.hpp).
// The same tape, with the challenges' identities in place of their values, is what the balance check walks (r0h_logup_check_balance: which
// classes of the chain links' tuples do not cancel; the kernels are described where they stand).
#include <algorithm>
#include <map>

#include "../../include/r0hip_circuit.h"
#include "circuit.hpp"

namespace r0h {

namespace {
struct Tape {
  std::vector<uint32_t> words;              // per accumulator, per fraction: table, num form, n_parts, (challenge index, form)...; form = n, (coef, column + 1)...
  std::vector<const uint32_t*> cols;        // column base pointers
  std::vector<Fp4> ch;                      // challenges; index 0 is "one"
  std::vector<uint64_t> ch_id;              // their identities, kind << 32 | index (0: "one"): what the balance check's weights are indexed by
  std::vector<uint32_t> acc_begin;          // word offset of every accumulator
};

// `n_accs`: the first n_accs accumulators alone (the balance check walks the chain links and nothing else); `first_acc`: those before
// it are left out (the session balance walks the accumulators with a public total and nothing else)
const char* build_tape(const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, const uint32_t* global, const uint32_t* mix, Tape* t, uint32_t n_accs = 0xffffffffu,
                       uint32_t first_acc = 0) {
  std::map<uint32_t, uint32_t> col_index;
  std::map<uint64_t, uint32_t> ch_index;
  t->ch.push_back(fp4_one());
  t->ch_id.push_back(0);
  auto form = [&](const Lf& lf) -> const char* {
    t->words.push_back((uint32_t)lf.terms.size());
    for (const LfTerm& term : lf.terms) {
      uint32_t coef = enc(term.coef);
      if (term.global) {
        R0H_REQUIRE(global, "log-derivative accumulation: a form reads a public input and none were given");
        coef = mul(coef, global[term.global - 1]);
      }
      uint32_t col = 0;
      if (term.col) {
        const uint32_t ref = term.col - 1;
        auto it = col_index.find(ref);
        if (it == col_index.end()) {
          const r0h_buf* src = (ref >> 28) == R0H_GROUP_CODE ? code : data;
          R0H_REQUIRE(src, "log-derivative accumulation: a form reads the %s group and none was given", (ref >> 28) == R0H_GROUP_CODE ? "CODE" : "DATA");
          it = col_index.emplace(ref, (uint32_t)t->cols.size()).first;
          t->cols.push_back(u32(src) + ((size_t)(ref & 0xfffffu) << po2));
        }
        col = it->second + 1;
      }
      t->words.push_back(coef);
      t->words.push_back(col);
    }
    return nullptr;
  };
  for (size_t j = first_acc; j < c->logup.accs.size(); j++) {
    const LogupAcc& a = c->logup.accs[j];
    if (first_acc + t->acc_begin.size() >= n_accs) break;
    t->acc_begin.push_back((uint32_t)t->words.size());
    for (const LogupFraction& f : a.fr) {
      t->words.push_back(f.table);
      R0H_TRY(form(f.num));
      t->words.push_back((uint32_t)f.parts.size());
      for (const LogupPart& q : f.parts) {
        uint32_t idx = 0;
        if (q.ch_kind) {
          const uint64_t key = (uint64_t)q.ch_kind << 32 | q.ch_idx;
          auto it = ch_index.find(key);
          if (it == ch_index.end()) {
            const uint32_t* src = q.ch_kind == 1 ? mix + 4 * (size_t)q.ch_idx : global + q.ch_idx;
            R0H_REQUIRE(q.ch_kind == 1 ? mix != nullptr : global != nullptr, "log-derivative accumulation: a challenge is read from %s and none were given", q.ch_kind == 1 ? "the mix" : "the public inputs");
            it = ch_index.emplace(key, (uint32_t)t->ch.size()).first;
            t->ch.push_back(Fp4{{src[0], src[1], src[2], src[3]}});
            t->ch_id.push_back(key);
          }
          idx = it->second;
        }
        t->words.push_back(idx);
        R0H_TRY(form(q.lf));
      }
    }
  }
  t->acc_begin.push_back((uint32_t)t->words.size());
  return nullptr;
}

struct DeviceTape {
  DevBuf buf;
  const uint32_t* words = nullptr;
  const uint32_t* const* cols = nullptr;
  const Fp4* ch = nullptr;
};
const char* upload_tape(r0h_ctx* ctx, const Tape& t, DeviceTape* d) {
  const size_t w_bytes = (t.words.size() * 4 + 15) & ~(size_t)15, c_bytes = (t.cols.size() * sizeof(void*) + 15) & ~(size_t)15, h_bytes = t.ch.size() * 16;
  R0H_TRY(d->buf.alloc(ctx, w_bytes + c_bytes + h_bytes));
  char* base = (char*)d->buf->ptr;
  R0H_TRY(stage_h2d(ctx, base, t.words.data(), t.words.size() * 4));
  R0H_TRY(stage_h2d(ctx, base + w_bytes, t.cols.data(), t.cols.size() * sizeof(void*)));
  R0H_TRY(stage_h2d(ctx, base + w_bytes + c_bytes, t.ch.data(), h_bytes));
  d->words = (const uint32_t*)base;
  d->cols = (const uint32_t* const*)(base + w_bytes);
  d->ch = (const Fp4*)(base + w_bytes + c_bytes);
  return nullptr;
}

__device__ __forceinline__ uint32_t eval_form(const uint32_t* __restrict__ tape, uint32_t& at, const uint32_t* const* __restrict__ cols, uint32_t r) {
  const uint32_t n = tape[at++];
  uint32_t acc = 0;
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t coef = tape[at], col = tape[at + 1];
    at += 2;
    acc = add(acc, col ? mul(coef, cols[col - 1][r]) : coef);
  }
  return acc;
}

// a form of the lookup list (circuit.hpp LookupList): columns are DATA column indices
__device__ __forceinline__ uint32_t eval_list_form(const uint32_t* __restrict__ list, uint32_t& at, const uint32_t* __restrict__ data, uint32_t po2, uint32_t r) {
  const uint32_t n = list[at++];
  uint32_t acc = 0;
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t coef = list[at], col = list[at + 1];
    at += 2;
    acc = add(acc, col ? mul(coef, data[((size_t)(col - 1) << po2) + r]) : coef);
  }
  return acc;
}

constexpr uint32_t BINS = 32768;         // one launch counts half a table: its whole value range is one LDS histogram (128 KB of the CU's 160)
constexpr uint32_t COUNT_THREADS = 1024;

// One launch per (table, half of its 65,536 values); a grid of at most one workgroup per CU, every workgroup striding over the rows.
// Every in-table lookup of this half is one LDS atomic, whatever its value; global memory sees the workgroup's flush alone: consecutive
// lanes add consecutive non-zero bins, at most BINS / 64 wave instructions per workgroup however many lookups there were.  A bin is a
// whole 32-bit word: it cannot overflow, for all the bins of a table together hold at most its lookup slots, which the caller has
// refused above p - 1 < 2^31 (at po2 = 24 with the trace circuit's 24 lookups a row: 24 * 2^24 < 2^29).  Zero is not counted (entry 0
// is the remainder); counters[0] takes the lookups binned, counters[1] the slots gated off (half 0 counts those), one add per workgroup
// each.  A numerator other than 0 or 1 sets bit 0 of *err, a value outside its table (numerator 1) bit 1.  No workgroup waits for another.
__global__ __launch_bounds__(COUNT_THREADS) void logup_count_kernel(uint32_t* __restrict__ hist /* [65536], this table's */, uint32_t* __restrict__ counters, uint32_t* __restrict__ err,
                                                                    const uint32_t* __restrict__ list, uint32_t n_entries, const uint32_t* __restrict__ data, uint32_t po2,
                                                                    uint32_t half, uint32_t is_and) {
  __shared__ uint32_t bins[BINS];
  __shared__ uint32_t sums[2];
  for (uint32_t i = threadIdx.x; i < BINS; i += COUNT_THREADS) bins[i] = 0;
  if (threadIdx.x < 2) sums[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t n = 1u << po2, lo = half * BINS;
  uint32_t gated = 0, bad = 0;
  for (uint32_t r = blockIdx.x * COUNT_THREADS + threadIdx.x; r < n; r += gridDim.x * COUNT_THREADS) {
    uint32_t at = 0;
    for (uint32_t e = 0; e < n_entries; e++) {
      const uint32_t num = eval_list_form(list, at, data, po2, r);
      const uint32_t value = eval_list_form(list, at, data, po2, r);
      if (num != ONE) {
        if (num) bad |= 1u;
        else gated++;
        continue;
      }
      uint32_t v = dec(neg(value));
      if (is_and) {
        v -= R0H_TAG_AND;
        if (v >> 24 || ((v & 255u) & ((v >> 8) & 255u)) != v >> 16) { bad |= 2u; continue; }
        v &= 0xffffu;
      } else if (v >> 16) {
        bad |= 2u;
        continue;
      }
      if (v && v - lo < BINS) atomicAdd(&bins[v - lo], 1u);
    }
  }
  if (bad) atomicOr(err, bad);
  __syncthreads();
  uint32_t binned = 0;
  for (uint32_t i = threadIdx.x; i < BINS; i += COUNT_THREADS) {
    const uint32_t cnt = bins[i];
    if (cnt) atomicAdd(&hist[lo + i], cnt);
    binned += cnt;
  }
  if (binned) atomicAdd(&sums[0], binned);
  if (gated && half == 0) atomicAdd(&sums[1], gated);
  __syncthreads();
  if (threadIdx.x < 2 && sums[threadIdx.x]) atomicAdd(&counters[threadIdx.x], sums[threadIdx.x]);
}
// hist -> multiplicity column: entry 0 takes what the lookups binned and the slots gated off leave of `total` lookup slots
__global__ void logup_mult_kernel(uint32_t* __restrict__ column, const uint32_t* __restrict__ hist, const uint32_t* __restrict__ counters, uint32_t total, uint32_t n) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n) return;
  uint32_t v = r < 65536u ? hist[r] : 0u;
  if (r == 0) v = total - counters[0] - counters[1];
  column[r] = enc(v);
}

// one accumulator's four fractions at row r as one quotient: sum_f n_f / d_f = top / den
__device__ __forceinline__ void eval_accumulator(const uint32_t* __restrict__ tape, uint32_t& at, const uint32_t* const* __restrict__ cols, const Fp4* __restrict__ ch, uint32_t r,
                                                 Fp4& top, Fp4& den_out) {
  Fp4 d[4];
  uint32_t num[4];
#pragma unroll
  for (uint32_t f = 0; f < 4; f++) {
    at++;  // table
    num[f] = eval_form(tape, at, cols, r);
    const uint32_t n_parts = tape[at++];
    Fp4 den = fp4_zero();
    for (uint32_t q = 0; q < n_parts; q++) {
      const uint32_t ci = tape[at++];
      const uint32_t v = eval_form(tape, at, cols, r);
      if (ci == 0) den.e[0] = add(den.e[0], v);
      else den = den + scale(ch[ci], v);
    }
    d[f] = den;
  }
  const Fp4 d01 = d[0] * d[1], d23 = d[2] * d[3];
  top = (scale(d[1], num[0]) + scale(d[0], num[1])) * d23 + (scale(d[3], num[2]) + scale(d[2], num[3])) * d01;
  den_out = d01 * d23;
}
// accumulators [j, j + NB) of the row with one inversion between them (fp4_batch_div); NB is a compile-time count: no array is indexed
// by a run-time value, so all of it stays in registers
template <int NB>
__device__ __forceinline__ void term_batch(uint32_t* __restrict__ accum, uint32_t* __restrict__ own_terms, const uint32_t* __restrict__ tape, uint32_t& at,
                                           const uint32_t* const* __restrict__ cols, const Fp4* __restrict__ ch, uint32_t j, uint32_t n_chain, uint32_t po2, uint32_t r, Fp4& run) {
  Fp4 top[NB], den[NB];
  eval_accumulator(tape, at, cols, ch, r, top[0], den[0]);  // (spelled out: the compiler declines to unroll a loop over a body this size)
  if constexpr (NB > 1) eval_accumulator(tape, at, cols, ch, r, top[1], den[1]);
  if constexpr (NB > 2) eval_accumulator(tape, at, cols, ch, r, top[2], den[2]);
  if constexpr (NB > 3) eval_accumulator(tape, at, cols, ch, r, top[3], den[3]);
  static_assert(NB >= 1 && NB <= 4, "batches of one to four accumulators");
  fp4_batch_div<NB>(top, den);
#pragma unroll
  for (int k = 0; k < NB; k++) {
    const Fp4 term = top[k];
    if (j + k < n_chain) {
      run = run + term;
      for (uint32_t i = 0; i < 4; i++) accum[((size_t)(4 * (j + k) + i) << po2) + r] = run.e[i];
    } else {
      *(uint4*)(own_terms + 4 * (((size_t)(j + k - n_chain) << po2) + r)) = make_uint4(term.e[0], term.e[1], term.e[2], term.e[3]);
    }
  }
}
// the row's fractions, accumulators [a0, a1), in batches of up to four: chain links leave their running sum within the row in the ACCUM
// columns and the row total in `row_total`; an accumulator with a public total leaves its term in its own scan buffer
__global__ __launch_bounds__(256) void logup_term_kernel(uint32_t* __restrict__ accum, uint32_t* __restrict__ row_total, uint32_t* __restrict__ own_terms,
                                                         const uint32_t* __restrict__ tape, const uint32_t* const* __restrict__ cols, const Fp4* __restrict__ ch,
                                                         uint32_t a0, uint32_t a1, uint32_t n_chain, uint32_t po2) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x, n = 1u << po2;
  if (r >= n) return;
  uint32_t at = 0;
  Fp4 run = fp4_zero();
  uint32_t j = a0;
  for (; j + 4 <= a1; j += 4) term_batch<4>(accum, own_terms, tape, at, cols, ch, j, n_chain, po2, r, run);
  if (a1 - j == 3) term_batch<3>(accum, own_terms, tape, at, cols, ch, j, n_chain, po2, r, run);
  else if (a1 - j == 2) term_batch<2>(accum, own_terms, tape, at, cols, ch, j, n_chain, po2, r, run);
  else if (a1 - j == 1) term_batch<1>(accum, own_terms, tape, at, cols, ch, j, n_chain, po2, r, run);
  if (a0 < n_chain) *(uint4*)(row_total + 4 * (size_t)r) = make_uint4(run.e[0], run.e[1], run.e[2], run.e[3]);
}
// chain links: add the sum of all earlier rows (inclusive scan of the row totals, one row back)
__global__ void logup_chain_kernel(uint32_t* __restrict__ accum, const uint32_t* __restrict__ scanned, uint32_t n_cols, uint32_t po2) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x, col = blockIdx.y;
  if (r == 0 || r >= (1u << po2) || col >= n_cols) return;
  uint32_t* cell = accum + ((size_t)col << po2) + r;
  *cell = add(*cell, scanned[4 * (size_t)(r - 1) + (col & 3u)]);
}
// ---- the balance check of the chain links (r0h_logup_check_balance, include/r0hip.h): every fraction with a non-zero numerator is a
// tuple, its class the denominator as a polynomial in the challenges, told apart by balance_key (circuit.hpp).  Classes meet in an
// open-addressed table in global memory -- one 64-bit compare-and-swap claims a slot, then a sum, a count and a minimum, all atomics
// at device scope, so the table's CONTENT does not depend on scheduling (where a class sits does; the host orders what it reads
// back) -- behind a table of the same shape in LDS that takes every insert of its workgroup first: on a real trace most lookup slots
// ask for value 0, one class of tens of millions of members, which without that stage would all meet in one global slot
// (profiles/r05/logup_before.md, for the multiplicity count).  No workgroup waits for another, every probe sequence is bounded by its
// table's size, and what the scan reads is complete by the kernel boundary alone.
struct BalanceSlot {
  unsigned long long key;        // 0: empty
  unsigned long long sum;        // of the canonical numerators
  unsigned long long first_inv;  // ~(row << 32 | fraction) of the lowest member: a maximum, so that an all-zero table is an empty one
  uint32_t members, pad;
};
static_assert(sizeof(BalanceSlot) == 32, "a slot is half a 64-byte line");
constexpr uint32_t BAL_THREADS = 1024;
constexpr uint32_t BAL_LDS_BITS = 12, BAL_LDS_SLOTS = 1u << BAL_LDS_BITS;  // 4,096 classes a workgroup: 112 KB of the CU's 160
constexpr uint32_t BAL_LDS_PROBES = 8;
constexpr unsigned long long BAL_SPREAD = 0x9E3779B97F4A7C15ull;
enum { BAL_TUPLES = 0, BAL_GLOBAL_INSERTS, BAL_IMBALANCED, BAL_FIRST_INV, BAL_ERR, BAL_CURSOR, BAL_COUNTERS };

__device__ __forceinline__ void balance_global_insert(BalanceSlot* __restrict__ table, uint32_t slot_bits, unsigned long long* __restrict__ ctr, unsigned long long key,
                                                      unsigned long long sum, uint32_t members, unsigned long long first_inv) {
  const unsigned long long mask = (1ull << slot_bits) - 1;
  unsigned long long i = (key * BAL_SPREAD) >> (64 - slot_bits);
  for (unsigned long long probe = 0; probe <= mask; probe++) {  // (at a load of 1/2 or less: a handful)
    BalanceSlot* s = table + i;
    const unsigned long long prev = atomicCAS(&s->key, 0ull, key);
    if (prev == 0ull || prev == key) {
      atomicAdd(&s->sum, sum);
      atomicAdd(&s->members, members);
      atomicMax(&s->first_inv, first_inv);
      return;
    }
    i = (i + 1) & mask;
  }
  atomicOr(&ctr[BAL_ERR], 1ull);  // every slot is another class's: the caller reports "table full"
}

// the tuples there are: what the table is sized from.  The numerators alone are evaluated; the parts are stepped over.
__global__ __launch_bounds__(BAL_THREADS) void balance_count_kernel(unsigned long long* __restrict__ ctr, const uint32_t* __restrict__ tape, const uint32_t* const* __restrict__ cols,
                                                                    uint32_t n_acc, uint32_t po2) {
  __shared__ unsigned long long total;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  const uint32_t n = 1u << po2;
  uint32_t count = 0;
  for (uint32_t r = blockIdx.x * BAL_THREADS + threadIdx.x; r < n; r += gridDim.x * BAL_THREADS) {
    uint32_t at = 0;
    for (uint32_t f = 0; f < 4 * n_acc; f++) {
      at++;  // table
      count += eval_form(tape, at, cols, r) != 0u;
      const uint32_t n_parts = tape[at++];
      for (uint32_t q = 0; q < n_parts; q++) {
        const uint32_t n_terms = tape[at + 1];
        at += 2 + 2 * n_terms;
      }
    }
  }
  if (count) atomicAdd(&total, (unsigned long long)count);
  __syncthreads();
  if (threadIdx.x == 0 && total) atomicAdd(&ctr[BAL_TUPLES], total);
}

// A grid of at most one workgroup per CU strides over the rows, a lane per row.  Every fraction's parts are evaluated whatever its
// numerator (the tape position stays uniform across the wave: scalar loads); a numerator of zero inserts nothing.
__global__ __launch_bounds__(BAL_THREADS) void balance_insert_kernel(BalanceSlot* __restrict__ table, uint32_t slot_bits, unsigned long long* __restrict__ ctr,
                                                                     const uint32_t* __restrict__ tape, const uint32_t* const* __restrict__ cols,
                                                                     const uint32_t* __restrict__ weights /* [2][n_ch] */, uint32_t n_ch, uint32_t n_acc, uint32_t po2) {
  __shared__ unsigned long long l_key[BAL_LDS_SLOTS], l_sum[BAL_LDS_SLOTS], l_first[BAL_LDS_SLOTS];
  __shared__ uint32_t l_members[BAL_LDS_SLOTS];
  __shared__ uint32_t l_used;
  __shared__ unsigned long long l_sent;
  for (uint32_t i = threadIdx.x; i < BAL_LDS_SLOTS; i += BAL_THREADS) {
    l_key[i] = 0;
    l_sum[i] = 0;
    l_first[i] = 0;
    l_members[i] = 0;
  }
  if (threadIdx.x == 0) {
    l_used = 0;
    l_sent = 0;
  }
  __syncthreads();
  const uint32_t n = 1u << po2;
  uint32_t sent = 0;  // inserts of this lane into the global table
  for (uint32_t base = blockIdx.x * BAL_THREADS; base < n; base += gridDim.x * BAL_THREADS) {  // uniform across the workgroup: it meets at barriers
    const uint32_t r = base + threadIdx.x;
    if (r < n) {
      uint32_t at = 0;
      for (uint32_t f = 0; f < 4 * n_acc; f++) {
        at++;  // table
        const uint32_t num = eval_form(tape, at, cols, r);
        const uint32_t n_parts = tape[at++];
        uint32_t h0 = 0, h1 = 0;
        for (uint32_t q = 0; q < n_parts; q++) {
          const uint32_t ci = tape[at++];
          const uint32_t v = eval_form(tape, at, cols, r);
          h0 = add(h0, mul(weights[ci], v));
          h1 = add(h1, mul(weights[n_ch + ci], v));
        }
        if (!num) continue;
        const unsigned long long key = balance_key(h0, h1), value = dec(num), first_inv = ~((unsigned long long)r << 32 | f);
        uint32_t i = (uint32_t)((key * BAL_SPREAD) >> (64 - BAL_LDS_BITS));
        bool placed = false;
        for (uint32_t probe = 0; probe < BAL_LDS_PROBES && !placed; probe++) {
          const unsigned long long prev = atomicCAS(&l_key[i], 0ull, key);
          if (prev == 0ull) atomicAdd(&l_used, 1u);
          if (prev == 0ull || prev == key) {
            atomicAdd(&l_sum[i], value);
            atomicAdd(&l_members[i], 1u);
            atomicMax(&l_first[i], first_inv);
            placed = true;
          }
          i = (i + 1) & (BAL_LDS_SLOTS - 1);
        }
        if (!placed) {  // the workgroup's table is full hereabouts: straight to the global one
          balance_global_insert(table, slot_bits, ctr, key, value, 1u, first_inv);
          sent++;
        }
      }
    }
    __syncthreads();
    const bool full = l_used > BAL_LDS_SLOTS / 2;
    const bool last = base + gridDim.x * BAL_THREADS >= n;  // (n <= 2^24 rows and at most a workgroup per CU: no wrap)
    __syncthreads();
    if (full || last) {  // flushed when it fills, and once more at the end
      for (uint32_t i = threadIdx.x; i < BAL_LDS_SLOTS; i += BAL_THREADS) {
        if (!l_key[i]) continue;
        balance_global_insert(table, slot_bits, ctr, l_key[i], l_sum[i], l_members[i], l_first[i]);
        sent++;
        l_key[i] = 0;
        l_sum[i] = 0;
        l_first[i] = 0;
        l_members[i] = 0;
      }
      if (threadIdx.x == 0) l_used = 0;
      __syncthreads();
    }
  }
  if (sent) atomicAdd(&l_sent, (unsigned long long)sent);
  __syncthreads();
  if (threadIdx.x == 0 && l_sent) atomicAdd(&ctr[BAL_GLOBAL_INSERTS], l_sent);
}

// the classes whose numerators do not sum to zero: how many, and the lowest (row, fraction) among their first members
template <class Slot>
__global__ __launch_bounds__(256) void balance_scan_kernel(const Slot* __restrict__ table, unsigned long long slots, unsigned long long* __restrict__ ctr) {
  unsigned long long count = 0, best = 0;
  for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i < slots; i += gridDim.x * 256ull) {
    const Slot s = table[i];
    if (!s.key || s.sum % P == 0) continue;
    count++;
    best = s.first_inv > best ? s.first_inv : best;
  }
  if (count) {
    atomicAdd(&ctr[BAL_IMBALANCED], count);
    atomicMax(&ctr[BAL_FIRST_INV], best);
  }
}
// ... and the list of them: those whose first member is at or below `floor_inv` (inverted: at or above), `room` of them at the most
template <class Slot>
__global__ __launch_bounds__(256) void balance_compact_kernel(Slot* __restrict__ list, unsigned long long room, const Slot* __restrict__ table, unsigned long long slots,
                                                              unsigned long long floor_inv, unsigned long long* __restrict__ ctr) {
  for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i < slots; i += gridDim.x * 256ull) {
    const Slot s = table[i];
    if (!s.key || s.sum % P == 0 || s.first_inv < floor_inv) continue;
    const unsigned long long at = atomicAdd(&ctr[BAL_CURSOR], 1ull);
    if (at < room) list[at] = s;
  }
}
// ---- the session balance (r0h_session_balance_*, include/r0hip.h): the same definitions over the accumulators with a public total,
// whose tuples cancel across the segments of a session and against the verifier's side.  The table belongs to the handle and lives
// through its additions: a slot is one 64-byte line and also holds the class's per-identity sums, written by whoever claims it.
struct SessionSlot {
  unsigned long long key;        // 0: empty
  unsigned long long sum;        // of the canonical numerators
  unsigned long long first_inv;  // ~(source << 32 | row << 8 | fraction) of the lowest member
  uint32_t members, pad;
  uint32_t values[8];            // canonical per-identity sums (class-constant)
};
static_assert(sizeof(SessionSlot) == 64, "a slot is one 64-byte line");
enum { SES_OCCUPIED = BAL_COUNTERS, SES_COUNTERS };
constexpr uint32_t SES_THREADS = 256, SES_FIRST_BITS = 10;

// `occupied`: where a claim is counted (nullptr: a rehash, which moves classes and makes none)
__device__ __forceinline__ void session_insert(SessionSlot* __restrict__ table, uint32_t slot_bits, unsigned long long* __restrict__ ctr, unsigned long long* __restrict__ occupied,
                                               unsigned long long key, unsigned long long sum, uint32_t members, unsigned long long first_inv, const uint32_t (&vals)[8]) {
  const unsigned long long mask = (1ull << slot_bits) - 1;
  unsigned long long i = (key * BAL_SPREAD) >> (64 - slot_bits);
  for (unsigned long long probe = 0; probe <= mask; probe++) {  // bounded by the table's size (at a load of 1/2 or less: a handful)
    SessionSlot* s = table + i;
    const unsigned long long prev = atomicCAS(&s->key, 0ull, key);
    if (prev == 0ull) {  // the claimer alone writes the class's values, two to a word; the scan reads them after the kernel boundary.  Atomic
                         // exchanges, not plain stores: the line's other words are updated by device-scope atomics from every XCD
      unsigned long long* v = (unsigned long long*)&s->values[0];
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) atomicExch(&v[k], (unsigned long long)vals[2 * k + 1] << 32 | vals[2 * k]);
      if (occupied) atomicAdd(occupied, 1ull);
    }
    if (prev == 0ull || prev == key) {
      atomicAdd(&s->sum, sum);
      atomicAdd(&s->members, members);
      atomicMax(&s->first_inv, first_inv);
      return;
    }
    i = (i + 1) & mask;
  }
  atomicOr(&ctr[BAL_ERR], 1ull);  // every slot is another class's: the caller reports "table full"
}

// One lane per row, straight into the global table: no LDS stage as in balance_insert_kernel, for there is nothing to merge -- a
// session class has two or three members in the whole session (a producer, a consumer, perhaps the verifier's word), and almost every
// row has no session tuple at all (the boundary rows and the COMMIT rows have).  So the parts are evaluated on rows with a numerator
// only; the tape position after a fraction is stepped to from the tape alone and stays uniform across the wave.  No workgroup waits
// for another.
__global__ __launch_bounds__(SES_THREADS) void session_insert_kernel(SessionSlot* __restrict__ table, uint32_t slot_bits, unsigned long long* __restrict__ ctr,
                                                                     const uint32_t* __restrict__ tape, const uint32_t* const* __restrict__ cols,
                                                                     const uint32_t* __restrict__ weights /* [2][n_ids] */, const uint32_t* __restrict__ ch_to_id, uint32_t n_ids,
                                                                     uint32_t n_acc, uint32_t first_fraction, uint32_t source, uint32_t po2) {
  const uint32_t r = blockIdx.x * SES_THREADS + threadIdx.x;
  if (r >= (1u << po2)) return;
  uint32_t at = 0;
  for (uint32_t f = 0; f < 4 * n_acc; f++) {
    at++;  // table
    const uint32_t num = eval_form(tape, at, cols, r);
    const uint32_t n_parts = tape[at++];
    uint32_t next = at;
    for (uint32_t q = 0; q < n_parts; q++) next += 2 + 2 * tape[next + 1];
    if (num) {
      uint32_t a = at, vals[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (uint32_t q = 0; q < n_parts; q++) {
        const uint32_t id = ch_to_id[tape[a++]];
        const uint32_t v = eval_form(tape, a, cols, r);
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) vals[k] = id == k ? add(vals[k], v) : vals[k];  // (no array indexed by a run-time value: registers)
      }
      uint32_t h0 = 0, h1 = 0;
#pragma unroll
      for (uint32_t k = 0; k < 8; k++) {
        if (k < n_ids) {
          h0 = add(h0, mul(weights[k], vals[k]));
          h1 = add(h1, mul(weights[n_ids + k], vals[k]));
        }
        vals[k] = dec(vals[k]);
      }
      session_insert(table, slot_bits, ctr, &ctr[SES_OCCUPIED], balance_key(h0, h1), dec(num), 1u, ~session_first(source, r, first_fraction + f), vals);
    }
    at = next;
  }
}
// tuples from outside (r0h_session_balance_add_tuples): the host has formed their keys with the same balance_key
__global__ __launch_bounds__(SES_THREADS) void session_list_kernel(SessionSlot* __restrict__ table, uint32_t slot_bits, unsigned long long* __restrict__ ctr,
                                                                   const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ numerators,
                                                                   const uint32_t* __restrict__ values /* [n][n_ids] */, uint32_t n_ids, uint32_t source, uint32_t n) {
  const uint32_t i = blockIdx.x * SES_THREADS + threadIdx.x;
  if (i >= n || !numerators[i]) return;
  uint32_t vals[8];
#pragma unroll
  for (uint32_t k = 0; k < 8; k++) vals[k] = k < n_ids ? values[(size_t)i * n_ids + k] : 0u;
  session_insert(table, slot_bits, ctr, &ctr[SES_OCCUPIED], keys[i], numerators[i], 1u, ~session_first(source, i, SESSION_OUTSIDE_FRACTION), vals);
}
// growth: every occupied slot of the old table into the new one -- sum (reduced: only its residue counts), members, first member, values
__global__ __launch_bounds__(SES_THREADS) void session_rehash_kernel(SessionSlot* __restrict__ to, uint32_t to_bits, unsigned long long* __restrict__ ctr,
                                                                     const SessionSlot* __restrict__ from, unsigned long long from_slots) {
  for (unsigned long long i = blockIdx.x * (unsigned long long)SES_THREADS + threadIdx.x; i < from_slots; i += gridDim.x * (unsigned long long)SES_THREADS) {
    const SessionSlot s = from[i];
    if (!s.key) continue;
    session_insert(to, to_bits, ctr, nullptr, s.key, s.sum % P, s.members, s.first_inv, s.values);
  }
}
}  // namespace

// tests/test_gpu_logup_kept.py hands the two internal entry points an empty LogupKept of its own making: one pointer, then po2, then n_own
static_assert(sizeof(DevBuf) == sizeof(void*) && sizeof(LogupKept) == sizeof(void*) + 8 && alignof(LogupKept) == alignof(void*),
              "LogupKept is no longer {buffer pointer, po2, n_own}: tests/test_gpu_logup_kept.py builds one by hand");
// standalone accumulators: terms -> running sums; totals_out (host, 4 words each) if wanted, ACCUM columns if `accum`
// `keep`: the scanned terms outlive the call (the accumulation of the same segment unpacks them: logup_accum_kept)
static const char* own_accumulators(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const Tape& t, const DeviceTape& d, r0h_buf* accum, uint32_t* totals_out, LogupKept* keep = nullptr) {
  const uint32_t n = 1u << po2, n_chain = c->logup.n_chain, n_acc = (uint32_t)c->logup.accs.size(), n_own = n_acc - n_chain;
  if (!n_own) return nullptr;
  DevBuf terms;
  R0H_TRY(terms.alloc(ctx, (size_t)n_own * n * 16));
  hipLaunchKernelGGL(logup_term_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, accum ? u32(accum) : nullptr, (uint32_t*)nullptr, u32(terms.get()),
                     d.words + t.acc_begin[n_chain], d.cols, d.ch, n_chain, n_acc, n_chain, po2);
  R0H_TRY(launch_ok("logup_term_kernel"));
  for (uint32_t k = 0; k < n_own; k++) {
    r0h_buf view = buf_view(terms.get(), (size_t)k * n * 16, (size_t)n * 16);
    R0H_TRY(r0h_prefix_sums(ctx, &view, n));
    if (accum) R0H_TRY(unpack_ext_columns(ctx, u32(accum) + ((size_t)(4 * (n_chain + k)) << po2), (const uint32_t*)view.ptr, po2));
    if (totals_out) R0H_TRY(r0h_buf_d2h(ctx, &view, (size_t)(n - 1) * 16, totals_out + 4 * k, 16));
  }
  if (keep) {
    keep->terms = std::move(terms);
    keep->po2 = po2;
    keep->n_own = n_own;
  }
  return nullptr;
}

const char* logup_accum(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, const uint32_t* global, const uint32_t* mix, r0h_buf* accum) {
  return logup_accum_kept(ctx, c, po2, code, data, global, mix, accum, nullptr);
}

const char* logup_accum_kept(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, const uint32_t* global, const uint32_t* mix, r0h_buf* accum,
                             const LogupKept* kept) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && c && data && accum, "r0h_accum: NULL argument");
  R0H_REQUIRE(po2 >= 4 && po2 <= R0H_MAX_PO2, "r0h_accum: po2 %u outside [4, %u]", po2, R0H_MAX_PO2);
  const uint32_t n = 1u << po2, n_chain = c->logup.n_chain;
  R0H_REQUIRE(((size_t)c->group_size[R0H_GROUP_DATA] << po2) * 4 <= data->bytes && ((size_t)c->group_size[R0H_GROUP_ACCUM] << po2) * 4 <= accum->bytes &&
                  (!code || ((size_t)c->group_size[R0H_GROUP_CODE] << po2) * 4 <= code->bytes),
              "r0h_accum: buffers too small for 2^%u rows", po2);
  for (uint32_t i = 0; i < c->n_mix; i++) R0H_REQUIRE(mix && mix[i] < P, "r0h_accum: mix[%u] missing or not canonical", i);
  for (uint32_t i = 0; i < c->n_global; i++) R0H_REQUIRE(!global || global[i] < P, "r0h_accum: global[%u] not canonical", i);
  Tape t;
  R0H_TRY(build_tape(c, po2, code, data, global, mix, &t));
  DeviceTape d;
  R0H_TRY(upload_tape(ctx, t, &d));
  KScope ks(ctx, "logup_accum", ((double)t.cols.size() + 2.0 * c->group_size[R0H_GROUP_ACCUM]) * n * 4);
  DevBuf totals;
  R0H_TRY(totals.alloc(ctx, (size_t)n * 16));
  hipLaunchKernelGGL(logup_term_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, u32(accum), u32(totals.get()), (uint32_t*)nullptr, d.words, d.cols, d.ch, 0u, n_chain, n_chain, po2);
  R0H_TRY(launch_ok("logup_term_kernel"));
  R0H_TRY(r0h_prefix_sums(ctx, totals.get(), n));
  hipLaunchKernelGGL(logup_chain_kernel, dim3((n + 255) / 256, 4 * n_chain), dim3(256), 0, ctx->stream, u32(accum), u32(totals.get()), 4 * n_chain, po2);
  R0H_TRY(launch_ok("logup_chain_kernel"));
  if (kept && kept->terms) {  // the totals step of this segment has evaluated and scanned them (same columns, same public inputs)
    const uint32_t n_own = (uint32_t)c->logup.accs.size() - n_chain;
    R0H_REQUIRE(kept->po2 == po2 && kept->n_own == n_own && kept->terms->ctx == ctx, "r0h_accum: the kept terms are not this segment's (2^%u rows, %u accumulators)", kept->po2, kept->n_own);
    for (uint32_t k = 0; k < n_own; k++)
      R0H_TRY(unpack_ext_columns(ctx, u32(accum) + ((size_t)(4 * (n_chain + k)) << po2), u32(kept->terms.get()) + 4 * (size_t)k * n, po2));
  } else {
    R0H_TRY(own_accumulators(ctx, c, po2, t, d, accum, nullptr));
  }
  R0H_TRY_HIP(hipStreamSynchronize(ctx->stream));  // the tape goes back to the pool
  return nullptr;
  R0H_GUARD_END
}

}  // namespace r0h

using namespace r0h;

extern "C" {

// Fill the multiplicity columns of `data` from the lookups its rows make (before DATA is committed).
const char* r0h_logup_multiplicities(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, r0h_buf* data, const uint32_t* global) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && c && data, "r0h_logup_multiplicities: NULL argument");
  if (c->logup.tables.empty()) return nullptr;
  R0H_REQUIRE(po2 >= 16 && po2 <= R0H_MAX_PO2, "r0h_logup_multiplicities: the tables have 2^16 rows: po2 %u outside [16, %u]", po2, R0H_MAX_PO2);
  R0H_REQUIRE(((size_t)c->group_size[R0H_GROUP_DATA] << po2) * 4 <= data->bytes, "r0h_logup_multiplicities: the DATA buffer is too small for 2^%u rows", po2);
  R0H_REQUIRE(c->logup.tables.size() <= 2, "r0h_logup_multiplicities: at most two tables");
  const uint32_t n = 1u << po2, n_tables = (uint32_t)c->logup.tables.size();
  LookupList list;  // the lookups alone, table by table: numerator and value (they read DATA only)
  R0H_TRY(logup_lookup_list(c, global, &list));
  std::vector<uint64_t> slots(n_tables, 0);  // lookup slots of each table: the chain links' lookups times the rows (only links look up)
  for (uint32_t k = 0; k < n_tables; k++) slots[k] = (uint64_t)list.entries[k] * n;
  for (uint32_t k = 0; k < n_tables; k++)
    R0H_REQUIRE(slots[k] <= P - 1, "r0h_logup_multiplicities: table %u has %llu lookup slots at 2^%u rows: more than p - 1", k, (unsigned long long)slots[k], po2);
  DevBuf dlist;
  R0H_TRY(dlist.alloc(ctx, list.words.size() * 4 + 16));
  R0H_TRY(stage_h2d(ctx, dlist->ptr, list.words.data(), list.words.size() * 4));
  DevBuf hist;  // [n_tables][65536] counts, then per table the lookups binned and the slots gated off, then the error word
  const size_t hist_words = (size_t)n_tables * 65536;
  R0H_TRY(hist.alloc(ctx, hist_words * 4 + 32));
  R0H_TRY_HIP(hipMemsetAsync(hist->ptr, 0, hist_words * 4 + 32, ctx->stream));
  uint32_t* const counters = u32(hist.get()) + hist_words;
  uint32_t* const err_word = counters + 4;
  if (!ctx->n_cu) R0H_TRY_HIP(hipDeviceGetAttribute(&ctx->n_cu, hipDeviceAttributeMultiprocessorCount, ctx->device));
  const uint32_t grid = std::min<uint32_t>((uint32_t)std::max(ctx->n_cu, 1), n / COUNT_THREADS);  // persistent: a workgroup per CU, fewer where the rows do not fill them
  KScope ks(ctx, "logup_multiplicities", 2.0 * list.n_cols * n * 4);  // (each half's launch reads the lookups' columns)
  for (uint32_t k = 0; k < n_tables; k++) {
    for (uint32_t half = 0; half < 2; half++) {
      hipLaunchKernelGGL(logup_count_kernel, dim3(grid), dim3(COUNT_THREADS), 0, ctx->stream, u32(hist.get()) + (size_t)k * 65536, counters + 2 * k, err_word, u32(dlist.get()) + list.begin[k],
                         list.entries[k], u32(data), po2, half, (uint32_t)(k + 1 == R0H_TABLE_AND));
      R0H_TRY(launch_ok("logup_count_kernel"));
    }
    const LogupTable& tb = c->logup.tables[k];
    hipLaunchKernelGGL(logup_mult_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, u32(data) + ((size_t)tb.data_col << po2), u32(hist.get()) + (size_t)k * 65536, counters + 2 * k,
                       (uint32_t)slots[k], n);
    R0H_TRY(launch_ok("logup_mult_kernel"));
  }
  R0H_TRY_HIP(hipStreamSynchronize(ctx->stream));
  uint32_t err = 0;
  R0H_TRY(r0h_buf_d2h(ctx, hist.get(), hist_words * 4 + 16, &err, 4));
  R0H_REQUIRE(!(err & 1u), "r0h_logup_multiplicities: a lookup's numerator is neither 0 nor 1");
  R0H_REQUIRE(!(err & 2u), "r0h_logup_multiplicities: a row whose numerator is 1 looks up a value that is not in its table");
  return nullptr;
  R0H_GUARD_END
}

// Which classes of the chain links' fractions do not cancel (include/r0hip.h).  Reads DATA, CODE and the public inputs: no mix.
const char* r0h_logup_check_balance(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, const uint32_t* global, r0h_imbalance* out,
                                    size_t capacity, size_t* n_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && c && data && n_out && (out || !capacity), "r0h_logup_check_balance: NULL argument");
  R0H_REQUIRE(po2 >= 4 && po2 <= R0H_MAX_PO2, "r0h_logup_check_balance: po2 %u outside [4, %u]", po2, R0H_MAX_PO2);
  *n_out = 0;
  const uint32_t n = 1u << po2, n_chain = c->logup.n_chain;
  if (!n_chain) return nullptr;
  R0H_REQUIRE(((size_t)c->group_size[R0H_GROUP_DATA] << po2) * 4 <= data->bytes && (!code || ((size_t)c->group_size[R0H_GROUP_CODE] << po2) * 4 <= code->bytes),
              "r0h_logup_check_balance: buffers too small for 2^%u rows", po2);
  R0H_REQUIRE(((uint64_t)(4 * n_chain) << po2) <= 0xffffffffull, "r0h_logup_check_balance: %u fractions on 2^%u rows: more than 2^32 - 1 tuples", 4 * n_chain, po2);
  for (uint32_t i = 0; i + c->n_late < c->n_global; i++) R0H_REQUIRE(!global || global[i] < P, "r0h_logup_check_balance: global[%u] not canonical", i);
  Tape t;
  std::vector<uint32_t> dummy_mix(c->n_mix, 0);  // the challenges' values are not read, their identities are
  R0H_TRY(build_tape(c, po2, code, data, global, dummy_mix.data(), &t, n_chain));
  DeviceTape d;
  R0H_TRY(upload_tape(ctx, t, &d));
  const uint32_t n_ch = (uint32_t)t.ch.size();
  std::vector<uint32_t> weights(2 * (size_t)n_ch);
  for (uint32_t j = 0; j < 2; j++)
    for (uint32_t k = 0; k < n_ch; k++) weights[(size_t)j * n_ch + k] = balance_weight(j, t.ch_id[k]);
  DevBuf side;  // the counters, then the two weight rows
  R0H_TRY(side.alloc(ctx, BAL_COUNTERS * 8 + weights.size() * 4));
  unsigned long long* const ctr = (unsigned long long*)side->ptr;
  const uint32_t* const d_weights = (const uint32_t*)(ctr + BAL_COUNTERS);
  R0H_TRY_HIP(hipMemsetAsync(ctr, 0, BAL_COUNTERS * 8, ctx->stream));
  R0H_TRY(stage_h2d(ctx, (void*)d_weights, weights.data(), weights.size() * 4));
  if (!ctx->n_cu) R0H_TRY_HIP(hipDeviceGetAttribute(&ctx->n_cu, hipDeviceAttributeMultiprocessorCount, ctx->device));
  const uint32_t grid = std::min<uint32_t>((uint32_t)std::max(ctx->n_cu, 1), (n + BAL_THREADS - 1) / BAL_THREADS);  // persistent: a workgroup per CU, fewer where the rows do not fill them
  KScope ks(ctx, "logup_check_balance", 2.0 * t.cols.size() * n * 4);
  hipLaunchKernelGGL(balance_count_kernel, dim3(grid), dim3(BAL_THREADS), 0, ctx->stream, ctr, d.words, d.cols, n_chain, po2);
  R0H_TRY(launch_ok("balance_count_kernel"));
  unsigned long long counters[BAL_COUNTERS];
  R0H_TRY(r0h_buf_d2h(ctx, side.get(), 0, counters, sizeof counters));
  const uint64_t tuples = counters[BAL_TUPLES];
  ctx->balance_stats[0] = tuples;
  ctx->balance_stats[1] = ctx->balance_stats[2] = 0;
  if (!tuples) return nullptr;
  uint32_t slot_bits = 10;  // a load of 1/2 at the most (every tuple a class of its own), and no table smaller than 1,024 slots
  while ((1ull << slot_bits) < 2 * tuples) slot_bits++;
  const uint64_t slots = 1ull << slot_bits;
  DevBuf table;
  R0H_TRY(table.alloc(ctx, slots * sizeof(BalanceSlot)));  // (an allocation the device refuses is this call's error)
  R0H_TRY_HIP(hipMemsetAsync(table->ptr, 0, slots * sizeof(BalanceSlot), ctx->stream));
  BalanceSlot* const d_table = (BalanceSlot*)table->ptr;
  hipLaunchKernelGGL(balance_insert_kernel, dim3(grid), dim3(BAL_THREADS), 0, ctx->stream, d_table, slot_bits, ctr, d.words, d.cols, d_weights, n_ch, n_chain, po2);
  R0H_TRY(launch_ok("balance_insert_kernel"));
  const uint32_t scan_grid = (uint32_t)std::min<uint64_t>((slots + 255) / 256, 8ull * (uint32_t)std::max(ctx->n_cu, 1));
  hipLaunchKernelGGL(balance_scan_kernel<BalanceSlot>, dim3(scan_grid), dim3(256), 0, ctx->stream, d_table, (unsigned long long)slots, ctr);
  R0H_TRY(launch_ok("balance_scan_kernel"));
  R0H_TRY(r0h_buf_d2h(ctx, side.get(), 0, counters, sizeof counters));
  ctx->balance_stats[1] = counters[BAL_GLOBAL_INSERTS];
  ctx->balance_stats[2] = slots;
  R0H_REQUIRE(!counters[BAL_ERR], "r0h_logup_check_balance: table full");
  const uint64_t n_bad = counters[BAL_IMBALANCED];
  *n_out = (size_t)n_bad;
  if (!n_bad || !capacity) return nullptr;
  // the `capacity` lowest: one wanted of many is the minimum the scan has found; otherwise all of them come back and are ordered here
  const bool lowest_only = capacity == 1 && n_bad > 1;
  const uint64_t room = lowest_only ? 1 : n_bad;
  DevBuf list;
  R0H_TRY(list.alloc(ctx, room * sizeof(BalanceSlot)));
  hipLaunchKernelGGL(balance_compact_kernel<BalanceSlot>, dim3(scan_grid), dim3(256), 0, ctx->stream, (BalanceSlot*)list->ptr, (unsigned long long)room, d_table, (unsigned long long)slots,
                     lowest_only ? counters[BAL_FIRST_INV] : 0ull, ctr);
  R0H_TRY(launch_ok("balance_compact_kernel"));
  std::vector<BalanceSlot> found(room);
  R0H_TRY(r0h_buf_d2h(ctx, list.get(), 0, found.data(), room * sizeof(BalanceSlot)));
  std::sort(found.begin(), found.end(), [](const BalanceSlot& a, const BalanceSlot& b) { return a.first_inv > b.first_inv; });
  for (size_t k = 0; k < found.size() && k < capacity; k++) {
    const uint64_t first = ~found[k].first_inv;
    out[k] = r0h_imbalance{(uint32_t)first, (uint32_t)(first >> 32), (uint32_t)(found[k].sum % P), found[k].members};
  }
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_logup_check_balance_stats(const r0h_ctx* ctx, uint64_t stats_out[3]) {
  R0H_REQUIRE(ctx && stats_out, "r0h_logup_check_balance_stats: NULL argument");
  for (int k = 0; k < 3; k++) stats_out[k] = ctx->balance_stats[k];
  return nullptr;
}

const char* r0h_ctx_set_check_balance(r0h_ctx* ctx, int on) {
  R0H_REQUIRE(ctx, "r0h_ctx_set_check_balance: ctx is NULL");
  ctx->check_balance = on != 0;
  for (r0h_ctx* h : ctx->helpers) h->check_balance = ctx->check_balance;
  return nullptr;
}

// The totals of the accumulators that run alone (their challenges are public inputs, so they can be had before the mix is drawn):
// global_io[final .. final + 4) of each is overwritten with its total over the rows.
const char* r0h_logup_totals(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, uint32_t* global_io) {
  return logup_totals_keep(ctx, c, po2, code, data, global_io, nullptr);
}

}  // extern "C"

const char* r0h::require_balance(const char* caller, r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, const uint32_t* global) {
  r0h_imbalance first = {0, 0, 0, 0};
  size_t n_bad = 0;
  R0H_TRY(r0h_logup_check_balance(ctx, c, po2, code, data, global, &first, 1, &n_bad));
  R0H_REQUIRE(!n_bad, "%s: fraction %u does not balance: net %u over %u tuples, first at row %u; %zu classes in all", caller, first.fraction, first.net, first.members, first.first_row, n_bad);
  return nullptr;
}

const char* r0h::logup_totals_keep(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, uint32_t* global_io, LogupKept* keep) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && c && data && global_io, "r0h_logup_totals: NULL argument");
  R0H_REQUIRE(po2 >= 4 && po2 <= R0H_MAX_PO2, "r0h_logup_totals: po2 %u outside [4, %u]", po2, R0H_MAX_PO2);
  const uint32_t n_chain = c->logup.n_chain, n_acc = (uint32_t)c->logup.accs.size();
  if (n_acc == n_chain) return nullptr;
  for (uint32_t j = n_chain; j < n_acc; j++)
    for (const LogupFraction& f : c->logup.accs[j].fr)
      for (const LogupPart& q : f.parts) R0H_REQUIRE(q.ch_kind != 1, "r0h_logup_totals: accumulator %u takes a challenge from the mix", j);
  Tape t;
  std::vector<uint32_t> dummy_mix(c->n_mix, 0);
  R0H_TRY(build_tape(c, po2, code ? code : data, data, global_io, dummy_mix.data(), &t));
  DeviceTape d;
  R0H_TRY(upload_tape(ctx, t, &d));
  std::vector<uint32_t> totals(4 * (size_t)(n_acc - n_chain));
  R0H_TRY(own_accumulators(ctx, c, po2, t, d, nullptr, totals.data(), keep));
  for (uint32_t j = n_chain; j < n_acc; j++) memcpy(global_io + c->logup.accs[j].final_global, totals.data() + 4 * (size_t)(j - n_chain), 16);
  return nullptr;
  R0H_GUARD_END
}

// ---- the session balance's device half (the handle and everything that needs no device: logup_host.cpp)
struct r0h::SessionTable {
  DevBuf side;   // SES_COUNTERS counters, then the two weight rows
  DevBuf table;  // 2^slot_bits slots
  uint32_t slot_bits = SES_FIRST_BITS;
  unsigned long long* ctr() const { return (unsigned long long*)side->ptr; }
  const uint32_t* weights() const { return (const uint32_t*)(ctr() + SES_COUNTERS); }
  SessionSlot* slots() const { return (SessionSlot*)table->ptr; }
};

namespace {
const char* session_table_ensure(r0h_session_balance* sb) {
  if (sb->table) return nullptr;
  r0h_ctx* ctx = sb->ctx;
  std::unique_ptr<SessionTable> t(new SessionTable());
  R0H_TRY(t->side.alloc(ctx, SES_COUNTERS * 8 + sb->weights.size() * 4 + 16));
  R0H_TRY_HIP(hipMemsetAsync(t->side->ptr, 0, SES_COUNTERS * 8, ctx->stream));
  if (!sb->weights.empty()) R0H_TRY(stage_h2d(ctx, (void*)t->weights(), sb->weights.data(), sb->weights.size() * 4));
  R0H_TRY(t->table.alloc(ctx, sizeof(SessionSlot) << t->slot_bits));
  R0H_TRY_HIP(hipMemsetAsync(t->table->ptr, 0, sizeof(SessionSlot) << t->slot_bits, ctx->stream));
  if (!ctx->n_cu) R0H_TRY_HIP(hipDeviceGetAttribute(&ctx->n_cu, hipDeviceAttributeMultiprocessorCount, ctx->device));
  sb->table = t.release();
  return nullptr;
}
// slots >= 2 x the tuples there will be: the next power of two that holds them, every occupied slot re-inserted, the old table released
const char* session_table_grow(r0h_session_balance* sb, uint64_t tuples) {
  SessionTable* t = sb->table;
  r0h_ctx* ctx = sb->ctx;
  uint32_t bits = t->slot_bits;
  while ((1ull << bits) < 2 * tuples) bits++;
  if (bits == t->slot_bits) return nullptr;
  DevBuf bigger;
  R0H_TRY(bigger.alloc(ctx, sizeof(SessionSlot) << bits));  // (an allocation the device refuses is this call's error)
  R0H_TRY_HIP(hipMemsetAsync(bigger->ptr, 0, sizeof(SessionSlot) << bits, ctx->stream));
  const unsigned long long from_slots = 1ull << t->slot_bits;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((from_slots + SES_THREADS - 1) / SES_THREADS, 8ull * (uint32_t)std::max(ctx->n_cu, 1));
  hipLaunchKernelGGL(session_rehash_kernel, dim3(grid), dim3(SES_THREADS), 0, ctx->stream, (SessionSlot*)bigger->ptr, bits, t->ctr(), t->slots(), from_slots);
  R0H_TRY(launch_ok("session_rehash_kernel"));
  R0H_TRY_HIP(hipStreamSynchronize(ctx->stream));  // the old table goes back to the pool
  t->table = std::move(bigger);
  t->slot_bits = bits;
  sb->grows++;
  return nullptr;
}
// after the inserts of one addition: they are complete, and none ran out of slots
const char* session_table_settle(r0h_session_balance* sb) {
  unsigned long long err = 0;
  R0H_TRY(r0h_buf_d2h(sb->ctx, sb->table->side.get(), BAL_ERR * 8, &err, 8));
  R0H_REQUIRE(!err, "r0h_session_balance: table full");
  return nullptr;
}
}  // namespace

void r0h::session_table_free(r0h_session_balance* sb) {
  delete sb->table;
  sb->table = nullptr;
}

const char* r0h::session_table_stats(r0h_session_balance* sb, uint64_t* slots_out, uint64_t* occupied_out) {
  KScope ks(sb->ctx, "session_balance", 0);
  R0H_TRY(session_table_ensure(sb));
  unsigned long long occupied = 0;
  R0H_TRY(r0h_buf_d2h(sb->ctx, sb->table->side.get(), SES_OCCUPIED * 8, &occupied, 8));
  *slots_out = 1ull << sb->table->slot_bits;
  *occupied_out = occupied;
  return nullptr;
}

const char* r0h::session_table_add_list(r0h_session_balance* sb, uint32_t source, const uint64_t* keys, const uint32_t* numerators, const uint32_t* values, size_t n) {
  r0h_ctx* ctx = sb->ctx;
  const uint32_t n_ids = (uint32_t)sb->ids.size();
  KScope ks(ctx, "session_balance", (double)n * (12 + 4 * n_ids));
  R0H_TRY(session_table_ensure(sb));
  uint64_t tuples = 0;
  for (size_t i = 0; i < n; i++) tuples += numerators[i] != 0;
  R0H_TRY(session_table_grow(sb, sb->tuples + tuples));
  const size_t k_bytes = n * 8, n_bytes = (n * 4 + 15) & ~(size_t)15, v_bytes = n * n_ids * 4;
  DevBuf list;  // keys, numerators, values
  R0H_TRY(list.alloc(ctx, k_bytes + n_bytes + v_bytes));
  char* base = (char*)list->ptr;
  R0H_TRY(r0h_buf_h2d(ctx, list.get(), 0, keys, k_bytes));
  R0H_TRY(r0h_buf_h2d(ctx, list.get(), k_bytes, numerators, n * 4));
  R0H_TRY(r0h_buf_h2d(ctx, list.get(), k_bytes + n_bytes, values, v_bytes));
  SessionTable* t = sb->table;
  hipLaunchKernelGGL(session_list_kernel, dim3((uint32_t)((n + SES_THREADS - 1) / SES_THREADS)), dim3(SES_THREADS), 0, ctx->stream, t->slots(), t->slot_bits, t->ctr(),
                     (const unsigned long long*)base, (const uint32_t*)(base + k_bytes), (const uint32_t*)(base + k_bytes + n_bytes), n_ids, source, (uint32_t)n);
  R0H_TRY(launch_ok("session_list_kernel"));
  return session_table_settle(sb);  // (synchronises: the list goes back to the pool)
}

const char* r0h::session_table_report(r0h_session_balance* sb, r0h_session_imbalance* out, size_t capacity, size_t* n_out) {
  r0h_ctx* ctx = sb->ctx;
  *n_out = 0;
  if (!sb->table) return nullptr;  // nothing was added
  SessionTable* t = sb->table;
  const uint64_t slots = 1ull << t->slot_bits;
  KScope ks(ctx, "session_balance", (double)slots * sizeof(SessionSlot));
  unsigned long long* const ctr = t->ctr();
  R0H_TRY_HIP(hipMemsetAsync(ctr + BAL_IMBALANCED, 0, 16, ctx->stream));  // ... and BAL_FIRST_INV: a report starts from nothing
  R0H_TRY_HIP(hipMemsetAsync(ctr + BAL_CURSOR, 0, 8, ctx->stream));
  static_assert(BAL_FIRST_INV == BAL_IMBALANCED + 1, "the two counters of a scan are cleared together");
  // scan and compaction as the chain's check has them; the host orders what comes back
  const uint32_t scan_grid = (uint32_t)std::min<uint64_t>((slots + 255) / 256, 8ull * (uint32_t)std::max(ctx->n_cu, 1));
  hipLaunchKernelGGL(balance_scan_kernel<SessionSlot>, dim3(scan_grid), dim3(256), 0, ctx->stream, t->slots(), (unsigned long long)slots, ctr);
  R0H_TRY(launch_ok("balance_scan_kernel"));
  unsigned long long counters[BAL_COUNTERS];
  R0H_TRY(r0h_buf_d2h(ctx, t->side.get(), 0, counters, sizeof counters));
  R0H_REQUIRE(!counters[BAL_ERR], "r0h_session_balance: table full");
  const uint64_t n_bad = counters[BAL_IMBALANCED];
  *n_out = (size_t)n_bad;
  if (!n_bad || !capacity) return nullptr;
  const bool lowest_only = capacity == 1 && n_bad > 1;
  const uint64_t room = lowest_only ? 1 : n_bad;
  DevBuf list;
  R0H_TRY(list.alloc(ctx, room * sizeof(SessionSlot)));
  hipLaunchKernelGGL(balance_compact_kernel<SessionSlot>, dim3(scan_grid), dim3(256), 0, ctx->stream, (SessionSlot*)list->ptr, (unsigned long long)room, t->slots(), (unsigned long long)slots,
                     lowest_only ? counters[BAL_FIRST_INV] : 0ull, ctr);
  R0H_TRY(launch_ok("balance_compact_kernel"));
  std::vector<SessionSlot> found(room);
  R0H_TRY(r0h_buf_d2h(ctx, list.get(), 0, found.data(), room * sizeof(SessionSlot)));
  std::sort(found.begin(), found.end(), [](const SessionSlot& a, const SessionSlot& b) { return a.first_inv > b.first_inv; });
  for (size_t k = 0; k < found.size() && k < capacity; k++) {
    const uint64_t first = ~found[k].first_inv;
    out[k] = r0h_session_imbalance{(uint32_t)(first >> 32), (uint32_t)(first & 255u), (uint32_t)(first >> 8) & 0xffffffu, (uint32_t)(found[k].sum % P), found[k].members, (uint32_t)sb->ids.size(),
                                   {0, 0, 0, 0, 0, 0, 0, 0}};
    memcpy(out[k].values, found[k].values, sizeof found[k].values);
  }
  return nullptr;
}

extern "C" const char* r0h_session_balance_add(r0h_session_balance* sb, uint32_t source, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data,
                                               const uint32_t* global_host) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(sb && c && data, "r0h_session_balance_add: NULL argument");
  R0H_REQUIRE(sb->ctx, "r0h_session_balance_add: this handle was made without a context: its segments are added with r0h_session_balance_add_host");
  R0H_REQUIRE(po2 >= 4 && po2 <= R0H_MAX_PO2, "r0h_session_balance_add: po2 %u outside [4, %u]", po2, R0H_MAX_PO2);
  R0H_REQUIRE(c->blob == sb->circuit.blob, "r0h_session_balance_add: the circuit is not the one the handle was made with");
  r0h_ctx* ctx = sb->ctx;
  R0H_REQUIRE(data->ctx->device == ctx->device && (!code || code->ctx->device == ctx->device), "r0h_session_balance_add: the buffers are on another device than the handle's context");
  const uint32_t n = 1u << po2, n_chain = c->logup.n_chain, n_own = (uint32_t)c->logup.accs.size() - n_chain, n_ids = (uint32_t)sb->ids.size();
  if (!n_own) return nullptr;
  R0H_REQUIRE(((size_t)c->group_size[R0H_GROUP_DATA] << po2) * 4 <= data->bytes && (!code || ((size_t)c->group_size[R0H_GROUP_CODE] << po2) * 4 <= code->bytes),
              "r0h_session_balance_add: buffers too small for 2^%u rows", po2);
  R0H_REQUIRE(global_host || !sb->reads_global, "r0h_session_balance_add: a form reads a public input and none were given");
  for (uint32_t i = 0; i + c->n_late < c->n_global; i++) R0H_REQUIRE(!global_host || global_host[i] < P, "r0h_session_balance_add: global[%u] not canonical", i);
  std::vector<uint32_t> no_global(c->n_global + 4, 0), dummy_mix(c->n_mix, 0);  // the challenges' values are not read, their identities are
  Tape t;
  R0H_TRY(build_tape(c, po2, code, data, global_host ? global_host : no_global.data(), dummy_mix.data(), &t, 0xffffffffu, n_chain));
  DeviceTape d;
  R0H_TRY(upload_tape(ctx, t, &d));
  std::vector<uint32_t> ch_to_id(t.ch_id.size() + 4, 0xffu);  // the tape's challenge numbers -> the handle's identities ("one" is on every tape, used or not)
  for (size_t k = 0; k < t.ch_id.size(); k++) {
    const auto it = std::find(sb->ids.begin(), sb->ids.end(), t.ch_id[k]);
    if (it != sb->ids.end()) ch_to_id[k] = (uint32_t)(it - sb->ids.begin());
  }
  KScope ks(ctx, "session_balance", (double)t.cols.size() * n * 4);
  R0H_TRY(session_table_ensure(sb));
  SessionTable* tb = sb->table;
  DevBuf map;
  R0H_TRY(map.alloc(ctx, ch_to_id.size() * 4));
  R0H_TRY(stage_h2d(ctx, map->ptr, ch_to_id.data(), ch_to_id.size() * 4));
  // the tuples to come: the numerators alone (the chain's counting kernel on this tape)
  R0H_TRY_HIP(hipMemsetAsync(tb->ctr() + BAL_TUPLES, 0, 8, ctx->stream));
  const uint32_t count_grid = std::min<uint32_t>((uint32_t)std::max(ctx->n_cu, 1), (n + BAL_THREADS - 1) / BAL_THREADS);
  hipLaunchKernelGGL(balance_count_kernel, dim3(count_grid), dim3(BAL_THREADS), 0, ctx->stream, tb->ctr(), d.words, d.cols, n_own, po2);
  R0H_TRY(launch_ok("balance_count_kernel"));
  unsigned long long tuples = 0;
  R0H_TRY(r0h_buf_d2h(ctx, tb->side.get(), BAL_TUPLES * 8, &tuples, 8));
  R0H_REQUIRE(sb->tuples + tuples <= 0xffffffffull, "r0h_session_balance_add: more than 2^32 - 1 tuples in one handle");
  if (tuples) {
    R0H_TRY(session_table_grow(sb, sb->tuples + tuples));
    hipLaunchKernelGGL(session_insert_kernel, dim3((n + SES_THREADS - 1) / SES_THREADS), dim3(SES_THREADS), 0, ctx->stream, tb->slots(), tb->slot_bits, tb->ctr(), d.words, d.cols, tb->weights(),
                       (const uint32_t*)map->ptr, n_ids, n_own, 4 * n_chain, source, po2);
    R0H_TRY(launch_ok("session_insert_kernel"));
  }
  R0H_TRY(session_table_settle(sb));  // (synchronises: the tape goes back to the pool, the caller's buffers are its own again)
  sb->tuples += tuples;
  return nullptr;
  R0H_GUARD_END
}
