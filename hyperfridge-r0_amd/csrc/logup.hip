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
// The term interpreter reads a flat tape of the fractions (logup_tape.hpp; uniform across the wave: scalar loads) built per launch on
// the host, public inputs folded into the coefficients.  The accumulators with a public total are evaluated and scanned for their
// totals (r0h_logup_totals); a session keeps those scanned terms for the accumulation of the same segment (LogupKept, circuit.hpp).
// The same tape, with the challenges' identities in place of their values, is what the balance checks walk (balance.hip).
#include <map>

#include "../../include/r0hip_circuit.h"
#include "logup_tape.hpp"

namespace r0h {

const char* build_tape(const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, const uint32_t* global, const uint32_t* mix, Challenges want, uint32_t first,
                       uint32_t count, Tape* t) {
  std::map<uint32_t, uint32_t> col_index;
  std::map<uint64_t, uint32_t> ch_index;
  t->ch.push_back(fp4_one());
  t->ch_id.push_back(0);
  auto form = [&](const Lf& lf) -> const char* {
    t->words.push_back((uint32_t)lf.terms.size());
    for (const LfTerm& term : lf.terms) {
      uint32_t coef = enc(term.coef);
      if (term.global && want == Challenges::deferred) {
        t->patch.push_back((uint32_t)t->words.size());  // (where the coefficient is pushed below)
        t->patch.push_back(term.global - 1);
      } else if (term.global) {
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
  for (uint32_t j = first; j < first + count; j++) {
    const LogupAcc& a = c->logup.accs[j];
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
            const uint32_t* src = q.ch_kind == 1 ? mix : global;
            const size_t at = q.ch_kind == 1 ? 4 * (size_t)q.ch_idx : q.ch_idx;
            R0H_REQUIRE(src || want != Challenges::values, "log-derivative accumulation: a challenge is read from %s and none were given", q.ch_kind == 1 ? "the mix" : "the public inputs");
            it = ch_index.emplace(key, (uint32_t)t->ch.size()).first;
            t->ch.push_back(want == Challenges::values ? Fp4{{src[at], src[at + 1], src[at + 2], src[at + 3]}} : fp4_zero());
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

// A deferred tape made whole where the public inputs and the mix are: lanes [0, n_patch) multiply a coefficient by its public input,
// the n_ch lanes behind them copy a challenge's four words from the public inputs (kind 2) or the mix (kind 1) into the tape's
// challenge block.  table = n_patch (tape word, public input) pairs, then n_ch (kind, index) pairs.  A few dozen lanes, once a tape:
// the term kernel then reads the block exactly as it reads an uploaded one -- through scalar loads of a wave-uniform address (the compiler
// emits s_load_dwordx4 for ch[ci] and s_load_dword for the tape words in both forms, for the term kernel is the same code object: 0
// bytes of scratch and the same VGPR count by construction; profiles/r23/session_enqueue.md has the figures).
__global__ __launch_bounds__(64) void logup_resolve_kernel(uint32_t* __restrict__ words, uint32_t* __restrict__ ch, const uint32_t* __restrict__ table, uint32_t n_patch, uint32_t n_ch,
                                                            const uint32_t* __restrict__ globals, const uint32_t* __restrict__ mix) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i < n_patch) {
    const uint32_t w = table[2 * i];
    words[w] = mul(words[w], globals[table[2 * i + 1]]);
  } else if (i - n_patch < n_ch) {
    const uint32_t k = i - n_patch, kind = table[2 * (n_patch + k)], idx = table[2 * (n_patch + k) + 1];
    const uint32_t* src = kind == 1 ? mix + 4 * (size_t)idx : globals + idx;
#pragma unroll
    for (int q = 0; q < 4; q++) ch[4 * (size_t)(k + 1) + q] = src[q];
  }
}

const char* upload_tape_deferred(r0h_ctx* ctx, const r0h_circuit* c, const Tape& t, const r0h_buf* globals, const r0h_buf* mix, DeviceTape* d) {
  R0H_REQUIRE(globals && globals->bytes >= (size_t)c->n_global * 4, "log-derivative accumulation: the device copy of the public inputs holds fewer than %u words", c->n_global);
  R0H_REQUIRE(!mix || mix->bytes >= (size_t)c->n_mix * 4, "log-derivative accumulation: the device mix holds fewer than %u words", c->n_mix);
  const uint32_t n_patch = (uint32_t)(t.patch.size() / 2), n_ch = (uint32_t)t.ch.size() - 1;
  std::vector<uint32_t> table(t.patch);
  for (uint32_t k = 0; k < n_patch; k++) R0H_REQUIRE(table[2 * k] < t.words.size() && table[2 * k + 1] < c->n_global, "log-derivative accumulation: a coefficient reads public input %u of %u", table[2 * k + 1], c->n_global);
  for (uint32_t k = 1; k <= n_ch; k++) {  // (ch[0] is "one", uploaded with the tape)
    const uint32_t kind = (uint32_t)(t.ch_id[k] >> 32), idx = (uint32_t)t.ch_id[k];
    R0H_REQUIRE(kind == 1 ? (mix && 4 * (size_t)idx + 4 <= c->n_mix) : (kind == 2 && (size_t)idx + 4 <= c->n_global),
                "log-derivative accumulation: challenge %u of kind %u lies outside %s", idx, kind, kind == 1 ? "the device mix (or none was given)" : "the public inputs");
    table.insert(table.end(), {kind, idx});
  }
  R0H_TRY(upload_tape(ctx, t, d));
  if (table.empty()) return nullptr;
  DevBuf d_table;  // back to the pool behind the launch that reads it
  R0H_TRY(d_table.alloc(ctx, table.size() * 4));
  R0H_TRY(stage_h2d(ctx, d_table->ptr, table.data(), table.size() * 4));
  KScope ks(ctx, "logup_resolve_kernel", 8.0 * (double)table.size());
  hipLaunchKernelGGL(logup_resolve_kernel, dim3((n_patch + n_ch + 63) / 64), dim3(64), 0, ctx->stream, const_cast<uint32_t*>(d->words), (uint32_t*)const_cast<Fp4*>(d->ch), u32(d_table.get()),
                     n_patch, n_ch, u32(globals), mix ? u32(mix) : nullptr);
  return launch_ok("logup_resolve_kernel");
}

namespace {
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
    const uint32_t n_parts = fraction_head(tape, at, cols, r, num[f]);
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
}  // namespace

// tests/test_gpu_logup_kept.py hands the two internal entry points an empty LogupKept of its own making: one pointer, then po2, then n_own
static_assert(sizeof(DevBuf) == sizeof(void*) && sizeof(LogupKept) == sizeof(void*) + 8 && alignof(LogupKept) == alignof(void*),
              "LogupKept is no longer {buffer pointer, po2, n_own}: tests/test_gpu_logup_kept.py builds one by hand");
// standalone accumulators (`own_words`: where theirs begin on the device tape): terms -> running sums; totals_out (host, 4 words each)
// if wanted, ACCUM columns if `accum`; `keep`: the scanned terms outlive the call (the accumulation of the same segment unpacks them: logup_accum_kept);
// `d_globals`: every total copied, device to device, into the four words of a device copy of the public inputs where the circuit reads it
static const char* own_accumulators(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const uint32_t* own_words, const DeviceTape& d, r0h_buf* accum, uint32_t* totals_out, LogupKept* keep = nullptr,
                                    r0h_buf* d_globals = nullptr) {
  const uint32_t n = 1u << po2, n_chain = c->logup.n_chain, n_acc = (uint32_t)c->logup.accs.size(), n_own = n_acc - n_chain;
  if (!n_own) return nullptr;
  DevBuf terms;
  R0H_TRY(terms.alloc(ctx, (size_t)n_own * n * 16));
  hipLaunchKernelGGL(logup_term_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, accum ? u32(accum) : nullptr, (uint32_t*)nullptr, u32(terms.get()),
                     own_words, d.cols, d.ch, n_chain, n_acc, n_chain, po2);
  R0H_TRY(launch_ok("logup_term_kernel"));
  for (uint32_t k = 0; k < n_own; k++) {
    r0h_buf view = buf_view(terms.get(), (size_t)k * n * 16, (size_t)n * 16);
    R0H_TRY(r0h_prefix_sums(ctx, &view, n));
    if (accum) R0H_TRY(unpack_ext_columns(ctx, u32(accum) + ((size_t)(4 * (n_chain + k)) << po2), (const uint32_t*)view.ptr, po2));
    if (totals_out) R0H_TRY(r0h_buf_d2h(ctx, &view, (size_t)(n - 1) * 16, totals_out + 4 * k, 16));
    if (d_globals) {  // the scan's last element is the total
      const uint32_t at = c->logup.accs[n_chain + k].final_global;
      R0H_REQUIRE((size_t)at + 4 <= d_globals->bytes / 4, "r0h_logup_totals: a total goes to public inputs %u..%u, the device copy holds %zu words", at, at + 3, d_globals->bytes / 4);
      R0H_TRY_HIP(hipMemcpyAsync(u32(d_globals) + at, (const uint32_t*)view.ptr + 4 * (size_t)(n - 1), 16, hipMemcpyDeviceToDevice, ctx->stream));
    }
  }
  if (keep) {
    keep->terms = std::move(terms);
    keep->po2 = po2;
    keep->n_own = n_own;
  }
  return nullptr;
}

// what both forms of the accumulation ask of their buffers
static const char* accum_args(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, const r0h_buf* accum) {
  R0H_REQUIRE(ctx && c && data && accum, "r0h_accum: NULL argument");
  R0H_REQUIRE(po2 >= 4 && po2 <= R0H_MAX_PO2, "r0h_accum: po2 %u outside [4, %u]", po2, R0H_MAX_PO2);
  R0H_REQUIRE(((size_t)c->group_size[R0H_GROUP_DATA] << po2) * 4 <= data->bytes && ((size_t)c->group_size[R0H_GROUP_ACCUM] << po2) * 4 <= accum->bytes &&
                  (!code || ((size_t)c->group_size[R0H_GROUP_CODE] << po2) * 4 <= code->bytes),
              "r0h_accum: buffers too small for 2^%u rows", po2);
  return nullptr;
}
// the launches of the accumulation over a tape that stands on the device: terms, scan, chain, the public accumulators.  Waits for nothing.
static const char* accum_launch(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const Tape& t, const DeviceTape& d, r0h_buf* accum, const LogupKept* kept) {
  const uint32_t n = 1u << po2, n_chain = c->logup.n_chain;
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
    R0H_TRY(own_accumulators(ctx, c, po2, d.words + t.acc_begin[n_chain], d, accum, nullptr));
  }
  return nullptr;
}

const char* logup_accum_kept(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, const uint32_t* global, const uint32_t* mix, r0h_buf* accum,
                             const LogupKept* kept) {
  R0H_GUARD_BEGIN
  R0H_TRY(accum_args(ctx, c, po2, code, data, accum));
  for (uint32_t i = 0; i < c->n_mix; i++) R0H_REQUIRE(mix && mix[i] < P, "r0h_accum: mix[%u] missing or not canonical", i);
  for (uint32_t i = 0; i < c->n_global; i++) R0H_REQUIRE(!global || global[i] < P, "r0h_accum: global[%u] not canonical", i);
  Tape t;
  R0H_TRY(build_tape(c, po2, code, data, global, mix, Challenges::values, 0, (uint32_t)c->logup.accs.size(), &t));
  DeviceTape d;
  R0H_TRY(upload_tape(ctx, t, &d));
  R0H_TRY(accum_launch(ctx, c, po2, t, d, accum, kept));
  R0H_TRY_HIP(ctx_wait(ctx));  // the tape goes back to the pool
  return nullptr;
  R0H_GUARD_END
}

// The same accumulation with the public inputs and the mix where the device's transcript left them: nothing of either is read on the
// host, and nothing waits.  The tape, its table and every temporary are DevBufs of the context's pool, which hands a block out again in
// stream order only; the host words of the uploads were copied into the pinned ring when they were staged (stage_h2d waits by itself in
// the rare case that the ring wraps around).  That is all the wait of the host form stands for: it protects nothing the owners do not.
const char* logup_accum_kept_device(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, const r0h_buf* globals, const r0h_buf* mix, r0h_buf* accum,
                                    const LogupKept* kept) {
  R0H_GUARD_BEGIN
  R0H_TRY(accum_args(ctx, c, po2, code, data, accum));
  R0H_REQUIRE(globals && (mix || !c->n_mix), "r0h_accum: NULL argument");
  R0H_REQUIRE(!c->logup.accs.empty(), "r0h_accum_public_device: the circuit has no log-derivative argument: its accumulation (r0h_accum) takes the mix from the host");
  Tape t;
  R0H_TRY(build_tape(c, po2, code, data, nullptr, nullptr, Challenges::deferred, 0, (uint32_t)c->logup.accs.size(), &t));
  DeviceTape d;
  R0H_TRY(upload_tape_deferred(ctx, c, t, globals, mix, &d));
  return accum_launch(ctx, c, po2, t, d, accum, kept);
  R0H_GUARD_END
}

}  // namespace r0h

using namespace r0h;

extern "C" {

// The launches of r0h_logup_multiplicities; `hist` keeps the counters, and behind them the error word (*err_word_out: a device pointer
// into it) the caller looks at once the stream has run: bit 0 a numerator that is neither 0 nor 1, bit 1 a value that is not in its table.
static const char* multiplicities_launch(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, r0h_buf* data, const uint32_t* global, DevBuf& hist, uint32_t** err_word_out) {
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
  // hist: [n_tables][65536] counts, then per table the lookups binned and the slots gated off, then the error word
  const size_t hist_words = (size_t)n_tables * 65536;
  R0H_TRY(hist.alloc(ctx, hist_words * 4 + 32));
  R0H_TRY_HIP(hipMemsetAsync(hist->ptr, 0, hist_words * 4 + 32, ctx->stream));
  uint32_t* const counters = u32(hist.get()) + hist_words;
  uint32_t* const err_word = counters + 4;
  uint32_t grid;
  R0H_TRY(persistent_grid(ctx, n / COUNT_THREADS, &grid));
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
  *err_word_out = err_word;
  return nullptr;
}
}  // extern "C"
namespace r0h {
const char* logup_multiplicities_verdict(uint32_t err) {
  R0H_REQUIRE(!(err & 1u), "r0h_logup_multiplicities: a lookup's numerator is neither 0 nor 1");
  R0H_REQUIRE(!(err & 2u), "r0h_logup_multiplicities: a row whose numerator is 1 looks up a value that is not in its table");
  return nullptr;
}
// r0h_logup_multiplicities without its wait: the error word goes device to device to err_out[err_word_offset], for the caller to read
// back with whatever else it gathers and hand to logup_multiplicities_verdict (session.cpp: phase 1 from the calling thread)
const char* logup_multiplicities_enqueue(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, r0h_buf* data, const uint32_t* global, r0h_buf* err_out, size_t err_word_offset) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && c && data && err_out, "r0h_logup_multiplicities: NULL argument");
  R0H_TRY(require_words_in("r0h_logup_multiplicities", "error word", err_out, err_word_offset, 1));
  if (c->logup.tables.empty()) {
    R0H_TRY_HIP(hipMemsetAsync(u32(err_out) + err_word_offset, 0, 4, ctx->stream));
    return nullptr;
  }
  DevBuf hist;  // back to the pool behind the copy that reads it
  uint32_t* err_word = nullptr;
  R0H_TRY(multiplicities_launch(ctx, c, po2, data, global, hist, &err_word));
  R0H_TRY_HIP(hipMemcpyAsync(u32(err_out) + err_word_offset, err_word, 4, hipMemcpyDeviceToDevice, ctx->stream));
  return nullptr;
  R0H_GUARD_END
}
}  // namespace r0h
extern "C" {
// Fill the multiplicity columns of `data` from the lookups its rows make (before DATA is committed).
const char* r0h_logup_multiplicities(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, r0h_buf* data, const uint32_t* global) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && c && data, "r0h_logup_multiplicities: NULL argument");
  if (c->logup.tables.empty()) return nullptr;
  DevBuf hist;
  uint32_t* err_word = nullptr;
  R0H_TRY(multiplicities_launch(ctx, c, po2, data, global, hist, &err_word));
  R0H_TRY_HIP(ctx_wait(ctx));
  uint32_t err = 0;
  R0H_TRY(r0h_buf_d2h(ctx, hist.get(), (size_t)((char*)err_word - (char*)hist->ptr), &err, 4));
  return logup_multiplicities_verdict(err);
  R0H_GUARD_END
}

// The totals of the accumulators that run alone (their challenges are public inputs, so they can be had before the mix is drawn):
// global_io[final .. final + 4) of each is overwritten with its total over the rows.
const char* r0h_logup_totals(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, uint32_t* global_io) {
  return logup_totals_keep(ctx, c, po2, code, data, global_io, nullptr);
}

const char* r0h_logup_totals_device(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, r0h_buf* globals_io) {
  return logup_totals_keep_device(ctx, c, po2, code, data, globals_io, nullptr);
}
const char* r0h_accum_public_device(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, const r0h_buf* globals, const r0h_buf* mix, r0h_buf* accum) {
  R0H_REQUIRE(ctx && c, "r0h_accum_public_device: NULL argument");
  return logup_accum_kept_device(ctx, c, po2, code, data, globals, mix, accum, nullptr);
}

}  // extern "C"

// r0h_logup_totals with the public inputs on the device: the challenges are read there and every total is left there, in the words of
// `globals` the circuit reads it from.  Nothing crosses to the host and nothing waits.
const char* r0h::logup_totals_keep_device(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, r0h_buf* globals, LogupKept* keep) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && c && data && globals, "r0h_logup_totals: NULL argument");
  R0H_REQUIRE(po2 >= 4 && po2 <= R0H_MAX_PO2, "r0h_logup_totals: po2 %u outside [4, %u]", po2, R0H_MAX_PO2);
  R0H_REQUIRE(((size_t)c->group_size[R0H_GROUP_DATA] << po2) * 4 <= data->bytes && (!code || ((size_t)c->group_size[R0H_GROUP_CODE] << po2) * 4 <= code->bytes),
              "r0h_logup_totals: buffers too small for 2^%u rows", po2);
  const uint32_t n_chain = c->logup.n_chain, n_acc = (uint32_t)c->logup.accs.size();
  if (n_acc == n_chain) return nullptr;
  for (uint32_t j = n_chain; j < n_acc; j++)
    for (const LogupFraction& f : c->logup.accs[j].fr)
      for (const LogupPart& q : f.parts) R0H_REQUIRE(q.ch_kind != 1, "r0h_logup_totals: accumulator %u takes a challenge from the mix", j);
  Tape t;
  R0H_TRY(build_tape(c, po2, code ? code : data, data, nullptr, nullptr, Challenges::deferred, n_chain, n_acc - n_chain, &t));
  DeviceTape d;
  R0H_TRY(upload_tape_deferred(ctx, c, t, globals, nullptr, &d));
  return own_accumulators(ctx, c, po2, d.words, d, nullptr, nullptr, keep, globals);
  R0H_GUARD_END
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
  R0H_TRY(build_tape(c, po2, code ? code : data, data, global_io, nullptr, Challenges::values, n_chain, n_acc - n_chain, &t));  // (no challenge of theirs is the mix's)
  DeviceTape d;
  R0H_TRY(upload_tape(ctx, t, &d));
  std::vector<uint32_t> totals(4 * (size_t)(n_acc - n_chain));
  R0H_TRY(own_accumulators(ctx, c, po2, d.words, d, nullptr, totals.data(), keep));
  for (uint32_t j = n_chain; j < n_acc; j++) memcpy(global_io + c->logup.accs[j].final_global, totals.data() + 4 * (size_t)(j - n_chain), 16);
  return nullptr;
  R0H_GUARD_END
}
