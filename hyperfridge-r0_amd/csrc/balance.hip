// The balance checks of the log-derivative argument, two diagnostics that are off by default: which classes of tuples fail to cancel
// among the chain links of one segment (r0h_logup_check_balance) and, over the accumulators with a public total, across the segments
// of a session and the verifier's side (r0h_session_balance_*: the device's table; the handle is balance_host.cpp's).  Both walk
// logup.hip's tape (logup_tape.hpp) with the challenges' identities in place of their values, and keep their classes in one kind of table.
#include <type_traits>

#include "../../include/r0hip_circuit.h"
#include "logup_tape.hpp"

namespace r0h {

namespace {
// ---- the class table: open-addressed, in global memory, keyed by balance_key (circuit.hpp).  One 64-bit compare-and-swap claims a
// slot, then a sum, a count and a minimum, all atomics at device scope, so the table's CONTENT does not depend on scheduling (where a
// class sits does; the host orders what it reads back).  No workgroup waits for another, every probe sequence is bounded by its
// table's size, and what a scan reads is complete by the kernel boundary alone.
struct BalanceSlot {
  unsigned long long key;        // 0: empty
  unsigned long long sum;        // of the canonical numerators
  unsigned long long first_inv;  // ~(row << 32 | fraction) of the lowest member: a maximum, so that an all-zero table is an empty one
  uint32_t members, pad;
};
static_assert(sizeof(BalanceSlot) == 32, "a slot is half a 64-byte line");
// a session's slot is one 64-byte line and also holds the class's per-identity sums, written by whoever claims it
struct SessionSlot {
  unsigned long long key;        // 0: empty
  unsigned long long sum;        // of the canonical numerators
  unsigned long long first_inv;  // ~(source << 32 | row << 8 | fraction) of the lowest member
  uint32_t members, pad;
  uint32_t values[8];            // canonical per-identity sums (class-constant)
};
static_assert(sizeof(SessionSlot) == 64, "a slot is one 64-byte line");
constexpr unsigned long long BAL_SPREAD = 0x9E3779B97F4A7C15ull;
enum { BAL_TUPLES = 0, BAL_GLOBAL_INSERTS, BAL_IMBALANCED, BAL_FIRST_INV, BAL_ERR, BAL_CURSOR, BAL_COUNTERS };
enum { SES_OCCUPIED = BAL_COUNTERS, SES_COUNTERS };  // a session's table counts its claimed slots as well

// A tuple, or a workgroup's or an old table's share of a class, into its slot.  A SessionSlot takes the class's values `vals` [8] from
// whoever claims it, and the claim is counted at `occupied` (nullptr: a rehash, which moves classes and makes none).  A BalanceSlot
// has neither and says so: no default, lest a session's caller leave its values out.
template <class Slot>
__device__ __forceinline__ void table_insert(Slot* __restrict__ table, uint32_t slot_bits, unsigned long long* __restrict__ ctr, unsigned long long key, unsigned long long sum,
                                             uint32_t members, unsigned long long first_inv, const uint32_t* vals, unsigned long long* __restrict__ occupied) {
  const unsigned long long mask = (1ull << slot_bits) - 1;
  unsigned long long i = (key * BAL_SPREAD) >> (64 - slot_bits);
  for (unsigned long long probe = 0; probe <= mask; probe++) {  // bounded by the table's size (at a load of 1/2 or less: a handful)
    Slot* s = table + i;
    const unsigned long long prev = atomicCAS(&s->key, 0ull, key);
    if constexpr (std::is_same<Slot, SessionSlot>::value)
      if (prev == 0ull) {  // the claimer alone writes the class's values, two to a word; the scan reads them after the kernel boundary.  Atomic
                           // exchanges, not plain stores: the line's other words are updated by device-scope atomics from every XCD
        unsigned long long* v = (unsigned long long*)&s->values[0];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) atomicExch(&v[k], (unsigned long long)vals[2 * k + 1] << 32 | vals[2 * k]);
        if (occupied) atomicAdd(occupied, 1ull);
      }
    if (prev == 0ull || prev == key) {
      atomicAdd(&s->sum, sum);
      // the count saturates at 2^32 - 1 (a merged share may bring one that is there already): whoever wraps the word sets it to the
      // maximum afterwards, and any addition after that wraps again and does the same, so the last word is the maximum iff any wrapped
      if (atomicAdd(&s->members, members) > ~members) atomicMax(&s->members, 0xffffffffu);
      atomicMax(&s->first_inv, first_inv);
      return;
    }
    i = (i + 1) & mask;
  }
  atomicOr(&ctr[BAL_ERR], 1ull);  // every slot is another class's: the caller reports "table full"
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

// What a table holds that does not balance: *n_out classes, in `found` the `capacity` lowest in order of their first members (one
// wanted of many is the minimum the scan has found; otherwise all come back and are ordered here).  `side` begins with the table's
// counters: a report starts from nothing (a session reports more than once; the chain's counters are fresh, and clearing them is idle) and leaves them in `counters` as the scan left them.
template <class Slot>
const char* table_report(const char* caller, r0h_ctx* ctx, const r0h_buf* side, const Slot* table, uint64_t slots, size_t capacity, size_t* n_out, std::vector<Slot>* found,
                         unsigned long long (&counters)[BAL_COUNTERS]) {
  unsigned long long* const ctr = (unsigned long long*)side->ptr;
  static_assert(BAL_FIRST_INV == BAL_IMBALANCED + 1, "the two counters of a scan are cleared together");
  R0H_TRY_HIP(hipMemsetAsync(ctr + BAL_IMBALANCED, 0, 16, ctx->stream));
  R0H_TRY_HIP(hipMemsetAsync(ctr + BAL_CURSOR, 0, 8, ctx->stream));
  uint32_t grid;
  R0H_TRY(scan_grid(ctx, slots, 256, &grid));
  hipLaunchKernelGGL(balance_scan_kernel<Slot>, dim3(grid), dim3(256), 0, ctx->stream, table, (unsigned long long)slots, ctr);
  R0H_TRY(launch_ok("balance_scan_kernel"));
  R0H_TRY(r0h_buf_d2h(ctx, side, 0, counters, sizeof counters));
  R0H_REQUIRE(!counters[BAL_ERR], "%s: table full", caller);
  const uint64_t n_bad = counters[BAL_IMBALANCED];
  *n_out = (size_t)n_bad;
  if (!n_bad || !capacity) return nullptr;
  const bool lowest_only = capacity == 1 && n_bad > 1;
  const uint64_t room = lowest_only ? 1 : n_bad;
  DevBuf list;
  R0H_TRY(list.alloc(ctx, room * sizeof(Slot)));
  hipLaunchKernelGGL(balance_compact_kernel<Slot>, dim3(grid), dim3(256), 0, ctx->stream, (Slot*)list->ptr, (unsigned long long)room, table, (unsigned long long)slots,
                     lowest_only ? counters[BAL_FIRST_INV] : 0ull, ctr);
  R0H_TRY(launch_ok("balance_compact_kernel"));
  found->resize(room);
  R0H_TRY(r0h_buf_d2h(ctx, list.get(), 0, found->data(), room * sizeof(Slot)));
  std::sort(found->begin(), found->end(), [](const Slot& a, const Slot& b) { return a.first_inv > b.first_inv; });
  if (found->size() > capacity) found->resize(capacity);
  return nullptr;
}

// ---- the chain links (r0h_logup_check_balance, include/r0hip.h): every fraction with a non-zero numerator is a tuple, its class the
// denominator as a polynomial in the challenges.  Before the global table stands one of the same shape in LDS that takes every insert
// of its workgroup first: on a real trace most lookup slots ask for value 0, one class of tens of millions of members, which would
// otherwise all meet in one global slot (profiles/r05/logup_before.md, for the multiplicity count).
constexpr uint32_t BAL_THREADS = 1024;
constexpr uint32_t BAL_LDS_BITS = 12, BAL_LDS_SLOTS = 1u << BAL_LDS_BITS;  // 4,096 classes a workgroup: 112 KB of the CU's 160
constexpr uint32_t BAL_LDS_PROBES = 8;

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
      uint32_t num;
      const uint32_t n_parts = fraction_head(tape, at, cols, r, num);
      count += num != 0u;
      at = after_parts(tape, at, n_parts);
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
        uint32_t num;
        const uint32_t n_parts = fraction_head(tape, at, cols, r, num);
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
          table_insert(table, slot_bits, ctr, key, value, 1u, first_inv, nullptr, nullptr);
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
        table_insert(table, slot_bits, ctr, l_key[i], l_sum[i], l_members[i], l_first[i], nullptr, nullptr);
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

// ---- the session (r0h_session_balance_*, include/r0hip.h): the same definitions over the accumulators with a public total, whose
// tuples cancel across segments and against the verifier's side.  The table belongs to the handle and lives through its additions.
constexpr uint32_t SES_THREADS = 256, SES_FIRST_BITS = 10;

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
    uint32_t num;
    const uint32_t n_parts = fraction_head(tape, at, cols, r, num);
    const uint32_t next = after_parts(tape, at, n_parts);
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
      table_insert(table, slot_bits, ctr, balance_key(h0, h1), dec(num), 1u, ~session_first(source, r, first_fraction + f), vals, &ctr[SES_OCCUPIED]);
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
  table_insert(table, slot_bits, ctr, keys[i], numerators[i], 1u, ~session_first(source, i, SESSION_OUTSIDE_FRACTION), vals, &ctr[SES_OCCUPIED]);
}
// growth: every occupied slot of the old table into the new one -- sum (reduced: only its residue counts), members, first member, values
__global__ __launch_bounds__(SES_THREADS) void session_rehash_kernel(SessionSlot* __restrict__ to, uint32_t to_bits, unsigned long long* __restrict__ ctr,
                                                                     const SessionSlot* __restrict__ from, unsigned long long from_slots) {
  for (unsigned long long i = blockIdx.x * (unsigned long long)SES_THREADS + threadIdx.x; i < from_slots; i += gridDim.x * (unsigned long long)SES_THREADS) {
    const SessionSlot s = from[i];
    if (!s.key) continue;
    table_insert(to, to_bits, ctr, s.key, s.sum % P, s.members, s.first_inv, s.values, nullptr);
  }
}
// every occupied slot into a dense list (r0h_session_balance_export): balance_compact_kernel with "occupied" for "does not balance"
__global__ __launch_bounds__(SES_THREADS) void session_export_kernel(SessionSlot* __restrict__ list, unsigned long long room, const SessionSlot* __restrict__ table,
                                                                     unsigned long long slots, unsigned long long* __restrict__ ctr) {
  for (unsigned long long i = blockIdx.x * (unsigned long long)SES_THREADS + threadIdx.x; i < slots; i += gridDim.x * (unsigned long long)SES_THREADS) {
    const SessionSlot s = table[i];
    if (!s.key) continue;
    const unsigned long long at = atomicAdd(&ctr[BAL_CURSOR], 1ull);
    if (at < room) list[at] = s;
  }
}
// classes from another handle (r0h_session_balance_merge; the host has checked every entry): one lane per entry, its own sum, members
// and first member into its class, a class not held yet claimed with the entry's values.  No workgroup waits for another.
__global__ __launch_bounds__(SES_THREADS) void session_merge_kernel(SessionSlot* __restrict__ table, uint32_t slot_bits, unsigned long long* __restrict__ ctr,
                                                                    const r0h_session_class* __restrict__ classes, uint32_t n) {
  const uint32_t i = blockIdx.x * SES_THREADS + threadIdx.x;
  if (i >= n) return;
  const r0h_session_class e = classes[i];
  table_insert(table, slot_bits, ctr, e.key, e.net, e.members, ~session_first(e.source, e.first_row, e.fraction), e.values, &ctr[SES_OCCUPIED]);
}
}  // namespace
}  // namespace r0h

using namespace r0h;

extern "C" {

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
  R0H_TRY(build_tape(c, po2, code, data, global, nullptr, Challenges::identities, 0, n_chain, &t));
  DeviceTape d;
  R0H_TRY(upload_tape(ctx, t, &d));
  const uint32_t n_ch = (uint32_t)t.ch.size();
  const std::vector<uint32_t> weights = balance_weights(t.ch_id);
  DevBuf side;  // the counters, then the two weight rows
  R0H_TRY(side.alloc(ctx, BAL_COUNTERS * 8 + weights.size() * 4));
  unsigned long long* const ctr = (unsigned long long*)side->ptr;
  const uint32_t* const d_weights = (const uint32_t*)(ctr + BAL_COUNTERS);
  R0H_TRY_HIP(hipMemsetAsync(ctr, 0, BAL_COUNTERS * 8, ctx->stream));
  R0H_TRY(stage_h2d(ctx, (void*)d_weights, weights.data(), weights.size() * 4));
  uint32_t grid;
  R0H_TRY(persistent_grid(ctx, (n + BAL_THREADS - 1) / BAL_THREADS, &grid));
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
  std::vector<BalanceSlot> found;
  const char* err = table_report("r0h_logup_check_balance", ctx, side.get(), d_table, slots, capacity, n_out, &found, counters);
  ctx->balance_stats[1] = counters[BAL_GLOBAL_INSERTS];
  ctx->balance_stats[2] = slots;
  R0H_TRY(err);
  for (size_t k = 0; k < found.size(); k++) {
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

}  // extern "C"
const char* r0h::require_balance(const char* caller, r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, const uint32_t* global) {
  r0h_imbalance first = {0, 0, 0, 0};
  size_t n_bad = 0;
  R0H_TRY(r0h_logup_check_balance(ctx, c, po2, code, data, global, &first, 1, &n_bad));
  R0H_REQUIRE(!n_bad, "%s: fraction %u does not balance: net %u over %u tuples, first at row %u; %zu classes in all", caller, first.fraction, first.net, first.members, first.first_row, n_bad);
  return nullptr;
}

// ---- the session balance's table (the handle and everything that needs no device: balance_host.cpp)
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
  sb->table = t.release();
  return nullptr;
}
// slots >= 2 x the classes there can be (`tuples`: sb->room and what is about to come): the next power of two that holds them, every
// occupied slot re-inserted, the old table released
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
  uint32_t grid;
  R0H_TRY(scan_grid(ctx, from_slots, SES_THREADS, &grid));
  hipLaunchKernelGGL(session_rehash_kernel, dim3(grid), dim3(SES_THREADS), 0, ctx->stream, (SessionSlot*)bigger->ptr, bits, t->ctr(), t->slots(), from_slots);
  R0H_TRY(launch_ok("session_rehash_kernel"));
  R0H_TRY_HIP(ctx_wait(ctx));  // the old table goes back to the pool
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
  R0H_TRY(session_table_grow(sb, sb->room + tuples));
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
  R0H_TRY(session_table_settle(sb));  // (synchronises: the list goes back to the pool)
  sb->room += tuples;
  return nullptr;
}

const char* r0h::session_table_export(r0h_session_balance* sb, std::vector<r0h_session_class>* out) {
  r0h_ctx* ctx = sb->ctx;
  out->clear();
  if (!sb->table) return nullptr;  // nothing was added
  SessionTable* t = sb->table;
  const uint64_t slots = 1ull << t->slot_bits;
  KScope ks(ctx, "session_balance", (double)slots * sizeof(SessionSlot));
  unsigned long long occupied = 0;
  R0H_TRY(r0h_buf_d2h(ctx, t->side.get(), SES_OCCUPIED * 8, &occupied, 8));
  if (!occupied) return nullptr;
  R0H_REQUIRE(occupied <= slots, "r0h_session_balance_export: %llu classes counted in %llu slots", occupied, (unsigned long long)slots);
  DevBuf list;
  R0H_TRY(list.alloc(ctx, occupied * sizeof(SessionSlot)));
  R0H_TRY_HIP(hipMemsetAsync(t->ctr() + BAL_CURSOR, 0, 8, ctx->stream));
  uint32_t grid;
  R0H_TRY(scan_grid(ctx, slots, SES_THREADS, &grid));
  hipLaunchKernelGGL(session_export_kernel, dim3(grid), dim3(SES_THREADS), 0, ctx->stream, (SessionSlot*)list->ptr, occupied, t->slots(), (unsigned long long)slots, t->ctr());
  R0H_TRY(launch_ok("session_export_kernel"));
  std::vector<SessionSlot> found(occupied);
  R0H_TRY(r0h_buf_d2h(ctx, list.get(), 0, found.data(), occupied * sizeof(SessionSlot)));  // (synchronises: the list goes back to the pool)
  unsigned long long copied = 0;
  R0H_TRY(r0h_buf_d2h(ctx, t->side.get(), BAL_CURSOR * 8, &copied, 8));
  R0H_REQUIRE(copied == occupied, "r0h_session_balance_export: %llu classes counted, %llu found", occupied, copied);
  out->resize(occupied);
  for (size_t k = 0; k < found.size(); k++) {
    const SessionSlot& s = found[k];
    const uint64_t first = ~s.first_inv;
    r0h_session_class& e = (*out)[k];
    e = r0h_session_class{s.key, (uint32_t)(s.sum % P), s.members, (uint32_t)(first >> 32), (uint32_t)(first >> 8) & 0xffffffu, (uint32_t)(first & 255u), (uint32_t)sb->ids.size(), {0, 0, 0, 0, 0, 0, 0, 0}};
    memcpy(e.values, s.values, sizeof e.values);
  }
  return nullptr;
}

const char* r0h::session_table_merge(r0h_session_balance* sb, const r0h_session_class* classes, size_t n, uint64_t distinct) {
  r0h_ctx* ctx = sb->ctx;
  KScope ks(ctx, "session_balance", (double)n * sizeof(r0h_session_class));
  R0H_TRY(session_table_ensure(sb));
  if (!n) return nullptr;
  R0H_TRY(session_table_grow(sb, sb->room + distinct));  // counted first: the load stays at 1/2 or below if every key is a class not held yet
  DevBuf list;
  R0H_TRY(list.alloc(ctx, n * sizeof(r0h_session_class)));
  R0H_TRY(r0h_buf_h2d(ctx, list.get(), 0, classes, n * sizeof(r0h_session_class)));
  SessionTable* t = sb->table;
  hipLaunchKernelGGL(session_merge_kernel, dim3((uint32_t)((n + SES_THREADS - 1) / SES_THREADS)), dim3(SES_THREADS), 0, ctx->stream, t->slots(), t->slot_bits, t->ctr(),
                     (const r0h_session_class*)list->ptr, (uint32_t)n);
  R0H_TRY(launch_ok("session_merge_kernel"));
  R0H_TRY(session_table_settle(sb));  // (synchronises: the list goes back to the pool)
  sb->room += distinct;
  return nullptr;
}

const char* r0h::session_table_report(r0h_session_balance* sb, r0h_session_imbalance* out, size_t capacity, size_t* n_out) {
  r0h_ctx* ctx = sb->ctx;
  *n_out = 0;
  if (!sb->table) return nullptr;  // nothing was added
  SessionTable* t = sb->table;
  const uint64_t slots = 1ull << t->slot_bits;
  KScope ks(ctx, "session_balance", (double)slots * sizeof(SessionSlot));
  unsigned long long counters[BAL_COUNTERS];
  std::vector<SessionSlot> found;
  R0H_TRY(table_report("r0h_session_balance", ctx, t->side.get(), t->slots(), slots, capacity, n_out, &found, counters));
  for (size_t k = 0; k < found.size(); k++) out[k] = session_entry(~found[k].first_inv, found[k].sum, found[k].members, sb->ids.size(), found[k].values);
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
  Tape t;
  R0H_TRY(build_tape(c, po2, code, data, global_host, nullptr, Challenges::identities, n_chain, n_own, &t));
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
  uint32_t count_grid;
  R0H_TRY(persistent_grid(ctx, (n + BAL_THREADS - 1) / BAL_THREADS, &count_grid));
  hipLaunchKernelGGL(balance_count_kernel, dim3(count_grid), dim3(BAL_THREADS), 0, ctx->stream, tb->ctr(), d.words, d.cols, n_own, po2);
  R0H_TRY(launch_ok("balance_count_kernel"));
  unsigned long long tuples = 0;
  R0H_TRY(r0h_buf_d2h(ctx, tb->side.get(), BAL_TUPLES * 8, &tuples, 8));
  R0H_REQUIRE(sb->tuples + tuples <= 0xffffffffull, "r0h_session_balance_add: more than 2^32 - 1 tuples in one handle");
  if (tuples) {
    R0H_TRY(session_table_grow(sb, sb->room + tuples));
    hipLaunchKernelGGL(session_insert_kernel, dim3((n + SES_THREADS - 1) / SES_THREADS), dim3(SES_THREADS), 0, ctx->stream, tb->slots(), tb->slot_bits, tb->ctr(), d.words, d.cols, tb->weights(),
                       (const uint32_t*)map->ptr, n_ids, n_own, 4 * n_chain, source, po2);
    R0H_TRY(launch_ok("session_insert_kernel"));
  }
  R0H_TRY(session_table_settle(sb));  // (synchronises: the tape goes back to the pool, the caller's buffers are its own again)
  sb->tuples += tuples;
  sb->room += tuples;
  return nullptr;
  R0H_GUARD_END
}
