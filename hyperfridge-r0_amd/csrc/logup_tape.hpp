// The fraction tape of the log-derivative argument: what logup.hip's term kernel and balance.hip's kernels walk.  Built per launch on
// the host from the blob's fractions (public inputs folded into the coefficients; build_tape / upload_tape are logup.hip's), read
// uniformly across the wave on the device: a tape position is a function of the tape alone, never of the row, so the loads stay scalar.
// The device helpers are header-inline: the library has no relocatable device code.
#pragma once
#include <algorithm>

#include "circuit.hpp"

namespace r0h {
struct Tape {
  std::vector<uint32_t> words;              // per accumulator, per fraction: table, num form, n_parts, (challenge index, form)...; form = n, (coef, column + 1)...
  std::vector<const uint32_t*> cols;        // column base pointers
  std::vector<Fp4> ch;                      // challenges; index 0 is "one"
  std::vector<uint64_t> ch_id;              // their identities, kind << 32 | index (0: "one"): what the balance checks' weights are indexed by
  std::vector<uint32_t> acc_begin;          // word offset of every accumulator on the tape, and the tape's end
  std::vector<uint32_t> patch;              // Challenges::deferred: (tape word, public input) pairs -- the coefficient there is still to be multiplied by that input
};
// The tape of accumulators [first, first + count).  `ch` holds the challenges' values (from `mix` and the public inputs: a missing
// source is an error), or zeros beside their identities (the balance checks read `ch_id` alone: `mix` may be nullptr).  `deferred`:
// neither `global` nor `mix` is read -- the identities as above, and the public inputs a coefficient takes listed in `patch` instead of
// folded in: upload_tape_deferred makes the tape whole on the device, from device copies of both
enum class Challenges { values, identities, deferred };
const char* build_tape(const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, const uint32_t* global, const uint32_t* mix, Challenges want, uint32_t first,
                       uint32_t count, Tape* t);

struct DeviceTape {
  DevBuf buf;
  const uint32_t* words = nullptr;
  const uint32_t* const* cols = nullptr;
  const Fp4* ch = nullptr;
};
const char* upload_tape(r0h_ctx* ctx, const Tape& t, DeviceTape* d);
// a Challenges::deferred tape uploaded and resolved in stream order: the coefficients in `patch` multiplied by their public inputs and
// the challenge block filled, both from `globals` (the circuit's n_global words) and `mix` (its n_mix words; nullptr if no identity is the mix's)
const char* upload_tape_deferred(r0h_ctx* ctx, const r0h_circuit* c, const Tape& t, const r0h_buf* globals, const r0h_buf* mix, DeviceTape* d);

// ---- grids.  The device's compute units, asked once a context
inline const char* cu_count(r0h_ctx* ctx, uint32_t* n_cu) {
  if (!ctx->n_cu) R0H_TRY_HIP(hipDeviceGetAttribute(&ctx->n_cu, hipDeviceAttributeMultiprocessorCount, ctx->device));
  *n_cu = (uint32_t)std::max(ctx->n_cu, 1);
  return nullptr;
}
// persistent: a workgroup per CU, fewer where `groups` of them hold all the rows
inline const char* persistent_grid(r0h_ctx* ctx, uint32_t groups, uint32_t* grid) {
  R0H_TRY(cu_count(ctx, grid));
  *grid = std::min(*grid, groups);
  return nullptr;
}
// a strided pass over the slots of a table: eight workgroups per CU at the most
inline const char* scan_grid(r0h_ctx* ctx, uint64_t slots, uint32_t threads, uint32_t* grid) {
  R0H_TRY(cu_count(ctx, grid));
  *grid = (uint32_t)std::min<uint64_t>((slots + threads - 1) / threads, 8ull * *grid);
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

// ---- the walk over one fraction.  Its head: the table word stepped over, the numerator at row r; returns n_parts, `at` at the first ...
__device__ __forceinline__ uint32_t fraction_head(const uint32_t* __restrict__ tape, uint32_t& at, const uint32_t* const* __restrict__ cols, uint32_t r, uint32_t& num) {
  at++;  // table
  num = eval_form(tape, at, cols, r);
  return tape[at++];
}
// ... which are evaluated (challenge index, then eval_form, n_parts times) or stepped over: the position after them
__device__ __forceinline__ uint32_t after_parts(const uint32_t* __restrict__ tape, uint32_t at, uint32_t n_parts) {
  for (uint32_t q = 0; q < n_parts; q++) at += 2 + 2 * tape[at + 1];
  return at;
}

}  // namespace r0h
