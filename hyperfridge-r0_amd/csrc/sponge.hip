// The rows of the in-circuit Poseidon2 sponge (include/r0hip_circuit.h SPONGE, tools/sponge_component.py) made on the device: what
// r0h_lift, r0h_join and the image proof plant into a witness.  The chain from one permutation to the next is sequential and stays on
// the host (poseidon2_host.cpp p2_sponge_chain_host: one pass gives the digest and what every permutation starts from); a permutation's 30 rows
// depend only on those 24 words, so the expansion -- 65 columns x 30 rows per permutation, 32 MB for a 2^20-row segment seal -- is
// one launch over the trace's rows instead of a host loop, a pageable staging vector and a 2-D copy.
#include "circuit.hpp"
#include "poseidon2_device.hpp"

namespace r0h {

// What the kernel reads beside the states: the round constants and the diagonal of the table the circuit's sponge constraints are
// written for -- the compiled-in one (p2_default), as p2_sponge_rows_host uses it, whatever table the context hashes Merkle trees with.
struct SpongeTable {
  uint32_t rc_full[2 * P2_HALF_FULL][P2_CELLS];
  uint32_t rc_partial[P2_PARTIAL];
  uint32_t diag[P2_CELLS];  // Montgomery form of (mu_i - 1)
  uint32_t pad[3];          // the states behind it start on a 16-byte boundary
};
static_assert(sizeof(SpongeTable) % 16 == 0, "SpongeTable is followed by the states");

// One lane per trace row.  Row 30 q + r holds permutation q's state after the external layer and r rounds, the cubes of round r - 1
// (all lanes of a full round, lane 0 of a partial one), the absorbed words on r = 0 and act = 1: the layout of p2_sponge_rows_host,
// word for word (every word is canonical, so the lazily reduced forms of poseidon2_device.hpp are not needed and not used).  Rows at
// or behind `used` = 30 n_perm are written as zero.
// The round loop is the same 29 rounds in every lane with the state update under a predicate (round j applies where j < r), not a
// per-lane trip count: a wave's 64 consecutive rows always hold an r = 29, so the wave runs 29 iterations either way, and with a
// uniform counter the kind of round and its constants are wave-uniform -- a scalar branch and scalar loads.
// Consecutive lanes are consecutive rows of each column: every store of a wave is one contiguous 256-byte run.
__global__ __launch_bounds__(256) void sponge_rows_kernel(uint32_t* __restrict__ cols, const SpongeTable* __restrict__ k, const uint32_t* __restrict__ states,
                                                           uint32_t n, uint32_t used) {
  const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;  // the grid is exactly n lanes
  uint32_t* __restrict__ out = cols + row;
  if (row >= used) {
#pragma unroll 1
    for (uint32_t col = 0; col < R0H_SPONGE_DATA_COLUMNS; col++) out[(size_t)col * n] = 0u;
    return;
  }
  const uint32_t q = row / R0H_SPONGE_PERIOD, r = row - q * R0H_SPONGE_PERIOD;
  uint32_t c[P2_CELLS], aux[P2_CELLS];
  const uint4* src = (const uint4*)(states + (size_t)q * P2_CELLS);
#pragma unroll
  for (int i = 0; i < P2_CELLS / 4; i++) {
    const uint4 v = src[i];
    c[4 * i] = v.x; c[4 * i + 1] = v.y; c[4 * i + 2] = v.z; c[4 * i + 3] = v.w;
  }
#pragma unroll
  for (int i = 0; i < P2_RATE; i++) out[(size_t)(2 * P2_CELLS + i) * n] = r == 0 ? c[i] : 0u;  // in[16]: the words absorbed on the first row
#pragma unroll
  for (int i = 0; i < P2_CELLS; i++) aux[i] = 0u;
  m_ext(c);
#pragma unroll 1
  for (uint32_t j = 0; j < (uint32_t)P2_ROUNDS; j++) {
    const bool live = j < r, last = j + 1 == r;
    uint32_t t[P2_CELLS];
    if (j < (uint32_t)P2_HALF_FULL || j >= (uint32_t)(P2_HALF_FULL + P2_PARTIAL)) {
      const uint32_t* __restrict__ rc = k->rc_full[j < (uint32_t)P2_HALF_FULL ? j : j - P2_PARTIAL];
#pragma unroll
      for (int i = 0; i < P2_CELLS; i++) {
        const uint32_t x = add(c[i], rc[i]), cube = mul(mul(x, x), x);
        t[i] = mul(mul(cube, cube), x);
        aux[i] = last ? cube : aux[i];
      }
      m_ext(t);
    } else {
      const uint32_t x = add(c[0], k->rc_partial[j - P2_HALF_FULL]), cube = mul(mul(x, x), x), y = mul(mul(cube, cube), x);
      aux[0] = last ? cube : aux[0];
      const uint32_t sum = add(y, sum_lanes_1_to_23(c));
      t[0] = add(sum, mul(k->diag[0], y));
#pragma unroll
      for (int i = 1; i < P2_CELLS; i++) t[i] = add(sum, mul(k->diag[i], c[i]));
    }
#pragma unroll
    for (int i = 0; i < P2_CELLS; i++) c[i] = live ? t[i] : c[i];
  }
#pragma unroll
  for (int i = 0; i < P2_CELLS; i++) {
    out[(size_t)i * n] = c[i];
    out[(size_t)(P2_CELLS + i) * n] = aux[i];
  }
  out[(size_t)(R0H_SPONGE_DATA_COLUMNS - 1) * n] = ONE;  // act
}

static const SpongeTable& sponge_table() {
  static const SpongeTable t = [] {
    SpongeTable s;
    const P2Consts& k = p2_default();
    memcpy(s.rc_full, k.rc_full, sizeof s.rc_full);
    memcpy(s.rc_partial, k.rc_partial, sizeof s.rc_partial);
    memcpy(s.diag, k.diag, sizeof s.diag);
    memset(s.pad, 0, sizeof s.pad);
    return s;
  }();
  return t;
}

// the 65 columns of 2^po2 rows at `cols` (device) from the chain's states (host): table and states go up through the pinned ring, in
// stream order; nothing is synchronised unless the states outgrow the ring (stage_h2d)
const char* sponge_rows_device(r0h_ctx* ctx, uint32_t* cols, uint32_t po2, const uint32_t* states, size_t n_perm) {
  const size_t n = (size_t)1 << po2;
  R0H_REQUIRE(po2 <= R0H_MAX_PO2 && n_perm >= 1 && n_perm * R0H_SPONGE_PERIOD < n, "sponge_rows_device: %zu permutations take %zu rows, the trace has 2^%u", n_perm, n_perm * R0H_SPONGE_PERIOD, po2);
  R0H_TRY_HIP(hipSetDevice(ctx->device));
  DevBuf up;
  R0H_TRY(up.alloc(ctx, sizeof(SpongeTable) + n_perm * P2_CELLS * 4));
  char* base = (char*)up->ptr;
  R0H_TRY(stage_h2d(ctx, base, &sponge_table(), sizeof(SpongeTable)));
  R0H_TRY(stage_h2d(ctx, base + sizeof(SpongeTable), states, n_perm * P2_CELLS * 4));
  const uint32_t threads = n < 256 ? (uint32_t)n : 256u;
  KScope ks(ctx, "sponge_rows_kernel", (double)R0H_SPONGE_DATA_COLUMNS * n * 4 + (double)n_perm * P2_CELLS * 4);
  hipLaunchKernelGGL(sponge_rows_kernel, dim3((uint32_t)(n / threads)), dim3(threads), 0, ctx->stream, cols, (const SpongeTable*)base, (const uint32_t*)(base + sizeof(SpongeTable)),
                     (uint32_t)n, (uint32_t)(n_perm * R0H_SPONGE_PERIOD));
  return launch_ok("sponge_rows_kernel");
}

const char* sponge_plant_states(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const uint32_t* states, size_t n_perm, r0h_buf* data) {
  R0H_REQUIRE(ctx && c && data && c->has_sponge && states, "sponge_plant: NULL argument, or a circuit without the sponge component");
  const size_t n = (size_t)1 << po2, rows = n_perm * R0H_SPONGE_PERIOD;
  R0H_REQUIRE(rows < n, "the in-circuit sponge over %zu permutations takes %zu rows: the recursion trace has 2^%u", n_perm, rows, po2);
  R0H_REQUIRE(((size_t)c->group_size[R0H_GROUP_DATA] << po2) * 4 <= data->bytes && c->sponge_data + R0H_SPONGE_DATA_COLUMNS <= c->group_size[R0H_GROUP_DATA],
              "sponge_plant: DATA buffer too small for 2^%u rows", po2);
  return sponge_rows_device(ctx, u32(data) + ((size_t)c->sponge_data << po2), po2, states, n_perm);
}

const char* sponge_plant(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const uint32_t* words, size_t n_words, r0h_buf* data) {
  R0H_REQUIRE(ctx && c && data && c->has_sponge && (words || !n_words), "sponge_plant: NULL argument, or a circuit without the sponge component");
  const size_t n = (size_t)1 << po2, n_perm = n_words ? (n_words + P2_RATE - 1) / P2_RATE : 1, rows = n_perm * R0H_SPONGE_PERIOD;
  R0H_REQUIRE(rows < n, "the in-circuit sponge over %zu words takes %zu rows: the recursion trace has 2^%u", n_words, rows, po2);
  for (size_t i = 0; i < n_words; i++) R0H_REQUIRE(words[i] < P, "sponge_plant: word %zu is not a canonical field element", i);
  std::vector<uint32_t> states;
  uint32_t digest[8];
  p2_sponge_chain_host(p2_default(), words, n_words, digest, &states);
  return sponge_plant_states(ctx, c, po2, states.data(), n_perm, data);
}

}  // namespace r0h

using namespace r0h;

extern "C" const char* r0h_sponge_trace_device(r0h_ctx* ctx, const uint32_t* words, size_t n_words, uint32_t po2, r0h_buf* cols_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && (words || n_words == 0) && cols_out, "r0h_sponge_trace_device: NULL argument");
  size_t n_perm = 0;
  R0H_TRY(sponge_trace_args("r0h_sponge_trace_device", words, n_words, po2, &n_perm));
  R0H_REQUIRE(((size_t)R0H_SPONGE_DATA_COLUMNS << po2) * 4 <= cols_out->bytes, "r0h_sponge_trace_device: %u columns of 2^%u rows exceed the output buffer", R0H_SPONGE_DATA_COLUMNS, po2);
  std::vector<uint32_t> states;
  uint32_t digest[8];
  p2_sponge_chain_host(p2_default(), words, n_words, digest, &states);
  return sponge_rows_device(ctx, u32(cols_out), po2, states.data(), n_perm);
  R0H_GUARD_END
}
