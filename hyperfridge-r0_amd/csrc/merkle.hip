// Row hashing and Merkle folding for gfx950 under the context's hash suite (hash_suite_device.hpp): Poseidon2 (BabyBear, t=24, rate 16,
// x^7, 4+21+4 rounds) or SHA-256.  Replaces risc0-zkp 3.0.4 hal `hash_rows` / `hash_fold` (CUDA side: risc0-sys 1.5.0 poseidon2 and
// sha256 kernels) -- SURVEY.md 8(a) a6-a8.
//
// One lane owns one row (hash_rows) or one parent node (hash_fold): the hash's state lives in VGPRs, the round constants are
// wave-uniform (Poseidon2: scalar loads; SHA-256: literals), and consecutive lanes read consecutive rows of each column so every
// column access of a wave is one contiguous 256-byte run.  Under Poseidon2 these kernels are VALU-integer bound (about 1.36k
// Montgomery products per permutation), not HBM bound: see DESIGN.md for the arithmetic.
#include "hash_suite_device.hpp"
#include "merkle_fused_plan.hpp"

namespace r0h {

template <class S>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(S::rows_waves))) void hash_rows_kernel(uint32_t* __restrict__ digests, const uint32_t* __restrict__ matrix,
                                                         uint32_t rows, uint32_t cols, typename S::Consts k) {
  uint32_t row = blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  uint32_t d[8];
  S::row(d, matrix + row, rows, cols, k);
  uint4* dst = (uint4*)(digests + (size_t)row * 8);
  dst[0] = make_uint4(d[0], d[1], d[2], d[3]);
  dst[1] = make_uint4(d[4], d[5], d[6], d[7]);
}

// nodes[i] = H(nodes[2i] || nodes[2i+1]), output_size <= i < 2*output_size
template <class S>
__global__ __launch_bounds__(256) void hash_fold_kernel(uint32_t* __restrict__ nodes, uint32_t output_size, typename S::Consts k) {
  uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= output_size) return;
  uint32_t i = output_size + t;
  const uint4* src = (const uint4*)(nodes + (size_t)2 * i * 8);
  uint32_t d[2][8];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    uint4 v = src[q];
    uint32_t* h = &d[q >> 1][4 * (q & 1)];
    h[0] = v.x; h[1] = v.y; h[2] = v.z; h[3] = v.w;
  }
  S::pair(d[0], d[0], d[1], k);
  uint4* dst = (uint4*)(nodes + (size_t)i * 8);
  dst[0] = make_uint4(d[0][0], d[0][1], d[0][2], d[0][3]);
  dst[1] = make_uint4(d[0][4], d[0][5], d[0][6], d[0][7]);
}

// Upper Merkle levels have fewer parents than the chip has lanes: one permutation per lane then takes a full
// single-wave latency (~26 us) per level, 17 levels per tree.  This variant spreads ONE permutation over 24 lanes of a
// 32-lane half-wave (p2_mix_lanes, poseidon2_device.hpp).  Latency per level drops ~7x.
// Poseidon2 only: a SHA-256 compression is a few microseconds of adds and rotates, there is nothing to gain from spreading one.
__global__ __launch_bounds__(256) void hash_fold_lanes_kernel(uint32_t* __restrict__ nodes, uint32_t output_size,
                                                               const P2Consts* __restrict__ k) {
  const uint32_t l = threadIdx.x & 31u, slot = (blockIdx.x * 256 + threadIdx.x) >> 5;  // one permutation per 32 lanes
  const bool live = slot < output_size;
  const uint32_t node = output_size + (live ? slot : 0u);
  uint32_t c = (live && l < 16u) ? nodes[(size_t)2 * node * 8 + l] : 0u;
  c = p2_mix_lanes(c, l, k);
  if (live && l < 8u) nodes[(size_t)node * 8 + l] = c;
}

// The top of a tree without a launch per level (r0h_hash_fold_top; the plan is merkle_fused_plan.hpp).  Workgroup b owns node
// r = G + b of the level of G nodes, reads the 2^d nodes d levels below it and folds them up to r.  The first level reads its children
// from `nodes`; every later one reads them from LDS, where the workgroup keeps its subtree as a heap of 2^d digests (node 1 is r, the
// children of h are 2h and 2h + 1, slot 0 is not used; a level only writes slots no earlier level wrote, so one barrier per level is
// all the order it needs).  Every parent is also written to its place in `nodes`, for the openings, and never read from there: other
// workgroups' stores are not visible inside a launch, and nothing here depends on them.
// Poseidon2: one permutation per half-wave (p2_mix_lanes), as in hash_fold_lanes_kernel -- a workgroup has fewer parents than lanes
// at every level.  Every lane runs every permutation of every level: the loop bounds are workgroup-uniform, `live` predicates loads
// and stores only, and nothing returns before the last barrier.  SHA-256: one lane per parent.
#ifndef R0H_MERKLE_FUSED_WG
#define R0H_MERKLE_FUSED_WG 1024  // Poseidon2: 32 half-waves, two permutations deep at a level of 64 parents (profiles/r24/merkle_fused_tops.md)
#endif
constexpr uint32_t MERKLE_FUSED_WG = R0H_MERKLE_FUSED_WG;
static_assert(MERKLE_FUSED_WG % 64 == 0 && MERKLE_FUSED_WG >= 64 && MERKLE_FUSED_WG <= 1024, "whole waves, one workgroup");
template <class S>
__global__ __launch_bounds__(MERKLE_FUSED_WG) void merkle_subtree_kernel(uint32_t* __restrict__ nodes, uint32_t G, uint32_t d, typename S::Consts k) {
  extern __shared__ uint4 subtree[];
  const uint32_t r = G + blockIdx.x;
  for (uint32_t j = d; j-- > 0;) {
    const uint32_t n = 1u << j;            // this level's parents: heap nodes n + p, tree nodes first + p, p < n
    const size_t first = (size_t)r << j;
    const bool from_nodes = j + 1 == d;
    if constexpr (S::poseidon2) {
      uint32_t* heap = (uint32_t*)subtree;
      const uint32_t l = threadIdx.x & 31u, slot = threadIdx.x >> 5, slots = blockDim.x >> 5;
      for (uint32_t p0 = 0; p0 < n; p0 += slots) {
        const uint32_t p = p0 + slot;
        const bool live = p < n;
        const uint32_t h = n + (live ? p : 0u);
        uint32_t c = 0u;
        if (live && l < 16u) {
          if (from_nodes) c = nodes[(first + p) * 16 + l];
          else c = heap[h * 16 + l];
        }
        c = p2_mix_lanes(c, l, k);
        if (live && l < 8u) {
          heap[h * 8 + l] = c;
          nodes[(first + p) * 8 + l] = c;
        }
      }
    } else {
      for (uint32_t p = threadIdx.x; p < n; p += blockDim.x) {
        const uint32_t h = n + p;
        const uint4* src = from_nodes ? (const uint4*)(nodes + (first + p) * 16) : subtree + 4 * h;
        uint32_t dg[2][8];
#pragma unroll
        for (int q = 0; q < 4; q++) {
          uint4 v = src[q];
          uint32_t* w = &dg[q >> 1][4 * (q & 1)];
          w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        }
        S::pair(dg[0], dg[0], dg[1], k);
        const uint4 lo = make_uint4(dg[0][0], dg[0][1], dg[0][2], dg[0][3]), hi = make_uint4(dg[0][4], dg[0][5], dg[0][6], dg[0][7]);
        subtree[2 * h] = lo;
        subtree[2 * h + 1] = hi;
        uint4* dst = (uint4*)(nodes + (first + p) * 8);
        dst[0] = lo;
        dst[1] = hi;
      }
    }
    __syncthreads();
  }
}

// R0H_MERKLE_FUSED_TOPS=1: trees are built with r0h_hash_fold_top unless their context says otherwise (r0h_ctx_set_merkle_fused_tops)
static bool merkle_fused_default() {
  const char* v = getenv("R0H_MERKLE_FUSED_TOPS");
  return v && strtoul(v, nullptr, 10) == 1;
}

// the two shape checks every Merkle entry point makes, under the caller's name (internal.hpp)
const char* require_pow2_rows(const char* caller, uint32_t rows) {
  R0H_REQUIRE(rows && (rows & (rows - 1)) == 0, "%s: rows %u is not a power of two", caller, rows);
  return nullptr;
}
const char* require_rows_in_tree(const char* caller, const uint32_t* idx_host, uint32_t n_q, uint32_t rows) {
  for (uint32_t q = 0; q < n_q; q++) R0H_REQUIRE(idx_host[q] < rows, "%s: query %u opens row %u of a %u-row tree", caller, q, idx_host[q], rows);
  return nullptr;
}

}  // namespace r0h

using namespace r0h;

extern "C" {

const char* r0h_hash_rows(r0h_ctx* ctx, r0h_buf* digests, const r0h_buf* matrix, uint32_t rows, uint32_t cols) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && digests && matrix, "r0h_hash_rows: NULL argument");
  R0H_REQUIRE((size_t)rows * cols * 4 <= matrix->bytes, "r0h_hash_rows: %u x %u matrix exceeds the buffer", rows, cols);
  R0H_REQUIRE((size_t)rows * 32 <= digests->bytes, "r0h_hash_rows: %u digests exceed the output buffer", rows);
  R0H_REQUIRE(((uintptr_t)digests->ptr & 15) == 0, "r0h_hash_rows: digest buffer must be 16-byte aligned");
  if (!rows) return nullptr;
  return with_suite(ctx, [&](auto suite) {
    using S = decltype(suite);
    KScope ks(ctx, S::rows_kernel, (double)rows * cols * 4 + (double)rows * 32);
    hipLaunchKernelGGL(hash_rows_kernel<S>, dim3((rows + 255) / 256), dim3(256), 0, ctx->stream, u32(digests), u32(matrix), rows, cols, S::consts(ctx));
    return launch_ok(S::rows_kernel);
  });
  R0H_GUARD_END
}

const char* r0h_hash_fold(r0h_ctx* ctx, r0h_buf* nodes, uint32_t output_size) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && nodes, "r0h_hash_fold: NULL argument");
  R0H_REQUIRE((size_t)output_size * 4 * 32 <= nodes->bytes, "r0h_hash_fold: output_size %u needs %zu bytes of nodes", output_size, (size_t)output_size * 128);
  R0H_REQUIRE(((uintptr_t)nodes->ptr & 15) == 0, "r0h_hash_fold: node buffer must be 16-byte aligned");
  if (!output_size) return nullptr;
  return with_suite(ctx, [&](auto suite) {
    using S = decltype(suite);
    KScope ks(ctx, S::fold_kernel, (double)output_size * 96);
    if (S::poseidon2 && output_size <= 8192) {  // Poseidon2 with fewer parents than the chip has SIMD slots (measured up to 8 K: 1.47 vs 1.52 ms per tree) (32x the instructions per permutation, ~7x less latency): spread each permutation over 24 lanes (latency, not throughput)
      hipLaunchKernelGGL(hash_fold_lanes_kernel, dim3((output_size * 32 + 255) / 256), dim3(256), 0, ctx->stream, u32(nodes), output_size, ctx->p2);
      return launch_ok("hash_fold_lanes_kernel");
    }
    hipLaunchKernelGGL(hash_fold_kernel<S>, dim3((output_size + 255) / 256), dim3(256), 0, ctx->stream, u32(nodes), output_size, S::consts(ctx));
    return launch_ok(S::fold_kernel);
  });
  R0H_GUARD_END
}

const char* r0h_hash_fold_top(r0h_ctx* ctx, r0h_buf* nodes, uint32_t output_size) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && nodes, "r0h_hash_fold_top: NULL argument");
  R0H_REQUIRE((output_size & (output_size - 1)) == 0 && output_size <= MERKLE_FUSED_MAX_PARENTS, "r0h_hash_fold_top: output_size %u is not a power of two up to %u", output_size,
              MERKLE_FUSED_MAX_PARENTS);
  R0H_REQUIRE((size_t)output_size * 4 * 32 <= nodes->bytes, "r0h_hash_fold_top: output_size %u needs %zu bytes of nodes", output_size, (size_t)output_size * 128);
  R0H_REQUIRE(((uintptr_t)nodes->ptr & 15) == 0, "r0h_hash_fold_top: node buffer must be 16-byte aligned");
  MerkleFusedLaunch plan[2];
  const int launches = merkle_fused_plan_top(output_size, MERKLE_FUSED_SPLIT, plan);
  return with_suite(ctx, [&](auto suite) -> const char* {
    using S = typename decltype(suite)::Subtree;
    for (int i = 0; i < launches; i++) {
      const uint32_t G = plan[i].G, d = plan[i].d;
      R0H_REQUIRE(d >= 1 && d <= MERKLE_FUSED_MAX_D, "r0h_hash_fold_top: a launch of %u levels", d);
      // Poseidon2: a half-wave per parent of the widest level, up to the workgroup's size; SHA-256: a lane per parent of it
      const uint32_t want = S::poseidon2 ? 32u << (d - 1) : 1u << (d - 1);
      const uint32_t wg = want >= MERKLE_FUSED_WG ? MERKLE_FUSED_WG : (want + 63u) & ~63u;
      KScope ks(ctx, S::subtree_kernel, (double)G * (((size_t)2 << d) - 1) * 32);
      hipLaunchKernelGGL(merkle_subtree_kernel<S>, dim3(G), dim3(wg), ((size_t)32 << d), ctx->stream, u32(nodes), G, d, S::consts(ctx));
      R0H_TRY(launch_ok(S::subtree_kernel));
    }
    return nullptr;
  });
  R0H_GUARD_END
}

// Hal::hash_fold(io, input_size, output_size): the trait names both sizes (the fold halves a level, so input_size == 2 * output_size)
const char* r0h_hash_fold_io(r0h_ctx* ctx, r0h_buf* io, uint32_t input_size, uint32_t output_size) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(input_size == 2 * (size_t)output_size, "r0h_hash_fold_io: a fold takes 2 * output_size = %zu digests in, not %u", 2 * (size_t)output_size, input_size);
  return r0h_hash_fold(ctx, io, output_size);
  R0H_GUARD_END
}

const char* r0h_merkle_build(r0h_ctx* ctx, r0h_buf* nodes, const r0h_buf* matrix, uint32_t rows, uint32_t cols) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && nodes && matrix, "r0h_merkle_build: NULL argument");
  R0H_TRY(require_pow2_rows("r0h_merkle_build", rows));
  R0H_REQUIRE((size_t)rows * 2 * 32 <= nodes->bytes, "r0h_merkle_build: node buffer too small for %u rows", rows);
  r0h_buf leaves = *nodes;
  leaves.ptr = (char*)nodes->ptr + (size_t)rows * 32;
  leaves.bytes = (size_t)rows * 32;
  R0H_TRY(r0h_hash_rows(ctx, &leaves, matrix, rows, cols));
  if (ctx->merkle_fused_tops < 0 ? merkle_fused_default() : ctx->merkle_fused_tops > 0) {  // r0h_ctx_set_merkle_fused_tops: the same nodes in fewer launches
    uint32_t sz = rows / 2;
    for (; sz > MERKLE_FUSED_MAX_PARENTS; sz /= 2) R0H_TRY(r0h_hash_fold(ctx, nodes, sz));
    return r0h_hash_fold_top(ctx, nodes, sz);
  }
  for (uint32_t sz = rows / 2; sz >= 1; sz /= 2) R0H_TRY(r0h_hash_fold(ctx, nodes, sz));
  return nullptr;
  R0H_GUARD_END
}

}  // extern "C"
