// The device side of a hash suite: the counterpart of the host `HashSuite` (hash_suite.cpp).  One struct per suite, and every
// kernel that depends on the suite (merkle.hip, merkle_top.hip, merkle_climb.hip) is a template over it:
//   Consts            the kernel argument the suite needs, and consts(ctx), its value for a context
//   row(d, src, stride, cols, k)   d = the row sponge's digest of the `cols` words src[0], src[stride], src[2 * stride], ..
//   pair(d, left, right, k)        d = H(left || right) over digests held in registers; d may be left, right, or neither
//                                  (both inputs are read into the hash's own state before a word of d is written)
//   *_kernel          the names the suite's kernels go by in r0h_kernel_stats
// Digests are in digest word order everywhere outside this file: the byte swaps of the SHA-256 convention, the zeroed capacity of
// Poseidon2 and the shortened ends of its permutation are stated here and nowhere else.
#pragma once
#include "poseidon2_device.hpp"
#include "sha256_device.hpp"

namespace r0h {

struct P2Device {
  typedef const P2Consts* __restrict__ Consts;  // (the qualifier is part of the kernels' signatures: without it hash_rows_kernel compiles to other code)
  static Consts consts(const r0h_ctx* ctx) { return ctx->p2; }
  static constexpr const char *rows_kernel = "hash_rows_kernel", *fold_kernel = "hash_fold_kernel", *open_top_kernel = "merkle_open_top_kernel",
                              *climb_kernel = "merkle_climb_kernel";
  static __device__ __forceinline__ void row(uint32_t (&d)[8], const uint32_t* src, uint32_t stride, uint32_t cols, Consts k) {
    uint32_t c[P2_CELLS];
    p2_hash_row(c, src, stride, cols, k);
#pragma unroll
    for (int w = 0; w < 8; w++) d[w] = c[w];
  }
  // one permutation of left || right || 0^8, of which the first eight cells are read
  static __device__ __forceinline__ void pair(uint32_t (&d)[8], const uint32_t (&left)[8], const uint32_t (&right)[8], Consts k) {
    uint32_t c[P2_CELLS];
#pragma unroll
    for (int w = 0; w < 8; w++) { c[w] = left[w]; c[8 + w] = right[w]; }
#pragma unroll
    for (int w = 16; w < P2_CELLS; w++) c[w] = 0;
    p2_mix<P2_ZERO_CAP | P2_DIGEST_ONLY>(c, k);
#pragma unroll
    for (int w = 0; w < 8; w++) d[w] = c[w];
  }
};

struct ShaDevice {
  typedef int Consts;  // (none: the round constants are literals)
  static Consts consts(const r0h_ctx*) { return 0; }
  static constexpr const char *rows_kernel = "sha256_hash_rows_kernel", *fold_kernel = "sha256_hash_fold_kernel",
                              *open_top_kernel = "sha256_merkle_open_top_kernel", *climb_kernel = "sha256_merkle_climb_kernel";
  static __device__ __forceinline__ void row(uint32_t (&d)[8], const uint32_t* src, uint32_t stride, uint32_t cols, Consts) {
    uint32_t st[8];
    sha_hash_row(st, src, stride, cols);
#pragma unroll
    for (int w = 0; w < 8; w++) d[w] = sha_bswap(st[w]);
  }
  // one compression of the IV over the 16 words left || right, no padding
  static __device__ __forceinline__ void pair(uint32_t (&d)[8], const uint32_t (&left)[8], const uint32_t (&right)[8], Consts) {
    uint32_t st[8], m[16];
    sha_init(st);
#pragma unroll
    for (int w = 0; w < 8; w++) { m[w] = sha_bswap(left[w]); m[8 + w] = sha_bswap(right[w]); }
    sha_compress(st, m);
#pragma unroll
    for (int w = 0; w < 8; w++) d[w] = sha_bswap(st[w]);
  }
};

// f(S{}) for the context's suite S (r0h_ctx_set_hashfn): how a launch picks its instantiation
template <class F>
auto with_suite(const r0h_ctx* ctx, F&& f) {
  return ctx->hashfn == HASH_SHA256 ? f(ShaDevice{}) : f(P2Device{});
}

}  // namespace r0h
