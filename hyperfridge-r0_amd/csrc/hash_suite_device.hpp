// The device side of a hash suite: the counterpart of the host `HashSuite` (hash_suite.cpp).  One struct per suite, and every
// kernel that depends on the suite (merkle.hip, merkle_top.hip, merkle_climb.hip) is a template over it:
//   Consts            the kernel argument the suite needs, and consts(ctx), its value for a context
//   row(d, src, stride, cols, k)   d = the row sponge's digest of the `cols` words src[0], src[stride], src[2 * stride], ..
//   pair(d, left, right, k)        d = H(left || right) over digests held in registers; d may be left, right, or neither
//                                  (both inputs are read into the hash's own state before a word of d is written)
//   *_kernel          the names the suite's kernels go by in r0h_kernel_stats
//   rows_waves        the waves per SIMD hash_rows_kernel is allocated for (amdgpu_waves_per_eu).  Poseidon2: the 7 the allocator
//                     reached by itself (66 VGPRs) until the tight schedule of the partial rounds left the scheduler free to move more
//                     of the multiply-adds (75 VGPRs, 6 waves); held to 7 it is at 66 again, without scratch.  SHA-256: what it has.
//   OpenTop           the suite merkle_open_top_kernel is instantiated for.  Poseidon2: always the safe schedule -- under the tight
//                     one the kernel (a row sponge and the pair hashes of a subtree in one body) takes 141 VGPRs instead of 118, 3 waves
//                     instead of 4, and 44 bytes of scratch when held to 4.  The words are the same under either schedule.
// Digests are in digest word order everywhere outside this file: the byte swaps of the SHA-256 convention, the zeroed capacity of
// Poseidon2 and the shortened ends of its permutation are stated here and nowhere else.
#pragma once
#include "poseidon2_device.hpp"
#include "sha256_device.hpp"

namespace r0h {

// DOT: the correction schedule of the partial rounds' dot products the suite's kernels are compiled for (poseidon2_dot_schedule.hpp).
// Both instantiations compute the same words; P2DotTight is only valid for a table fill_p2 found it to cover (r0h_ctx::p2_tight).
template <class DOT>
struct P2DeviceT {
  static constexpr bool poseidon2 = true;
  static constexpr int rows_waves = 7;
  typedef P2DeviceT<P2DotSafe> OpenTop;
  typedef const P2Consts* __restrict__ Consts;  // (the qualifier is part of the kernels' signatures: without it hash_rows_kernel compiles to other code)
  static Consts consts(const r0h_ctx* ctx) { return ctx->p2; }
  static constexpr const char *rows_kernel = "hash_rows_kernel", *fold_kernel = "hash_fold_kernel", *open_top_kernel = "merkle_open_top_kernel",
                              *climb_kernel = "merkle_climb_kernel";
  static __device__ __forceinline__ void row(uint32_t (&d)[8], const uint32_t* src, uint32_t stride, uint32_t cols, Consts k) {
    uint32_t c[P2_CELLS];
    p2_hash_row<DOT>(c, src, stride, cols, k);
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
    p2_mix<P2_ZERO_CAP | P2_DIGEST_ONLY, DOT>(c, k);
#pragma unroll
    for (int w = 0; w < 8; w++) d[w] = c[w];
  }
};
typedef P2DeviceT<P2DotTight> P2Device;    // the compiled-in diagonal D_1..D_23, whatever the round constants and D_0: the schedule leaves so
                                           // little slack that no other diagonal tried stayed covered (profiles/r19/poseidon2_dot_schedule.md)
typedef P2DeviceT<P2DotSafe> P2DeviceSafe;  // every other canonical table (r0h_poseidon2_set_consts)

struct ShaDevice {
  static constexpr bool poseidon2 = false;
  static constexpr int rows_waves = 6;
  typedef ShaDevice OpenTop;
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
  if (ctx->hashfn == HASH_SHA256) return f(ShaDevice{});
  return ctx->p2_tight ? f(P2Device{}) : f(P2DeviceSafe{});
}

}  // namespace r0h
