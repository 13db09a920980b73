// The device side of a hash suite: the counterpart of the host `HashSuite` (hash_suite.cpp).  One struct per suite, and every
// kernel that depends on the suite (merkle.hip, merkle_top.hip, merkle_climb.hip) is a template over it:
//   Consts            the kernel argument the suite needs, and consts(ctx), its value for a context
//   row(d, src, stride, cols, k)   d = the row sponge's digest of the `cols` words src[0], src[stride], src[2 * stride], ..
//   pair(d, left, right, k)        d = H(left || right) over digests held in registers; d may be left, right, or neither
//                                  (both inputs are read into the hash's own state before a word of d is written)
//   Transcript        the suite's transcript generator and its hash of a word slice, run by one wave (iop.hip): the host's P2Rng / ShaRng
//                     and p2_hash_elems_host / sha_hash_elems_host (hash_suite.cpp) word for word, over a state in device memory.
//                       state_words, pool_limit      the state's layout: the generator's words as the host holds them, pool_used last
//                       Rng(state, k) / store(state) the state into registers and back (every lane of the wave holds or shares it)
//                       mix(d) / elem() / bits(n)    d: eight digest words in global memory or LDS; the values returned are wave-uniform
//                       hash_slice(out, w, n, k)     out[0..7] (LDS) = digest of the n words at w; a barrier stands before the return
//                     Poseidon2 spreads every permutation over the lanes of a half-wave (p2_mix_lanes), the chain is latency-bound;
//                     SHA-256 runs the same compressions in every lane.  Both halves of the wave compute the same words.
//   *_kernel          the names the suite's kernels go by in r0h_kernel_stats
//   rows_waves        the waves per SIMD hash_rows_kernel is allocated for (amdgpu_waves_per_eu).  Poseidon2: the 7 the allocator
//                     reached by itself (66 VGPRs) until the tight schedule of the partial rounds left the scheduler free to move more
//                     of the multiply-adds (75 VGPRs, 6 waves); held to 7 it is at 66 again, without scratch.  SHA-256: what it has.
//   Subtree           the suite merkle_subtree_kernel (merkle.hip) is instantiated for.  Poseidon2: it runs the lanes form alone, which has no
//                     dot products, so one instantiation serves both schedules.
//   OpenTop           the suite merkle_open_top_kernel is instantiated for.  Poseidon2: always the safe schedule -- under the tight
//                     one the kernel (a row sponge and the pair hashes of a subtree in one body) takes 141 VGPRs instead of 118, 3 waves
//                     instead of 4, and 44 bytes of scratch when held to 4.  The words are the same under either schedule.
// Digests are in digest word order everywhere outside this file: the byte swaps of the SHA-256 convention, the zeroed capacity of
// Poseidon2 and the shortened ends of its permutation are stated here and nowhere else.
#pragma once
#include "poseidon2_device.hpp"
#include "sha256_device.hpp"

namespace r0h {

// The Poseidon2 generator: lane l of each half-wave holds cell l (lanes 24..31: don't-cares), pool_used is uniform.
struct P2Transcript {
  static constexpr uint32_t state_words = P2_CELLS + 1, pool_limit = P2_RATE;
  static constexpr const char *commit_kernel = "iop_commit_kernel", *commit_elems_kernel = "iop_commit_elems_kernel", *draw_kernel = "iop_draw_kernel",
                              *queries_kernel = "iop_queries_kernel";
  typedef const P2Consts* __restrict__ Consts;
  static Consts consts(const r0h_ctx* ctx) { return ctx->p2; }
  struct Rng {
    uint32_t c, used, l;
    Consts k;
    __device__ __forceinline__ Rng(const uint32_t* state, Consts kk) : l(threadIdx.x & 31u), k(kk) {
      c = l < (uint32_t)P2_CELLS ? state[l] : 0u;
      used = state[P2_CELLS];
    }
    __device__ __forceinline__ void store(uint32_t* state) const {
      if (threadIdx.x < (uint32_t)P2_CELLS) state[threadIdx.x] = c;
      if (threadIdx.x == 0) state[P2_CELLS] = used;
    }
    __device__ __forceinline__ void mix(const uint32_t* d) {
      if (used != 0) { c = p2_mix_lanes(c, l, k); used = 0; }
      if (l < 8u) c = add(c, d[l]);
      c = p2_mix_lanes(c, l, k);
    }
    __device__ __forceinline__ uint32_t elem() {
      if (used == (uint32_t)P2_RATE) { c = p2_mix_lanes(c, l, k); used = 0; }
      return half_shfl(c, used++);
    }
    __device__ __forceinline__ uint32_t bits(uint32_t n) {
      uint32_t val = dec(elem());
      for (int i = 0; i < 3; i++) { const uint32_t nv = dec(elem()); if (val == 0) val = nv; }
      return val & (uint32_t)(((uint64_t)1 << n) - 1);
    }
  };
  // the sponge of p2_hash_elems_host: rate blocks overwrite cells 0..15 (the last zero-padded), one permutation per block, at least one
  static __device__ __forceinline__ void hash_slice(uint32_t* out, const uint32_t* w, uint32_t n, Consts k) {
    const uint32_t l = threadIdx.x & 31u, blocks = n ? (n + P2_RATE - 1) / P2_RATE : 1u;
    uint32_t c = 0, next = (l < (uint32_t)P2_RATE && l < n) ? w[l] : 0u;
    for (uint32_t blk = 0; blk < blocks; blk++) {
      if (l < (uint32_t)P2_RATE) c = next;
      const uint32_t at = (blk + 1) * P2_RATE + l;  // the next block's word is on its way while this one is permuted
      next = (l < (uint32_t)P2_RATE && at < n) ? w[at] : 0u;
      c = p2_mix_lanes(c, l, k);
    }
    if (threadIdx.x < 8u) out[threadIdx.x] = c;
    __syncthreads();
  }
};

// DOT: the correction schedule of the partial rounds' dot products the suite's kernels are compiled for (poseidon2_dot_schedule.hpp).
// Both instantiations compute the same words; P2DotTight is only valid for a table fill_p2 found it to cover (r0h_ctx::p2_tight).
template <class DOT>
struct P2DeviceT {
  static constexpr bool poseidon2 = true;
  static constexpr int rows_waves = 7;
  typedef P2DeviceT<P2DotSafe> OpenTop;
  typedef P2DeviceT<P2DotSafe> Subtree;
  typedef P2Transcript Transcript;  // (no dot products in the lanes form: one for both schedules)
  typedef const P2Consts* __restrict__ Consts;  // (the qualifier is part of the kernels' signatures: without it hash_rows_kernel compiles to other code)
  static Consts consts(const r0h_ctx* ctx) { return ctx->p2; }
  static constexpr const char *rows_kernel = "hash_rows_kernel", *fold_kernel = "hash_fold_kernel", *subtree_kernel = "merkle_subtree_kernel",
                              *open_top_kernel = "merkle_open_top_kernel", *climb_kernel = "merkle_climb_kernel";
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

// The SHA-256 generator: every lane holds both pools and runs the same compressions.
struct ShaTranscript {
  static constexpr uint32_t state_words = 17, pool_limit = 8;
  static constexpr const char *commit_kernel = "sha256_iop_commit_kernel", *commit_elems_kernel = "sha256_iop_commit_elems_kernel",
                              *draw_kernel = "sha256_iop_draw_kernel", *queries_kernel = "sha256_iop_queries_kernel";
  typedef int Consts;
  static Consts consts(const r0h_ctx*) { return 0; }
  // H(left || right) as ShaDevice::pair has it (one compression of the IV, digests byte-swapped both ways)
  static __device__ __forceinline__ void pair(uint32_t (&d)[8], const uint32_t (&left)[8], const uint32_t (&right)[8]) {
    uint32_t st[8], m[16];
    sha_init(st);
#pragma unroll
    for (int w = 0; w < 8; w++) { m[w] = sha_bswap(left[w]); m[8 + w] = sha_bswap(right[w]); }
    sha_compress(st, m);
#pragma unroll
    for (int w = 0; w < 8; w++) d[w] = sha_bswap(st[w]);
  }
  struct Rng {
    uint32_t pool0[8], pool1[8], used;
    __device__ __forceinline__ Rng(const uint32_t* state, Consts) {
#pragma unroll
      for (int w = 0; w < 8; w++) { pool0[w] = state[w]; pool1[w] = state[8 + w]; }
      used = state[16];
    }
    __device__ __forceinline__ void store(uint32_t* state) const {
      if (threadIdx.x != 0) return;
#pragma unroll
      for (int w = 0; w < 8; w++) { state[w] = pool0[w]; state[8 + w] = pool1[w]; }
      state[16] = used;
    }
    __device__ __forceinline__ void step() {
      pair(pool0, pool0, pool1);
      pair(pool1, pool0, pool1);
      used = 0;
    }
    __device__ __forceinline__ uint32_t random_u32() {
      if (used == 8u) step();
      uint32_t v = pool0[0];  // pool0[used] without a register index
#pragma unroll
      for (int w = 1; w < 8; w++) v = used == (uint32_t)w ? pool0[w] : v;
      used++;
      return v;
    }
    __device__ __forceinline__ void mix(const uint32_t* d) {
#pragma unroll
      for (int w = 0; w < 8; w++) pool0[w] ^= d[w];
      step();
    }
    __device__ __forceinline__ uint32_t elem() {
      uint64_t val = 0;
      for (int i = 0; i < 6; i++) val = ((val << 32) + random_u32()) % P;
      return enc((uint32_t)val);
    }
    __device__ __forceinline__ uint32_t bits(uint32_t n) { return random_u32() & (uint32_t)(((uint64_t)1 << n) - 1); }
  };
  // sha_hash_elems_host: 16-word blocks chained from the IV, the last partial block zero-filled, no length block; n = 0 gives the IV
  static __device__ __forceinline__ void hash_slice(uint32_t* out, const uint32_t* w, uint32_t n, Consts) {
    uint32_t st[8];
    sha_hash_row(st, w, 1, n);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int j = 0; j < 8; j++) out[j] = sha_bswap(st[j]);
    }
    __syncthreads();
  }
};

struct ShaDevice {
  static constexpr bool poseidon2 = false;
  static constexpr int rows_waves = 6;
  typedef ShaDevice OpenTop;
  typedef ShaDevice Subtree;
  typedef ShaTranscript Transcript;
  typedef int Consts;  // (none: the round constants are literals)
  static Consts consts(const r0h_ctx*) { return 0; }
  static constexpr const char *rows_kernel = "sha256_hash_rows_kernel", *fold_kernel = "sha256_hash_fold_kernel", *subtree_kernel = "sha256_merkle_subtree_kernel",
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
