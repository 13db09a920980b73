// Device side of the SHA-256 hash suite (gfx950): one compression per call, everything in registers.
// The suite is recalled from risc0-zkp core/hash/sha and risc0-sys sha256.h (unpinned; tests/sha_suite_ref.py is normative here,
// hash_suite.cpp states it in words).  A digest word is bswap32 of a state word and a message word is bswap32 of an input word.
//
// Per lane: 8 state words, 8 working words and a rolling window of 16 schedule words, all VGPRs (the 64 rounds are unrolled, so
// every index into the window is a compile-time constant and nothing goes to scratch).  Rotates are v_alignbit_b32 with both
// sources the same register.  Ch and Maj are bit selects and the sigmas three-way xors: one v_bitop3_b32 each (gfx950's
// any-function-of-three-words instruction, which takes the place gfx90a's v_bfi_b32 has; truth tables 0xCA, 0xE8, 0x96).
// The round constants are the same for every lane: after unrolling they are 32-bit literals that the scalar unit moves into
// SGPRs -- no table in memory, no vector load, no VGPR.  No multiplies anywhere: about 1.5 k VALU instructions per 16 words
// against about 1.36 k Montgomery products (several instructions each, on the quarter-rate 32x32 multiplier) for one Poseidon2
// permutation.
#pragma once
#include "internal.hpp"

namespace r0h {

__device__ constexpr uint32_t SHA256_K[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
    0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
    0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
    0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
    0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
    0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

__device__ __forceinline__ uint32_t sha_rotr(uint32_t x, uint32_t n) { return __builtin_amdgcn_alignbit(x, x, n); }
__device__ __forceinline__ uint32_t sha_ch(uint32_t e, uint32_t f, uint32_t g) { return __builtin_amdgcn_bitop3_b32(e, f, g, 0xCA); }   // e ? f : g
__device__ __forceinline__ uint32_t sha_maj(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8); }  // (a ^ b) ? c : b
__device__ __forceinline__ uint32_t sha_xor3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }
__device__ __forceinline__ uint32_t sha_bswap(uint32_t x) { return __builtin_bswap32(x); }                                // v_perm_b32

__device__ __forceinline__ void sha_init(uint32_t st[8]) {
  st[0] = 0x6a09e667u; st[1] = 0xbb67ae85u; st[2] = 0x3c6ef372u; st[3] = 0xa54ff53au;
  st[4] = 0x510e527fu; st[5] = 0x9b05688cu; st[6] = 0x1f83d9abu; st[7] = 0x5be0cd19u;
}

// st += compression(st, w): w holds the 16 MESSAGE words (input words already byte-swapped) and is used up as the rolling schedule
__device__ __forceinline__ void sha_compress(uint32_t st[8], uint32_t w[16]) {
  uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
  for (int i = 0; i < 64; i++) {
    if (i >= 16) {
      const uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
      const uint32_t s0 = sha_xor3(sha_rotr(w15, 7), sha_rotr(w15, 18), w15 >> 3), s1 = sha_xor3(sha_rotr(w2, 17), sha_rotr(w2, 19), w2 >> 10);
      w[i & 15] = w[i & 15] + s0 + w[(i + 9) & 15] + s1;
    }
    const uint32_t t1 = h + sha_xor3(sha_rotr(e, 6), sha_rotr(e, 11), sha_rotr(e, 25)) + sha_ch(e, f, g) + SHA256_K[i] + w[i & 15];
    const uint32_t t2 = sha_xor3(sha_rotr(a, 2), sha_rotr(a, 13), sha_rotr(a, 22)) + sha_maj(a, b, c);
    h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
  }
  st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

// The row sponge: st = state after the `cols` words src[0], src[rows], src[2 * rows], .. (one row of a column-major matrix), compressed in
// 16-word blocks chained from the IV, the last partial block zero-filled, no length block (`hash_raw_data_slice`); cols = 0 gives the IV.
// Digest word j is sha_bswap(st[j]): ShaDevice::row (hash_suite_device.hpp), what sha256_hash_rows_kernel computes per lane,
// sha256_merkle_open_top_kernel per leaf and sha256_merkle_climb_kernel per opening.
__device__ __forceinline__ void sha_hash_row(uint32_t st[8], const uint32_t* src, uint32_t rows, uint32_t cols) {
  uint32_t w[16];
  sha_init(st);
  const uint32_t blocks = (cols + 15) / 16, full = cols / 16;
  for (uint32_t blk = 0; blk < blocks; blk++) {
    if (blk < full) {  // (wave-uniform: cols is a kernel argument)
#pragma unroll
      for (int i = 0; i < 16; i++) w[i] = sha_bswap(src[(size_t)(blk * 16 + i) * rows]);
    } else {
#pragma unroll
      for (int i = 0; i < 16; i++) w[i] = blk * 16 + i < cols ? sha_bswap(src[(size_t)(blk * 16 + i) * rows]) : 0u;
    }
    sha_compress(st, w);
  }
}

}  // namespace r0h
