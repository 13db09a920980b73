// SHA-256 row hashing and Merkle folding for gfx950: the second hash suite behind r0h_hash_rows / r0h_hash_fold (risc0 `ProverOpts`
// hashfn "sha-256"; recalled from risc0-zkp core/hash/sha and risc0-sys sha256.h, unpinned -- tests/sha_suite_ref.py is normative).
//
// One lane owns one row (hash_rows) or one parent node (hash_fold), as in poseidon2.hip: consecutive lanes read consecutive rows of
// each column, so every column access of a wave is one contiguous 256-byte run.  A row of `cols` words is compressed in 16-word
// blocks chained from the IV, the last partial block zero-filled, no length block (`hash_raw_data_slice`); cols = 0 gives the IV.
// The upper levels of a tree run the same per-lane fold: a compression is a few microseconds of adds and rotates, there is nothing
// to gain from spreading one over lanes as the Poseidon2 variant does.
#include "sha256_device.hpp"

namespace r0h {

__global__ __launch_bounds__(256) void sha256_hash_rows_kernel(uint32_t* __restrict__ digests, const uint32_t* __restrict__ matrix,
                                                                uint32_t rows, uint32_t cols) {
  const uint32_t row = blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  uint32_t st[8];
  sha_hash_row(st, matrix + row, rows, cols);  // the row sponge (sha256_device.hpp)
  uint4* dst = (uint4*)(digests + (size_t)row * 8);
  dst[0] = make_uint4(sha_bswap(st[0]), sha_bswap(st[1]), sha_bswap(st[2]), sha_bswap(st[3]));
  dst[1] = make_uint4(sha_bswap(st[4]), sha_bswap(st[5]), sha_bswap(st[6]), sha_bswap(st[7]));
}

// nodes[i] = H(nodes[2i] || nodes[2i+1]), output_size <= i < 2*output_size: one compression of the IV, no padding
__global__ __launch_bounds__(256) void sha256_hash_fold_kernel(uint32_t* __restrict__ nodes, uint32_t output_size) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= output_size) return;
  const uint32_t i = output_size + t;
  const uint4* src = (const uint4*)(nodes + (size_t)2 * i * 8);
  uint32_t st[8], w[16];
  sha_init(st);
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const uint4 v = src[q];
    w[4 * q] = sha_bswap(v.x); w[4 * q + 1] = sha_bswap(v.y); w[4 * q + 2] = sha_bswap(v.z); w[4 * q + 3] = sha_bswap(v.w);
  }
  sha_compress(st, w);
  uint4* dst = (uint4*)(nodes + (size_t)i * 8);
  dst[0] = make_uint4(sha_bswap(st[0]), sha_bswap(st[1]), sha_bswap(st[2]), sha_bswap(st[3]));
  dst[1] = make_uint4(sha_bswap(st[4]), sha_bswap(st[5]), sha_bswap(st[6]), sha_bswap(st[7]));
}

// the callers (r0h_hash_rows / r0h_hash_fold in poseidon2.hip) have checked the buffers' sizes and alignment and that there is work
const char* sha256_hash_rows(r0h_ctx* ctx, r0h_buf* digests, const r0h_buf* matrix, uint32_t rows, uint32_t cols) {
  KScope ks(ctx, "sha256_hash_rows_kernel", (double)rows * cols * 4 + (double)rows * 32);
  hipLaunchKernelGGL(sha256_hash_rows_kernel, dim3((rows + 255) / 256), dim3(256), 0, ctx->stream, u32(digests), u32(matrix), rows, cols);
  return launch_ok("sha256_hash_rows_kernel");
}
const char* sha256_hash_fold(r0h_ctx* ctx, r0h_buf* nodes, uint32_t output_size) {
  KScope ks(ctx, "sha256_hash_fold_kernel", (double)output_size * 96);
  hipLaunchKernelGGL(sha256_hash_fold_kernel, dim3((output_size + 255) / 256), dim3(256), 0, ctx->stream, u32(nodes), output_size);
  return launch_ok("sha256_hash_fold_kernel");
}

}  // namespace r0h
