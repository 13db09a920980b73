// A Merkle tree kept as its top alone, and openings made from it (what an evicted segment of a session keeps of its
// DATA commitment).  A path needs the whole tree only because the sibling at level l covers 2^l leaves: with the tree kept from the
// root down to `levels` levels above the leaves -- digests [0, 2 * rows >> levels), 2^-levels of the nodes -- the bottom `levels`
// siblings of a queried leaf are the inner nodes of ONE subtree of 2^levels leaves, hashed again from the matrix rows under it when
// the opening is made.  50 queries at levels = 6: 3200 row hashes and 3150 pair hashes instead of the 4 M + 4 M of the full tree.
//
// merkle_open_top_kernel: one workgroup per query, 2^levels lanes (levels = 6: one wave64).  Lane j hashes leaf row
// ((idx >> levels) << levels) + j with the row sponge of hash_rows (consecutive lanes read consecutive rows of each column: one
// contiguous run of 4 * 2^levels bytes per column), the digests go to LDS word-major [8][2^levels], and `levels` rounds of pair hashing
// follow -- before each, the sibling of the queried path at that level is written out.  The subtree's root must be the node the
// kept top has there: that is the check that top and matrix belong together, made at every query (a mismatch is counted and the
// lowest query number kept; the host reports it).  The levels above come from the top as merkle_open_kernel, the opening of a tree
// held in full, takes them from its nodes (path_above, below), and the packed opening is the same: `cols` column values, then
// path_digests sibling digests.  One template, instantiated per hash suite (row and pair of hash_suite_device.hpp).
#include "hash_suite_device.hpp"
#include "seal_layout.hpp"

namespace r0h {

// The sibling digests of `row`'s path from `first` levels above the leaves up to (excluding) level n_path, out of the node array of a
// `rows`-leaf tree (node i at words [8i, 8i + 8), the root at 1), into path[8 * first, 8 * n_path): one word per lane and step
__device__ __forceinline__ void path_above(uint32_t* path, const uint32_t* nodes, uint32_t row, uint32_t rows, uint32_t first, uint32_t n_path) {
  for (uint32_t w = threadIdx.x + 8 * first; w < 8 * n_path; w += blockDim.x) {
    const uint32_t sibling = ((row + rows) >> (w >> 3)) ^ 1u;
    path[w] = nodes[(size_t)sibling * 8 + (w & 7)];
  }
}

// out[q] = column values at row idx[q] followed by the sibling digests up to (excluding) the top layer.  Does not depend on the suite.
__global__ void merkle_open_kernel(uint32_t* __restrict__ out, const uint32_t* __restrict__ matrix, const uint32_t* __restrict__ nodes,
                                   const uint32_t* __restrict__ idx, uint32_t row_size, uint32_t col_size, uint32_t n_path) {
  const uint32_t q = blockIdx.x, row = idx[q];
  uint32_t* dst = out + (size_t)q * (col_size + 8 * n_path);
  for (uint32_t i = threadIdx.x; i < col_size; i += blockDim.x) dst[i] = matrix[(size_t)i * row_size + row];
  path_above(dst + col_size, nodes, row, row_size, 0, n_path);
}

// report[0]: queries whose subtree root is not the top's node; report[1]: the lowest such query number (0xffffffff: none)
template <class S>
__global__ __launch_bounds__(256) void merkle_open_top_kernel(uint32_t* __restrict__ out, const uint32_t* __restrict__ matrix, const uint32_t* __restrict__ top,
                                                               const uint32_t* __restrict__ idx, uint32_t rows, uint32_t cols, uint32_t n_path, uint32_t levels,
                                                               uint32_t* __restrict__ report, typename S::Consts k) {
  extern __shared__ uint32_t lds[];  // [8][n]: word w of the node in slot s at lds[w * n + s]
  const uint32_t q = blockIdx.x, row = idx[q], n = 1u << levels, j = threadIdx.x;  // blockDim.x == n <= rows
  uint32_t* dst = out + (size_t)q * (cols + 8 * n_path);
  for (uint32_t i = j; i < cols; i += n) dst[i] = matrix[(size_t)i * rows + row];
  const uint32_t base = (row >> levels) << levels, local = row - base;  // the subtree's first leaf row; base + j < rows
  uint32_t d[8];
  S::row(d, matrix + base + j, rows, cols, k);
#pragma unroll
  for (int w = 0; w < 8; w++) lds[w * n + j] = d[w];
  __syncthreads();
  for (uint32_t l = 0; l < levels; l++) {  // slots [0, n >> l) hold the subtree's nodes l levels above the leaves
    for (uint32_t w = j; w < 8; w += n) dst[cols + 8 * l + w] = lds[w * n + ((local >> l) ^ 1u)];
    const bool parent = j < (n >> (l + 1));
    if (parent) {  // the nodes in slots 2j and 2j + 1
      uint32_t right[8];
#pragma unroll
      for (int w = 0; w < 8; w++) { d[w] = lds[w * n + 2 * j]; right[w] = lds[w * n + 2 * j + 1]; }
      S::pair(d, d, right, k);
    }
    __syncthreads();  // every pair has been read before a slot is written
    if (parent) {
#pragma unroll
      for (int w = 0; w < 8; w++) lds[w * n + j] = d[w];
    }
    __syncthreads();
  }
  const uint32_t node = (row + rows) >> levels;  // the subtree's root, as the kept top has it
  if (j == 0) {
    bool differs = false;
#pragma unroll
    for (int w = 0; w < 8; w++) differs = differs || lds[w * n] != top[(size_t)node * 8 + w];
    if (differs) {
      atomicAdd(&report[0], 1u);
      atomicMin(&report[1], q);
    }
  }
  path_above(dst + cols, top, row, rows, levels, n_path);  // the path above the subtree: out of the top
}

// how many digests the top of a `rows`-leaf tree kept to `levels` above the leaves holds (index 0 unused, the root at 1)
static size_t top_digests(uint32_t rows, uint32_t levels) { return ((size_t)2 * rows) >> levels; }

static const char* require_top_shape(const char* caller, uint32_t rows, uint32_t levels) {
  R0H_TRY(require_pow2_rows(caller, rows));
  const uint32_t path = (uint32_t)MerkleShape(rows, 0).path_digests(), most = path < R0H_MERKLE_TOP_MAX_LEVELS ? path : R0H_MERKLE_TOP_MAX_LEVELS;
  R0H_REQUIRE(levels >= 1 && levels <= most, "%s: levels %u outside [1, %u] (at most %u, and at most the %u path digests of an opening in a tree of %u rows)", caller, levels,
              most, (unsigned)R0H_MERKLE_TOP_MAX_LEVELS, path, rows);
  return nullptr;
}

const char* merkle_top_copy(r0h_ctx* ctx, const r0h_buf* nodes, uint32_t rows, uint32_t levels, r0h_buf* top_out, const char* caller) {
  R0H_TRY(require_top_shape(caller, rows, levels));
  const size_t bytes = top_digests(rows, levels) * 32;
  R0H_REQUIRE(bytes <= nodes->bytes, "%s: the node buffer holds fewer than the %zu digests of the top", caller, bytes / 32);
  R0H_REQUIRE(bytes <= top_out->bytes, "%s: the top of a %u-row tree at %u levels is %zu bytes, the output buffer holds %zu", caller, rows, levels, bytes, top_out->bytes);
  (void)hipSetDevice(ctx->device);
  R0H_TRY_HIP(hipMemcpyAsync(top_out->ptr, nodes->ptr, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  return nullptr;
}

const char* merkle_open_top(r0h_ctx* ctx, uint32_t* out, const uint32_t* matrix, const uint32_t* top, uint32_t levels, const uint32_t* d_idx, uint32_t n_q, uint32_t rows,
                            uint32_t cols, uint32_t* report) {
  const uint32_t clean[2] = {0u, 0xffffffffu};
  R0H_TRY(stage_h2d(ctx, report, clean, sizeof clean));
  const uint32_t n = 1u << levels, n_path = (uint32_t)MerkleShape(rows, cols).path_digests();
  const size_t lds_bytes = (size_t)8 * n * 4;
  return with_suite(ctx, [&](auto suite) {
    using S = typename decltype(suite)::OpenTop;
    KScope ks(ctx, S::open_top_kernel, (double)n_q * n * cols * 4);
    hipLaunchKernelGGL(merkle_open_top_kernel<S>, dim3(n_q), dim3(n), lds_bytes, ctx->stream, out, matrix, top, d_idx, rows, cols, n_path, levels, report, S::consts(ctx));
    return launch_ok(S::open_top_kernel);
  });
}

const char* merkle_open(r0h_ctx* ctx, uint32_t* out, const uint32_t* matrix, const uint32_t* nodes, const uint32_t* d_idx, uint32_t n_q, uint32_t rows, uint32_t cols) {
  hipLaunchKernelGGL(merkle_open_kernel, dim3(n_q), dim3(256), 0, ctx->stream, out, matrix, nodes, d_idx, rows, cols, (uint32_t)MerkleShape(rows, cols).path_digests());
  return launch_ok("merkle_open_kernel");
}

const char* merkle_open_top_verdict(const char* caller, const uint32_t report[2], const uint32_t* idx_host) {
  R0H_REQUIRE(!report[0], "%s: tree top does not match the matrix under query %u (row %u)%s", caller, report[1], idx_host[report[1]],
              report[0] > 1 ? ", nor under later ones" : "");
  return nullptr;
}

}  // namespace r0h

using namespace r0h;

extern "C" {

const char* r0h_merkle_top(r0h_ctx* ctx, const r0h_buf* nodes, uint32_t rows, uint32_t levels, r0h_buf* top_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && nodes && top_out, "r0h_merkle_top: NULL argument");
  return merkle_top_copy(ctx, nodes, rows, levels, top_out, "r0h_merkle_top");
  R0H_GUARD_END
}

const char* r0h_merkle_open_top(r0h_ctx* ctx, r0h_buf* out, const r0h_buf* matrix, const r0h_buf* top, uint32_t levels, const uint32_t* idx_host, uint32_t n_q, uint32_t rows,
                                uint32_t cols, uint32_t* first_mismatch_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && out && matrix && top && (idx_host || !n_q), "r0h_merkle_open_top: NULL argument");
  R0H_TRY(require_top_shape("r0h_merkle_open_top", rows, levels));
  const MerkleShape mp(rows, cols);
  R0H_REQUIRE((size_t)rows * cols * 4 <= matrix->bytes, "r0h_merkle_open_top: %u x %u matrix exceeds the buffer", rows, cols);
  R0H_REQUIRE(top_digests(rows, levels) * 32 <= top->bytes, "r0h_merkle_open_top: the top of a %u-row tree at %u levels is %zu bytes, the buffer holds %zu", rows, levels,
              top_digests(rows, levels) * 32, top->bytes);
  R0H_REQUIRE((size_t)n_q * mp.opening_words() * 4 <= out->bytes, "r0h_merkle_open_top: %u openings of %zu words exceed the output buffer", n_q, mp.opening_words());
  R0H_TRY(require_rows_in_tree("r0h_merkle_open_top", idx_host, n_q, rows));
  if (first_mismatch_out) *first_mismatch_out = 0xffffffffu;
  if (!n_q) return nullptr;
  (void)hipSetDevice(ctx->device);
  DevBuf block;  // the queried rows, then the kernel's report
  R0H_TRY(block.alloc(ctx, (size_t)n_q * 4 + 8));
  R0H_TRY(stage_h2d(ctx, block->ptr, idx_host, (size_t)n_q * 4));
  uint32_t* d_report = u32(block.get()) + n_q;
  R0H_TRY(merkle_open_top(ctx, u32(out), u32(matrix), u32(top), levels, u32(block.get()), n_q, rows, cols, d_report));
  uint32_t report[2];
  R0H_TRY(r0h_buf_d2h(ctx, block.get(), (size_t)n_q * 4, report, sizeof report));
  if (first_mismatch_out) *first_mismatch_out = report[1];
  return merkle_open_top_verdict("r0h_merkle_open_top", report, idx_host);
  R0H_GUARD_END
}

}  // extern "C"
