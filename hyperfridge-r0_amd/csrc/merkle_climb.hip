// Packed Merkle openings climbed to the layer a seal carries: the counterpart of merkle_open_kernel / merkle_open_top_kernel, and the
// hashing half of a seal's verification (csrc/verify.cpp collects the openings of a batch of seals, this kernel hashes
// them, the host compares what is reached with the top layers it read from the seals and decides).  The device computes digests and
// nothing else: it sees no top layer, makes no comparison and returns no verdict.
//
// A job is {word offset, cols, path digests, row index} over one buffer of packed openings: `cols` values, then the sibling digests
// l = 0 .. path_digests - 1, as the sequencer and r0h_merkle_open_top pack them.  Per job: the row sponge of hash_rows over the values,
// then per sibling H(cur || sib) when bit l of the row index is 0 and H(sib || cur) when it is 1; the eight words reached are written.
//
// merkle_climb_kernel: one lane per opening, one wave per workgroup.  The openings of one tree share cols and path length and the 50
// queries of a seal fit one wave, so the host sorts the jobs by (cols, path) and cuts every run into waves of at most 64: the block
// loop of the sponge and the climb are wave-uniform, only the side a sibling goes to differs between lanes (a select, no branch).
// A batch is at most 7 x 50 jobs per seal, each a chain of cols / 16 + path dependent permutations: a latency problem, so the
// grid is one wave per (tree, seal) spread over as many compute units, and nothing is shared between lanes (no LDS).
// One template, instantiated per hash suite (row and pair of hash_suite_device.hpp).
#include <algorithm>
#include <numeric>

#include "hash_suite_device.hpp"
#include "seal_layout.hpp"

namespace r0h {

// jobs: {word offset, cols, path digests, row index} in the host's sorted order; waves: {first job, jobs (1..64)} per workgroup, all of
// whose jobs have the cols and path of the first.  reached[j][8] for sorted job j.  Every offset + cols + 8 * path lies inside `words`
// (the host has checked it against the buffer before the launch).
template <class S>
__global__ __launch_bounds__(64) void merkle_climb_kernel(uint32_t* __restrict__ reached, const uint32_t* __restrict__ words, const uint4* __restrict__ jobs,
                                                          const uint2* __restrict__ waves, typename S::Consts k) {
  const uint2 wave = waves[blockIdx.x];
  if (threadIdx.x >= wave.y) return;
  const uint32_t cols = __builtin_amdgcn_readfirstlane(jobs[wave.x].y), path = __builtin_amdgcn_readfirstlane(jobs[wave.x].z);
  const uint4 job = jobs[wave.x + threadIdx.x];
  const uint32_t* __restrict__ opening = words + job.x;
  uint32_t cur[8];
  S::row(cur, opening, 1, cols, k);
#pragma unroll 1
  for (uint32_t l = 0; l < path; l++) {  // cur = H(sib || cur) where the path comes up from the right, H(cur || sib) from the left
    const uint32_t* __restrict__ sib = opening + cols + 8 * l;
    const bool right_side = (job.w >> l) & 1u;
    uint32_t left[8], right[8];
#pragma unroll
    for (int w = 0; w < 8; w++) {
      const uint32_t s = sib[w];
      left[w] = right_side ? s : cur[w];
      right[w] = right_side ? cur[w] : s;
    }
    S::pair(cur, left, right, k);
  }
  uint32_t* dst = reached + (size_t)(wave.x + threadIdx.x) * 8;
#pragma unroll
  for (int w = 0; w < 8; w++) dst[w] = cur[w];
}

// The jobs' openings lie in the device words [0, n_words) at d_words.  reached_host[j][8] in the caller's job order.  Blocks until
// the digests are back.
const char* merkle_climb(r0h_ctx* ctx, const uint32_t* d_words, size_t n_words, const ClimbJob* jobs, size_t n_jobs, uint32_t* reached_host) {
  if (!n_jobs) return nullptr;
  R0H_REQUIRE(n_jobs < ((size_t)1 << 28), "merkle_climb: %zu jobs in one batch", n_jobs);
  for (size_t j = 0; j < n_jobs; j++) {
    const ClimbJob& b = jobs[j];
    R0H_REQUIRE(b.path <= 32 && (size_t)b.offset + b.cols + (size_t)8 * b.path <= n_words, "merkle_climb: job %zu (offset %u, %u values, %u path digests) leaves the %zu words of openings",
                j, b.offset, b.cols, b.path, n_words);
  }
  // a wave holds one tree's openings: sorted by (cols, path), the caller's order kept inside a run
  std::vector<uint32_t> order(n_jobs);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return std::make_pair(jobs[a].cols, jobs[a].path) < std::make_pair(jobs[b].cols, jobs[b].path); });
  std::vector<uint32_t> table(4 * n_jobs), waves;
  for (size_t j = 0; j < n_jobs; j++) {
    const ClimbJob& b = jobs[order[j]];
    table[4 * j] = b.offset; table[4 * j + 1] = b.cols; table[4 * j + 2] = b.path; table[4 * j + 3] = b.row;
  }
  for (size_t j = 0; j < n_jobs;) {
    size_t end = j + 1;
    while (end < n_jobs && end - j < 64 && table[4 * end + 1] == table[4 * j + 1] && table[4 * end + 2] == table[4 * j + 2]) end++;
    waves.push_back((uint32_t)j);
    waves.push_back((uint32_t)(end - j));
    j = end;
  }
  (void)hipSetDevice(ctx->device);
  const size_t table_bytes = table.size() * 4, waves_bytes = waves.size() * 4, reached_bytes = n_jobs * 32;
  DevBuf block;  // the job table (16-byte units), the reached digests, the wave table
  R0H_TRY(block.alloc(ctx, table_bytes + reached_bytes + waves_bytes));
  uint32_t* d_table = u32(block.get());
  uint32_t* d_reached = d_table + table.size();
  uint32_t* d_waves = d_reached + 8 * n_jobs;
  R0H_TRY(stage_h2d(ctx, d_table, table.data(), table_bytes));
  R0H_TRY(stage_h2d(ctx, d_waves, waves.data(), waves_bytes));
  const uint32_t n_waves = (uint32_t)(waves.size() / 2);
  R0H_TRY(with_suite(ctx, [&](auto suite) {
    using S = decltype(suite);
    KScope ks(ctx, S::climb_kernel, (double)n_words * 4);
    hipLaunchKernelGGL(merkle_climb_kernel<S>, dim3(n_waves), dim3(64), 0, ctx->stream, d_reached, d_words, (const uint4*)d_table, (const uint2*)d_waves, S::consts(ctx));
    return launch_ok(S::climb_kernel);
  }));
  std::vector<uint32_t> sorted(8 * n_jobs);
  R0H_TRY(r0h_buf_d2h(ctx, block.get(), table_bytes, sorted.data(), reached_bytes));
  for (size_t j = 0; j < n_jobs; j++) memcpy(reached_host + 8 * (size_t)order[j], &sorted[8 * j], 32);
  return nullptr;
}

// The same over openings that lie in host memory: the spans go up back to back through the staging helpers (span s starts at the
// word where span s - 1 ended; the jobs' offsets count from the first), one upload per span and one launch for all.
const char* merkle_climb_spans(r0h_ctx* ctx, const ClimbSpan* spans, size_t n_spans, const ClimbJob* jobs, size_t n_jobs, uint32_t* reached_host, size_t* upload_bytes_out) {
  size_t n_words = 0;
  for (size_t s = 0; s < n_spans; s++) n_words += spans[s].n;
  R0H_REQUIRE(n_words < ((size_t)1 << 32), "merkle_climb: %zu words of openings in one batch", n_words);
  if (upload_bytes_out) *upload_bytes_out = n_jobs ? n_words * 4 + n_jobs * 16 : 0;
  if (!n_jobs) return nullptr;
  (void)hipSetDevice(ctx->device);
  DevBuf words;
  R0H_TRY(words.alloc(ctx, n_words * 4));
  size_t at = 0;
  for (size_t s = 0; s < n_spans; s++) {
    R0H_TRY(stage_h2d(ctx, u32(words.get()) + at, spans[s].w, spans[s].n * 4));
    at += spans[s].n;
  }
  return merkle_climb(ctx, u32(words.get()), n_words, jobs, n_jobs, reached_host);
}

}  // namespace r0h

using namespace r0h;

extern "C" {

const char* r0h_merkle_climb(r0h_ctx* ctx, const r0h_buf* openings, const uint32_t* idx_host, uint32_t n_q, uint32_t rows, uint32_t cols, uint32_t* reached_host) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && openings && ((idx_host && reached_host) || !n_q), "r0h_merkle_climb: NULL argument");
  R0H_TRY(require_pow2_rows("r0h_merkle_climb", rows));
  R0H_REQUIRE(cols >= 1, "r0h_merkle_climb: cols 0: an opening holds at least one value");
  const MerkleShape mp(rows, cols);
  R0H_REQUIRE((size_t)n_q * mp.opening_words() * 4 <= openings->bytes, "r0h_merkle_climb: %u openings of %zu words exceed the buffer", n_q, mp.opening_words());
  R0H_REQUIRE((size_t)n_q * mp.opening_words() < ((size_t)1 << 32), "r0h_merkle_climb: %u openings of %zu words in one call", n_q, mp.opening_words());
  R0H_TRY(require_rows_in_tree("r0h_merkle_climb", idx_host, n_q, rows));
  std::vector<ClimbJob> jobs(n_q);
  for (uint32_t q = 0; q < n_q; q++) jobs[q] = ClimbJob{(uint32_t)(q * mp.opening_words()), cols, (uint32_t)mp.path_digests(), idx_host[q]};
  return merkle_climb(ctx, u32(openings), (size_t)n_q * mp.opening_words(), jobs.data(), n_q, reached_host);
  R0H_GUARD_END
}

}  // extern "C"
