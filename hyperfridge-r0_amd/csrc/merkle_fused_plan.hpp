// Which workgroup folds which nodes when the top of a Merkle tree is built by merkle_subtree_kernel (merkle.hip,
// r0h_hash_fold_top): the plan, kept apart from the kernel so that it compiles for the host alone and is walked there
// (tools/fuzz/merkle_fused_check.cpp).
//
// A launch (G, d) has G workgroups.  Workgroup b owns node r = G + b of the level that has G nodes, reads the 2^d nodes
// (r << d) .. (r << d) + 2^d - 1 that lie d levels below r, and writes every node of the d levels from there up to r: node
// (r << j) + p for j = d - 1 .. 0, p < 2^j.  A workgroup reads nothing another workgroup of its launch writes, so levels cross
// workgroups only from one launch to the next, in stream order.
#pragma once
#include <stdint.h>

namespace r0h {

constexpr uint32_t MERKLE_FUSED_MAX_PARENTS = 8192;  // the widest level r0h_hash_fold_top produces (r0h_hash_fold's lanes form ends there too)
// The split a: a top of more than a levels is cut at the level of 2^a nodes.  Chosen by measurement (profiles/r24/merkle_fused_tops.md);
// a build with another value is what tools/ab/ab_merkle_fused.py compares it against.
#ifndef R0H_MERKLE_FUSED_SPLIT
#define R0H_MERKLE_FUSED_SPLIT 7
#endif
constexpr uint32_t MERKLE_FUSED_SPLIT = R0H_MERKLE_FUSED_SPLIT;
constexpr uint32_t MERKLE_FUSED_MAX_D = 10;  // a workgroup's subtree lives in 2^d * 32 bytes of LDS: 32 KiB at most
static_assert(MERKLE_FUSED_SPLIT >= 4 && MERKLE_FUSED_SPLIT <= MERKLE_FUSED_MAX_D, "either launch of a 14-level top folds at most MERKLE_FUSED_MAX_D levels");

struct MerkleFusedLaunch {
  uint32_t G, d;
};

// The launches that fill the levels output_size, output_size / 2, .., 1 from the level of 2 * output_size nodes (output_size a power
// of two, at most MERKLE_FUSED_MAX_PARENTS; 0: none).  At most two: one workgroup when the top has no more than `split` levels, else
// 2^split workgroups down to the level of 2^split nodes and one workgroup from there.  Returns how many it wrote to `out`.
inline int merkle_fused_plan_top(uint32_t output_size, uint32_t split, MerkleFusedLaunch out[2]) {
  if (output_size == 0) return 0;
  uint32_t levels = 1;  // log2(2 * output_size): the levels to produce
  while ((1u << levels) < 2 * output_size) levels++;
  if (levels <= split) {
    out[0] = MerkleFusedLaunch{1u, levels};
    return 1;
  }
  out[0] = MerkleFusedLaunch{1u << split, levels - split};
  out[1] = MerkleFusedLaunch{1u, split};
  return 2;
}

// The fused part of a tree of `rows` leaves (a power of two): *output_size is the widest level it produces -- rows / 2, or
// MERKLE_FUSED_MAX_PARENTS for a larger tree, whose wider levels are r0h_hash_fold's -- and the launches are those of
// merkle_fused_plan_top for it.  A tree of one row has no parents: no launch, *output_size = 0.
inline int merkle_fused_plan(uint32_t rows, uint32_t split, MerkleFusedLaunch out[2], uint32_t* output_size) {
  *output_size = rows / 2 < MERKLE_FUSED_MAX_PARENTS ? rows / 2 : MERKLE_FUSED_MAX_PARENTS;
  return merkle_fused_plan_top(*output_size, split, out);
}

}  // namespace r0h
