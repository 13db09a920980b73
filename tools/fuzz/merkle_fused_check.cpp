// The plan of r0h_hash_fold_top (csrc/merkle_fused_plan.hpp) walked on the host: which workgroup of which launch folds which nodes.
// For every rows = 2^k, k = 0 .. 26, under both hash suites, the launches merkle_fused_plan returns are carried out over a host array
// with the host suite's hash_pair, workgroup by workgroup, in the order merkle_subtree_kernel folds (merkle.hip), and three things
// are asserted:
//   * every node in [1, min(rows, 2^14)) is produced exactly once, and nothing else is written;
//   * every read is of a node of the base level, or of one produced earlier by the same workgroup or by an earlier launch -- never of
//     one another workgroup of the same launch writes;
//   * the nodes equal the plain level-by-level fold.
// The base level is the leaves for rows <= 2^14 and, for a larger tree, the level of 16384 nodes r0h_hash_fold leaves (seeded words
// stand for it: the plan depends on nothing below).  The compiled-in split is walked with the hashes; every other split the header
// admits is walked for the first two properties alone.
// Built with -fsanitize=address,undefined by tools/fuzz/run_merkle_fused_check.sh; needs no GPU.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "internal.hpp"
#include "merkle_fused_plan.hpp"

using namespace r0h;

#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      fprintf(stderr, "merkle_fused_check: ");    \
      fprintf(stderr, __VA_ARGS__);               \
      fprintf(stderr, "\n");                      \
      abort();                                    \
    }                                             \
  } while (0)

struct Producer {
  int launch = -1;  // -1: not produced
  uint32_t group = 0;
};

// suite == nullptr: the structure alone
static long walk(const HashSuite* suite, const char* name, uint32_t k, uint32_t split) {
  const uint32_t rows = 1u << k;
  MerkleFusedLaunch plan[2];
  uint32_t top = 0;
  const int launches = merkle_fused_plan(rows, split, plan, &top);
  CHECK(top == (rows / 2 < 8192u ? rows / 2 : 8192u), "%s rows 2^%u: the fused part starts at %u parents", name, k, top);
  CHECK(launches >= 0 && launches <= 2 && (launches == 0) == (top == 0), "%s rows 2^%u: %d launches", name, k, launches);
  const size_t total = top ? (size_t)4 * top : 2;  // digests: nodes [0, 2 top) to produce (0 is no node), base level [2 top, 4 top)
  std::vector<uint32_t> nodes(total * 8, 0xA5A5A5A5u), want;
  std::mt19937 rng(1000 * k + split);
  for (size_t w = (size_t)2 * top * 8; w < total * 8; w++) nodes[w] = (uint32_t)(rng() % P);
  if (suite) {
    want = nodes;
    for (uint32_t sz = top; sz >= 1; sz /= 2)
      for (uint32_t i = sz; i < 2 * sz; i++) suite->hash_pair(&want[(size_t)2 * i * 8], &want[(size_t)(2 * i + 1) * 8], &want[(size_t)i * 8]);
  }
  std::vector<Producer> made(total);
  long hashes = 0;
  for (int i = 0; i < launches; i++) {
    const uint32_t G = plan[i].G, d = plan[i].d;
    CHECK(G >= 1 && (G & (G - 1)) == 0 && d >= 1 && d <= MERKLE_FUSED_MAX_D, "%s rows 2^%u: launch %d is (%u, %u)", name, k, i, G, d);
    for (uint32_t b = 0; b < G; b++) {
      const uint32_t r = G + b;
      for (uint32_t j = d; j-- > 0;) {
        for (uint32_t p = 0; p < (1u << j); p++) {
          const size_t node = ((size_t)r << j) + p;
          CHECK(node >= 1 && 2 * node + 1 < total, "%s rows 2^%u: launch %d workgroup %u folds node %zu of a buffer of %zu", name, k, i, b, node, total);
          for (size_t child = 2 * node; child <= 2 * node + 1; child++) {
            if (child >= (size_t)2 * top) continue;  // the base level
            const Producer& c = made[child];
            CHECK(c.launch >= 0, "%s rows 2^%u: launch %d workgroup %u reads node %zu before anything produced it", name, k, i, b, child);
            CHECK(c.launch < i || c.group == b, "%s rows 2^%u: launch %d workgroup %u reads node %zu, which workgroup %u of the same launch writes", name, k, i, b, child, c.group);
          }
          CHECK(node < (size_t)2 * top, "%s rows 2^%u: launch %d workgroup %u writes node %zu of the base level", name, k, i, b, node);
          CHECK(made[node].launch < 0, "%s rows 2^%u: node %zu is produced twice", name, k, node);
          made[node].launch = i;
          made[node].group = b;
          if (suite) suite->hash_pair(&nodes[2 * node * 8], &nodes[(2 * node + 1) * 8], &nodes[node * 8]);
          hashes++;
        }
      }
    }
  }
  for (size_t node = 1; node < (size_t)2 * top; node++) CHECK(made[node].launch >= 0, "%s rows 2^%u: node %zu is never produced", name, k, node);
  CHECK(made[0].launch < 0, "%s rows 2^%u: node 0 is written", name, k);
  if (suite) CHECK(nodes == want, "%s rows 2^%u: the nodes differ from the level-by-level fold", name, k);
  return hashes;
}

int main() {
  long hashes = 0, walks = 0;
  for (int fn : {(int)HASH_POSEIDON2, (int)HASH_SHA256}) {
    const std::unique_ptr<HashSuite> suite = make_suite(fn, &p2_default());
    const char* name = fn == HASH_SHA256 ? "sha-256" : "poseidon2";
    for (uint32_t k = 0; k <= 26; k++) {
      hashes += walk(suite.get(), name, k, MERKLE_FUSED_SPLIT);
      walks++;
    }
  }
  for (uint32_t split = 4; split <= MERKLE_FUSED_MAX_D; split++)
    for (uint32_t k = 0; k <= 26; k++) {
      walk(nullptr, "structure", k, split);
      walks++;
    }
  printf("merkle fused check: no report (%ld walks, %ld pair hashes, split %u)\n", walks, hashes, MERKLE_FUSED_SPLIT);
  return 0;
}
