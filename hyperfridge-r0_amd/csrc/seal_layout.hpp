// What the sequencer (prover.hip) and the verifier (verify.cpp) must agree on about a seal before either reads a word of it: how the
// transcript opens, which Merkle layer a commitment writes out (and with it the size of an opening), and the FRI rounds of a trace
// size.  Host only.  Everything else -- the DEEP weights, the tap points, the queries -- is formulated per side: batched device jobs
// there, per-query host work here.
#pragma once
#include "circuit.hpp"

namespace r0h {

inline unsigned log2u(size_t x) { unsigned n = 0; while (((size_t)1 << n) < x) n++; return n; }

// A committed matrix of `rows` x `cols` words.  The seal carries layer `top_layer` of its tree (the deepest one of at most R0H_QUERIES
// nodes) instead of the root; an opening is the row followed by the sibling digests from the leaf up to, excluding, that layer.
struct MerkleShape {
  size_t rows, cols, layers, top_layer, top_size;
  MerkleShape(size_t r, size_t c) : rows(r), cols(c), layers(log2u(r)), top_layer(0) {
    for (size_t i = 1; i < layers; i++) {
      if (((size_t)1 << i) > R0H_QUERIES) break;
      top_layer = i;
    }
    top_size = (size_t)1 << top_layer;
  }
  size_t path_digests() const { return layers - top_layer; }
  size_t opening_words() const { return cols + 8 * path_digests(); }
};

// risc0-circuit-rv32im prove/hal: the hashes of two 16-byte ProtocolInfo tags (one field element per byte) open the transcript -- the
// proof system's and the circuit's -- then the early public inputs and po2 (the late ones, R0H_SEC_LATE, follow the DATA commitment).
// `Io` is WriteIop or SealReader; `global` holds canonical words (the caller has checked them).
template <class Io>
void transcript_open(Io& io, const r0h_circuit& c, const uint32_t* global, uint32_t po2) {
  static const char proof_system_info[] = "RISC0_STARK:v1__";
  uint32_t e[16];
  for (int i = 0; i < 16; i++) e[i] = enc((uint8_t)proof_system_info[i]);
  io.commit_elems(e, 16);
  for (int i = 0; i < 16; i++) e[i] = enc(c.info[i]);
  io.commit_elems(e, 16);
  std::vector<uint32_t> early(global, global + (c.n_global - c.n_late));
  early.push_back(enc(po2));
  io.commit_elems(early.data(), early.size());
}

// The FRI rounds of a trace of n rows: a round commits a polynomial of `degree` coefficients, evaluated on `domain` points, as a tree
// of `rows` rows (R0H_FRI_FOLD extension values each) and folds it by R0H_FRI_FOLD; what is left goes into the seal as it is.
struct FriRound { size_t degree, domain, rows; };
struct FriSchedule {
  std::vector<FriRound> rounds;
  size_t final_degree;
  explicit FriSchedule(size_t n) {
    size_t deg = n;
    for (; deg > R0H_FRI_MIN_DEGREE; deg /= R0H_FRI_FOLD) rounds.push_back(FriRound{deg, deg * R0H_INV_RATE, deg * R0H_INV_RATE / R0H_FRI_FOLD});
    final_degree = deg;
  }
};

}  // namespace r0h
