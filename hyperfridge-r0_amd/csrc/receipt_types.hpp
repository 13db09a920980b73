// Receipt / claim types shared by receipt.cpp (JSON reader and writer) and claim.cpp (digests, receipt verification).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/r0hip.h"
#include "circuit.hpp"

struct r0h_receipt {
  int kind = R0H_RECEIPT_FAKE;
  std::vector<uint8_t> journal;
  struct Segment {
    std::vector<uint32_t> seal;
    uint32_t index = 0;
    std::string hashfn;
    bool has_claim = false;
    r0h_receipt_claim claim{};
    uint8_t verifier_parameters[32] = {0};
  };
  std::vector<Segment> segments;
  std::vector<uint32_t> image_seal;  // optional: the image proof of a trace-circuit session (csrc/image.cpp), `inner.Composite.image_proof.seal`
  bool has_metadata = false;  // risc0 >= 1.0 `Receipt.metadata`; the reference's (older) Fake fixtures have none
  uint8_t verifier_parameters[32] = {0};
};

// A node of the lift / join tree (recursion.cpp): its seal, the composed claim it is carried with and -- when every leaf below it is a
// trace-circuit segment -- its leaves' session parts in leaf order, R0H_NODE_SESSION_WORDS each: what r0h_root_verify_session_* reads.
struct r0h_node {
  std::vector<uint32_t> seal;
  r0h_receipt_claim claim;
  std::vector<uint32_t> session;
};

namespace r0h {
// One leaf of a trace-circuit session as its checks read it (claim.cpp session_verdict): the segment seal's early public inputs, the
// root of its DATA commitment, the challenge and the sum the seal carries.  A receipt's segments and a root's session parts both give these.
struct SessionLeaf {
  const uint32_t* early;      // R0H_TRACE_GLOBALS - R0H_TRACE_LATE_GLOBALS words
  const uint32_t* data_root;  // 8
  const uint32_t* challenge;  // 16 (the seal's words at R0H_TRACE_GAMMA)
  const uint32_t* sum;        // 4 (at R0H_TRACE_SUM)
};
// what the balance is held against: the program's image words (the ELF's) or the verified image proof's public inputs, and the journal
struct SessionOtherSide {
  const std::vector<std::pair<uint32_t, uint32_t>>* image;  // or nullptr
  const uint32_t* image_public;                              // or nullptr: R0H_IMAGE_GLOBALS words
  const uint8_t* first_root;                                 // the merkle root in the first claim's pre-state (what an image proof must be about)
  const uint8_t* journal;
  size_t journal_len;
};
// The session section of a trace-circuit receipt's verification, over n leaves of which leaf `term` ends the run: numbers 1..n, the
// closing rules, every leaf's challenge = session_challenge over all records (R0H_RECEIPT_V_SESSION); then, with `other`, the image
// proof's digest and challenge (R0H_RECEIPT_V_IMAGE_PROOF) and the balance of the leaves' sums with the image's and the journal's words
// (R0H_RECEIPT_V_SESSION_SUM; a journal that is no whole number of words: R0H_RECEIPT_V_JOURNAL at `term`).  Without `other` the
// ELF-free checks only.  Returns R0H_RECEIPT_V_OK or the verdict, *leaf_out the leaf it is about.
int session_verdict(const std::vector<SessionLeaf>& leaves, size_t term, const SessionOtherSide* other, size_t* leaf_out);
// the session part of one verified trace-circuit seal (R0H_NODE_SESSION_WORDS words: early public inputs, DATA root, challenge, sum)
void session_part_of(const uint32_t* seal, const uint32_t data_root[8], uint32_t part_out[R0H_NODE_SESSION_WORDS]);
struct Sha256 {
  uint32_t h[8];
  uint64_t total;
  uint8_t buf[64];
  size_t fill;
  Sha256() { reset(); }
  void reset();
  void update(const void* data, size_t n);
  void finish(uint8_t out[32]);

 private:
  void block(const uint8_t* p);
};
void sha256(const void* data, size_t n, uint8_t out[32]);
// one compression (FIPS 180-4 6.2.2): state and the sixteen message words in the hash's own word order; the initial state
void sha256_compress(uint32_t state[8], const uint32_t w[16]);
extern const uint32_t SHA_IV[8];
void tagged_struct(const char* tag, const uint8_t (*down)[32], size_t n_down, const uint32_t* data, size_t n_data, uint8_t out[32]);
void system_state_digest(const r0h_system_state& st, uint8_t out[32]);
void claim_digest(const r0h_receipt_claim& c, uint8_t out[32]);
void claim_globals(const uint8_t digest[32], uint32_t out[8]);
bool is_trace_circuit(const r0h_circuit& circ);
bool is_image_circuit(const r0h_circuit& circ);  // image.cpp
bool trace_seal_carries_claim(const uint32_t* seal, const r0h_receipt_claim& claim);
void session_challenge(const uint32_t* records, size_t n_records, uint32_t out[16]);
void image_stream(const std::vector<std::pair<uint32_t, uint32_t>>& image, std::vector<uint32_t>& words_out);  // rv32im.cpp: the image circuit's sponge blocks (Montgomery)
void image_digest(const std::vector<std::pair<uint32_t, uint32_t>>& image, uint32_t digest_out[8]);             // ... and their digest: the root of the initial memory state
const char* elf_image(const uint8_t* elf, size_t n, std::vector<std::pair<uint32_t, uint32_t>>& image, uint32_t* entry, uint8_t image_id[32]);  // rv32im.cpp
}  // namespace r0h
