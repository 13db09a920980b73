// Receipt claims (host-only, no device work) -- SURVEY.md 8(a) a18, the types `host` serialises and `verifier` checks:
//   risc0-zkvm 3.0.5 receipt/{mod.rs, composite.rs, segment.rs}, receipt_claim.rs; risc0-binfmt 3.0.4 {hash.rs `tagged_struct`,
//   sys_state.rs `SystemState`, exit_code.rs `ExitCode`} (Cargo.lock:3226-3228, 2954-2956), reached from
//   verifier/src/main.rs:118-126 (`serde_json::from_slice::<Receipt>` then `receipt.verify(image_id)`) and host/src/main.rs:251-267.
// Everything below the SHA-256 itself is RECALLED from the public risc0 sources -- the reference holds only `"inner":"Fake"`
// receipts, so field names, tags and the digest layout are "parity unpinned" until a real risc0 3.0.5 receipt is available:
//   tagged_struct(tag, down[], data[]) = SHA-256( SHA-256(tag) || down[0] || .. || data[i] as u32 LE .. || (down.len() as u16 LE) )
//   SystemState.digest   = tagged_struct("risc0.SystemState", [merkle_root], [pc])
//   Output.digest        = tagged_struct("risc0.Output", [SHA-256(journal), assumptions.digest], [])
//   ReceiptClaim.digest  = tagged_struct("risc0.ReceiptClaim", [input, pre.digest, post.digest, output], [exit.system, exit.user])
//   ExitCode -> (system, user): Halted(u) = (0, u), Paused(u) = (1, u), SystemSplit = (2, 0), SessionLimit = (2, 2)
// What is pinned: SHA-256 against the FIPS 180-4 example vectors (tests/test_claims.py), and, through the journal, the
// reference's receipt fixtures.
//
// How a claim is tied to a seal here: risc0's rv32im circuit exposes the claim's digests in its public outputs (globals) and
// `SegmentReceipt::verify_integrity` decodes and compares them.  This repository's circuits are synthetic, so the binding is
// made through their first eight globals: globals[0..8) = Poseidon2 sponge over the sixteen 16-bit halves of the claim digest
// (r0h_claim_globals).  The transcript commits to the globals, so a seal proves "a trace of this program exists whose public
// inputs name this claim"; r0h_receipt_verify recomputes the claim digest from the receipt's fields and compares.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/r0hip.h"
#include "internal.hpp"
#include "receipt_types.hpp"

namespace r0h {

// ---------------------------------------------------------------- SHA-256 (FIPS 180-4)
namespace {
const uint32_t SHA_K[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
    0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
    0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
    0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
    0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
    0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
inline uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
}  // namespace

const uint32_t SHA_IV[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
void sha256_compress(uint32_t st[8], const uint32_t m[16]) {
  uint32_t w[64];
  memcpy(w, m, 64);
  for (int i = 16; i < 64; i++) {
    const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3), s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
    w[i] = w[i - 16] + s0 + w[i - 7] + s1;
  }
  uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
  for (int i = 0; i < 64; i++) {
    const uint32_t t1 = h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + SHA_K[i] + w[i];
    const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
    h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
  }
  st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

void Sha256::reset() {
  memcpy(h, SHA_IV, sizeof h);
  total = 0;
  fill = 0;
}
void Sha256::block(const uint8_t* p) {
  uint32_t w[16];
  for (int i = 0; i < 16; i++) w[i] = ((uint32_t)p[4 * i] << 24) | ((uint32_t)p[4 * i + 1] << 16) | ((uint32_t)p[4 * i + 2] << 8) | p[4 * i + 3];
  sha256_compress(h, w);
}
void Sha256::update(const void* data, size_t n) {
  const uint8_t* p = (const uint8_t*)data;
  total += n;
  if (fill) {
    size_t take = 64 - fill < n ? 64 - fill : n;
    memcpy(buf + fill, p, take);
    fill += take; p += take; n -= take;
    if (fill < 64) return;
    block(buf);
    fill = 0;
  }
  for (; n >= 64; p += 64, n -= 64) block(p);
  if (n) { memcpy(buf, p, n); fill = n; }
}
void Sha256::finish(uint8_t out[32]) {
  const uint64_t bits = total * 8;
  uint8_t pad[72] = {0x80};
  const size_t padlen = (fill < 56 ? 56 : 120) - fill;
  for (int i = 0; i < 8; i++) pad[padlen + i] = (uint8_t)(bits >> (56 - 8 * i));
  update(pad, padlen + 8);
  for (int i = 0; i < 8; i++) { out[4 * i] = (uint8_t)(h[i] >> 24); out[4 * i + 1] = (uint8_t)(h[i] >> 16); out[4 * i + 2] = (uint8_t)(h[i] >> 8); out[4 * i + 3] = (uint8_t)h[i]; }
}
void sha256(const void* data, size_t n, uint8_t out[32]) {
  Sha256 s;
  s.update(data, n);
  s.finish(out);
}

// risc0-binfmt hash.rs `tagged_struct::<sha::Impl>(tag, down, data)`
void tagged_struct(const char* tag, const uint8_t (*down)[32], size_t n_down, const uint32_t* data, size_t n_data, uint8_t out[32]) {
  uint8_t tag_digest[32];
  sha256(tag, strlen(tag), tag_digest);
  Sha256 s;
  s.update(tag_digest, 32);
  for (size_t i = 0; i < n_down; i++) s.update(down[i], 32);
  for (size_t i = 0; i < n_data; i++) {
    const uint8_t le[4] = {(uint8_t)data[i], (uint8_t)(data[i] >> 8), (uint8_t)(data[i] >> 16), (uint8_t)(data[i] >> 24)};
    s.update(le, 4);
  }
  const uint8_t len[2] = {(uint8_t)n_down, (uint8_t)(n_down >> 8)};
  s.update(len, 2);
  s.finish(out);
}

void system_state_digest(const r0h_system_state& st, uint8_t out[32]) {
  uint8_t down[1][32];
  memcpy(down[0], st.merkle_root, 32);
  tagged_struct("risc0.SystemState", down, 1, &st.pc, 1, out);
}

void claim_digest(const r0h_receipt_claim& c, uint8_t out[32]) {
  uint8_t down[4][32];
  memcpy(down[0], c.input_digest, 32);
  system_state_digest(c.pre, down[1]);
  system_state_digest(c.post, down[2]);
  memcpy(down[3], c.output_digest, 32);
  const uint32_t data[2] = {c.exit_system, c.exit_user};
  tagged_struct("risc0.ReceiptClaim", down, 4, data, 2, out);
}

void claim_globals(const uint8_t digest[32], uint32_t out[8]) {
  uint32_t halves[16];
  for (int i = 0; i < 16; i++) halves[i] = enc((uint32_t)digest[2 * i] | ((uint32_t)digest[2 * i + 1] << 8));
  p2_hash_elems_host(p2_default(), halves, 16, out);
}

// what a trace-circuit seal says in its public inputs beyond the claim's name, held against the claim it is carried with: the pc the
// run starts from and stops at, whether it ends in HALT / PAUSE, and with which exit code (r0h_receipt_verify, r0h_lift)
bool is_trace_circuit(const r0h_circuit& circ) {
  return !memcmp(circ.info, "R0HIP_TRACE:v5__", 16) && circ.n_global == R0H_TRACE_GLOBALS && circ.n_late == R0H_TRACE_LATE_GLOBALS;
}
bool trace_seal_carries_claim(const uint32_t* seal, const r0h_receipt_claim& claim) {
  if (seal[8] != enc(claim.pre.pc) || seal[9] != enc(claim.post.pc)) return false;
  const uint32_t kind = claim.exit_system == 0 ? 1u : claim.exit_system == 1 ? 2u : 0u, code = kind ? claim.exit_user : 0u;
  return seal[11] == enc(kind) && seal[12] == enc(kind ? 1u : 0u) && seal[13] == enc(code & 0xffffu) && seal[14] == enc(code >> 16);
}

// The challenge all segments of a trace-circuit session share (late public inputs 20..35 of every seal): alpha_g and gamma, gamma^2,
// gamma^3, drawn from the Poseidon2 digest of a tag and every segment's record -- its early public inputs and the root of its DATA
// commitment -- in index order.  Every tuple of the session sum is committed before the challenge exists.
void session_challenge(const uint32_t* records, size_t n_records, uint32_t out[16]) {
  static const char tag[] = "R0HIP_SESSION:v1";
  std::vector<uint32_t> elems;
  elems.reserve(16 + n_records * R0H_SESSION_RECORD_WORDS);
  for (int i = 0; i < 16; i++) elems.push_back(enc((uint8_t)tag[i]));
  elems.insert(elems.end(), records, records + n_records * R0H_SESSION_RECORD_WORDS);
  uint32_t cells[P2_CELLS] = {0};
  p2_hash_elems_host(p2_default(), elems.data(), elems.size(), cells);
  p2_mix_host(p2_default(), cells);
  Fp4 alpha{{cells[0], cells[1], cells[2], cells[3]}}, g{{cells[4], cells[5], cells[6], cells[7]}};
  const Fp4 g2 = g * g, g3 = g2 * g;
  memcpy(out, alpha.e, 16);
  memcpy(out + 4, g.e, 16);
  memcpy(out + 8, g2.e, 16);
  memcpy(out + 12, g3.e, 16);
}


void session_part_of(const uint32_t* seal, const uint32_t data_root[8], uint32_t part_out[R0H_NODE_SESSION_WORDS]) {
  constexpr size_t early = R0H_TRACE_GLOBALS - R0H_TRACE_LATE_GLOBALS;
  static_assert(early + 8 == R0H_SESSION_RECORD_WORDS && R0H_SESSION_RECORD_WORDS + 16 + 4 == R0H_NODE_SESSION_WORDS, "session part layout");
  memcpy(part_out, seal, early * 4);
  memcpy(part_out + early, data_root, 32);
  memcpy(part_out + R0H_SESSION_RECORD_WORDS, seal + R0H_TRACE_GAMMA, 64);
  memcpy(part_out + R0H_SESSION_RECORD_WORDS + 16, seal + R0H_TRACE_SUM, 16);
}

int session_verdict(const std::vector<SessionLeaf>& leaves, size_t term, const SessionOtherSide* other, size_t* leaf_out) {
  constexpr size_t early = R0H_TRACE_GLOBALS - R0H_TRACE_LATE_GLOBALS;
  const size_t n = leaves.size();
  auto done = [&](int v, size_t leaf) { *leaf_out = leaf; return v; };
  // ---- the session: numbers, closing segments, the common challenge
  std::vector<uint32_t> records(n * R0H_SESSION_RECORD_WORDS);
  for (size_t i = 0; i < n; i++) {
    memcpy(&records[i * R0H_SESSION_RECORD_WORDS], leaves[i].early, early * 4);
    memcpy(&records[i * R0H_SESSION_RECORD_WORDS + early], leaves[i].data_root, 32);
  }
  uint32_t challenge[16];
  session_challenge(records.data(), n, challenge);
  bool closing_seen = false;
  uint32_t closed_up_to = 0;
  for (size_t i = 0; i < n; i++) {
    const uint32_t* sl = leaves[i].early;
    const uint32_t fin = sl[16];
    if (sl[15] != enc((uint32_t)i + 1) || (fin != 0 && fin != ONE) || sl[17] != (fin ? 0u : sl[15])) return done(R0H_RECEIPT_V_SESSION, i);
    if (memcmp(leaves[i].challenge, challenge, 64) != 0) return done(R0H_RECEIPT_V_SESSION, i);
    // closing segments: the one that ends the run when it is the last, else every segment after it; their rows go up through the addresses
    const bool must_close = term == n - 1 ? i == term : i > term;
    if ((fin != 0) != must_close) return done(R0H_RECEIPT_V_SESSION, i);
    if (fin) {
      const uint32_t lo = dec(sl[18]), hi = dec(sl[19]);
      if (closing_seen && lo <= closed_up_to) return done(R0H_RECEIPT_V_SESSION, i);
      if (hi < lo) return done(R0H_RECEIPT_V_SESSION, i);
      closing_seen = true;
      closed_up_to = hi;
    }
  }
  if (!other) return done(R0H_RECEIPT_V_OK, 0);
  const uint32_t* image_public = other->image_public;
  const std::vector<std::pair<uint32_t, uint32_t>>* image = other->image;
  if (image_public) {  // the image's side comes from the image proof: it must be about THIS image (the digest in the first claim's pre-state,
    // which is held against the image id by the caller) and under THIS session's challenge
    const uint8_t* root = other->first_root;
    for (int i = 0; i < 8; i++) {
      const uint32_t w = (uint32_t)root[4 * i] | (uint32_t)root[4 * i + 1] << 8 | (uint32_t)root[4 * i + 2] << 16 | (uint32_t)root[4 * i + 3] << 24;
      if (w >= P || image_public[i] != enc(w)) return done(R0H_RECEIPT_V_IMAGE_PROOF, 0);
    }
    if (memcmp(&image_public[R0H_IMAGE_GAMMA], challenge, 64) != 0) return done(R0H_RECEIPT_V_IMAGE_PROOF, 0);
  }
  // ---- the balance: sum of the segments' sums = sum over the image's words + sum over the journal's words of 1 / fingerprint
  const Fp4 ag{{challenge[0], challenge[1], challenge[2], challenge[3]}}, g1{{challenge[4], challenge[5], challenge[6], challenge[7]}},
      g2{{challenge[8], challenge[9], challenge[10], challenge[11]}}, g3{{challenge[12], challenge[13], challenge[14], challenge[15]}};
  Fp4 total = fp4_zero();
  for (size_t i = 0; i < n; i++) {
    const uint32_t* q = leaves[i].sum;
    total = total + Fp4{{q[0], q[1], q[2], q[3]}};
  }
  // batched inversion: the fingerprints are multiplied up, one inversion, and walked back
  std::vector<Fp4> fps;
  fps.reserve((image ? image->size() : 0) + other->journal_len / 4);
  auto fingerprint = [&](uint32_t addr, uint32_t word, uint32_t tag) {
    Fp4 f = ag - scale(g1, enc(word & 0xffffu)) - scale(g2, enc(word >> 16)) - scale(g3, enc(tag));
    f.e[0] = sub(f.e[0], enc(addr));
    fps.push_back(f);
  };
  if (image)
    for (const auto& w : *image) fingerprint(w.first, w.second, R0H_SESSION_TAG_IMAGE);
  if (other->journal_len % 4) return done(R0H_RECEIPT_V_JOURNAL, term);  // COMMIT moves words
  for (size_t j = 0; j < other->journal_len / 4; j++) {
    const uint8_t* b = &other->journal[4 * j];
    fingerprint(R0H_JOURNAL_BASE / 4 + (uint32_t)j, (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24, R0H_SESSION_TAG_JOURNAL);
  }
  std::vector<Fp4> prefix(fps.size() + 1, fp4_one());
  for (size_t k = 0; k < fps.size(); k++) prefix[k + 1] = prefix[k] * fps[k];
  Fp4 inv_run = fp4_inv(prefix[fps.size()]), rest = fp4_zero();
  for (size_t k = fps.size(); k-- > 0;) {
    rest = rest + inv_run * prefix[k];
    inv_run = inv_run * fps[k];
  }
  if (!image) rest = rest + Fp4{{image_public[R0H_IMAGE_SUM], image_public[R0H_IMAGE_SUM + 1], image_public[R0H_IMAGE_SUM + 2], image_public[R0H_IMAGE_SUM + 3]}};
  if (!(total == rest)) return done(R0H_RECEIPT_V_SESSION_SUM, 0);
  return done(R0H_RECEIPT_V_OK, 0);
}

}  // namespace r0h

using namespace r0h;

extern "C" {

const char* r0h_sha256(const uint8_t* bytes, size_t n, uint8_t digest_out[32]) {
  R0H_REQUIRE((bytes || n == 0) && digest_out, "r0h_sha256: NULL argument");
  sha256(bytes, n, digest_out);
  return nullptr;
}

const char* r0h_tagged_struct(const char* tag, const uint8_t* down_digests, size_t n_down, const uint32_t* data, size_t n_data, uint8_t digest_out[32]) {
  R0H_REQUIRE(tag && (down_digests || !n_down) && (data || !n_data) && digest_out, "r0h_tagged_struct: NULL argument");
  R0H_REQUIRE(n_down <= 0xffff, "r0h_tagged_struct: the count of digests is a u16");
  tagged_struct(tag, (const uint8_t(*)[32])down_digests, n_down, data, n_data, digest_out);
  return nullptr;
}

const char* r0h_system_state_digest(const r0h_system_state* st, uint8_t digest_out[32]) {
  R0H_REQUIRE(st && digest_out, "r0h_system_state_digest: NULL argument");
  system_state_digest(*st, digest_out);
  return nullptr;
}

const char* r0h_output_digest(const uint8_t* journal, size_t n, const uint8_t* assumptions_digest, uint8_t digest_out[32]) {
  R0H_REQUIRE((journal || n == 0) && digest_out, "r0h_output_digest: NULL argument");
  uint8_t down[2][32];
  sha256(journal, n, down[0]);
  if (assumptions_digest) memcpy(down[1], assumptions_digest, 32);
  else memset(down[1], 0, 32);  // an empty assumption list hashes to Digest::ZERO
  tagged_struct("risc0.Output", down, 2, nullptr, 0, digest_out);
  return nullptr;
}

const char* r0h_claim_digest(const r0h_receipt_claim* claim, uint8_t digest_out[32]) {
  R0H_REQUIRE(claim && digest_out, "r0h_claim_digest: NULL argument");
  R0H_REQUIRE(claim->exit_system <= 2, "r0h_claim_digest: exit code system part %u is not one of Halted(0) / Paused(1) / Split,Limit(2)", claim->exit_system);
  claim_digest(*claim, digest_out);
  return nullptr;
}

const char* r0h_session_challenge(const uint32_t* records, size_t n_records, uint32_t challenge_out[16]) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(records && n_records && challenge_out, "r0h_session_challenge: NULL argument");
  for (size_t i = 0; i < n_records * R0H_SESSION_RECORD_WORDS; i++) R0H_REQUIRE(records[i] < P, "r0h_session_challenge: word %zu is not a canonical field word", i);
  session_challenge(records, n_records, challenge_out);
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_claim_globals(const uint8_t claim_digest[32], uint32_t globals_out[8]) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(claim_digest && globals_out, "r0h_claim_globals: NULL argument");
  claim_globals(claim_digest, globals_out);
  return nullptr;
  R0H_GUARD_END
}

// The image id as the reference writes and reads it (host/src/main.rs:445-449 `{:08x}` per u32 word of HYPERFRIDGE_ID,
// verifier/src/main.rs:131-143 `u32::from_str_radix` per 8 digits, fixture host/out/IMAGE_ID.hex): eight big-endian-printed words,
// each of which risc0's `Digest::from([u32; 8])` stores little-endian -- so digest byte 4i + k is digits [8i + 6 - 2k, 8i + 8 - 2k).
const char* r0h_image_id_from_hex(const char* hex, uint8_t image_id_out[32]) {
  R0H_REQUIRE(hex && image_id_out, "r0h_image_id_from_hex: NULL argument");
  R0H_REQUIRE(strlen(hex) == 64, "image id: exactly 64 hex digits wanted (verifier/src/main.rs:131-134)");
  for (int i = 0; i < 8; i++) {
    uint32_t w = 0;
    for (int d = 0; d < 8; d++) {
      const char ch = hex[8 * i + d];
      const int v = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : ch >= 'A' && ch <= 'F' ? ch - 'A' + 10 : -1;
      R0H_REQUIRE(v >= 0, "image id: '%c' is not a hex digit", ch);
      w = w << 4 | (uint32_t)v;
    }
    for (int k = 0; k < 4; k++) image_id_out[4 * i + k] = (uint8_t)(w >> (8 * k));
  }
  return nullptr;
}
const char* r0h_image_id_to_hex(const uint8_t image_id[32], char hex_out[65]) {
  R0H_REQUIRE(image_id && hex_out, "r0h_image_id_to_hex: NULL argument");
  for (int i = 0; i < 8; i++) {
    const uint32_t w = (uint32_t)image_id[4 * i] | (uint32_t)image_id[4 * i + 1] << 8 | (uint32_t)image_id[4 * i + 2] << 16 | (uint32_t)image_id[4 * i + 3] << 24;
    snprintf(hex_out + 8 * i, 9, "%08x", w);
  }
  return nullptr;
}

const char* r0h_receipt_verify_reason(int verdict) {
  static const char* const names[] = {"ok", "not a composite receipt (Fake receipts prove nothing)", "a segment seal was rejected",
                                      "no control root known for a segment's trace size", "a segment carries no claim",
                                      "a seal's public inputs do not name its claim", "segments do not chain (index / post-state / exit code)",
                                      "the journal is not the one the last segment's claim commits to", "the first pre-state is not the expected image id",
                                      "the final exit code is not Halted(0) or Paused(0)", "the circuit exposes fewer than 8 globals: claims cannot be bound",
                                      "a segment names a hash function other than poseidon2",
                                      "seals, claims and chain are valid but no image id was given: nothing ties the receipt to a program",
                                      "a seal's session number, closing flag or challenge is not this session's",
                                      "the segments' session sums do not balance with the program image and the journal",
                                      "seals, claims, chain and image id are valid, but the program image (the ELF) was not given: the session sum is unchecked",
                                      "the receipt's image proof is missing, was rejected, or is not about this image or this session"};
  return verdict >= 0 && verdict <= R0H_RECEIPT_V_IMAGE_PROOF ? names[verdict] : "unknown";
}

// What stands between the walk of a receipt and the verification of segment g's seal: R0H_RECEIPT_V_OK with the control root the seal
// is verified against, or the verdict the walk ends with at this segment (one definition for the walk and for the batch the _on forms
// verify ahead of it).  The seal names its trace size in its public part (globals, then po2): that size's control root is picked.
static int segment_seal_root(const r0h_circuit& circ, const r0h_receipt::Segment& g, const uint32_t* control_roots, size_t n_roots, const uint32_t** root_out) {
  *root_out = nullptr;
  if (g.hashfn != "poseidon2") return R0H_RECEIPT_V_HASHFN;  // the only suite this prover and this verifier implement
  if (g.seal.size() < (size_t)circ.n_global + 1 || g.seal[circ.n_global] >= P) return R0H_RECEIPT_V_SEAL;
  const uint32_t po2 = dec(g.seal[circ.n_global]);
  for (size_t k = 0; k < n_roots; k++)
    if (control_roots[9 * k] == po2) *root_out = control_roots + 9 * k + 1;
  return *root_out ? R0H_RECEIPT_V_OK : R0H_RECEIPT_V_NO_CONTROL_ROOT;
}

// risc0-zkvm receipt/composite.rs `verify_integrity_with_context` + receipt/mod.rs `Receipt::verify(image_id)`
static const char* receipt_verify_impl(const r0h_receipt* rc, const uint32_t* blob, size_t blob_words, const uint32_t* control_roots, size_t n_roots,
                                       const uint8_t* image_id, const std::vector<std::pair<uint32_t, uint32_t>>* image, int* verdict_out, size_t* segment_out,
                                       int* seal_verdict_out, const uint32_t* image_public = nullptr /* the verified image proof's 28 public inputs */,
                                       std::vector<SealCheck>* verified = nullptr /* the _on forms: segment i's seal as receipt_seal_batch verified it */) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(rc && blob && verdict_out && (control_roots || !n_roots), "r0h_receipt_verify: NULL argument");
  if (segment_out) *segment_out = 0;
  if (seal_verdict_out) *seal_verdict_out = R0H_VERIFY_OK;
  auto done = [&](int v, size_t seg) { *verdict_out = v; if (segment_out) *segment_out = seg; return (const char*)nullptr; };
  if (rc->kind != R0H_RECEIPT_COMPOSITE || rc->segments.empty()) return done(R0H_RECEIPT_V_NOT_COMPOSITE, 0);
  r0h_circuit circ;
  R0H_TRY(parse_blob(&circ, blob, blob_words));
  if (circ.n_global < 8) return done(R0H_RECEIPT_V_NO_BINDING, 0);
  const size_t n = rc->segments.size();
  // the trace circuit's seals also carry the first and last pc of the segment, how it ends, and the session's public inputs
  const bool trace_circuit = is_trace_circuit(circ);
  for (size_t i = 0; i < n; i++)  // before any claim is read (the chain check below looks one segment ahead)
    if (!rc->segments[i].has_claim) return done(R0H_RECEIPT_V_NO_CLAIM, i);
  // the segment that ends the run: the first whose claim is Halted / Paused; what follows it can only be rows that close the session
  size_t term = n - 1;
  for (size_t i = 0; i < n; i++)
    if (rc->segments[i].claim.exit_system <= 1) { term = i; break; }
  if (!trace_circuit && term != n - 1) return done(R0H_RECEIPT_V_CHAIN, term + 1);
  std::vector<uint32_t> records(trace_circuit ? n * R0H_SESSION_RECORD_WORDS : 0);
  for (size_t i = 0; i < n; i++) {
    const r0h_receipt::Segment& g = rc->segments[i];
    // the seal is verified bound to the control root of the trace size it names
    const uint32_t* root = nullptr;
    const int reach = segment_seal_root(circ, g, control_roots, n_roots, &root);
    if (reach == R0H_RECEIPT_V_SEAL && seal_verdict_out) *seal_verdict_out = R0H_VERIFY_TRUNCATED;
    if (reach != R0H_RECEIPT_V_OK) return done(reach, i);
    int sv = -1;
    uint32_t data_root[8];
    if (verified) {  // verified with the batch, against this very root
      SealCheck& sc = (*verified)[i];
      if (sc.err) { const char* err = sc.err; sc.err = nullptr; return err; }
      sv = sc.verdict;
      memcpy(data_root, sc.data_root, 32);
    } else {
      R0H_TRY(r0h_verify_seal_roots(blob, blob_words, g.seal.data(), g.seal.size(), root, &sv, nullptr, data_root));
    }
    if (sv != R0H_VERIFY_OK) {
      if (seal_verdict_out) *seal_verdict_out = sv;
      return done(R0H_RECEIPT_V_SEAL, i);
    }
    // `SegmentReceipt::verify_integrity`: the claim decoded from the seal's public outputs must be the receipt's claim
    uint8_t cd[32];
    uint32_t want[8];
    claim_digest(g.claim, cd);
    claim_globals(cd, want);
    if (memcmp(want, g.seal.data(), 32) != 0) return done(R0H_RECEIPT_V_CLAIM_MISMATCH, i);
    // the trace circuit proves a run from its public first pc to its public last pc: they are the claim's
    // ... and it ends in a HALT / PAUSE ecall exactly when its public inputs say so, with the exit code they carry: the claim's ExitCode
    if (trace_circuit) {
      if (!trace_seal_carries_claim(g.seal.data(), g.claim)) return done(R0H_RECEIPT_V_CLAIM_MISMATCH, i);
      memcpy(&records[i * R0H_SESSION_RECORD_WORDS], g.seal.data(), (R0H_TRACE_GLOBALS - R0H_TRACE_LATE_GLOBALS) * 4);
      memcpy(&records[i * R0H_SESSION_RECORD_WORDS + (R0H_TRACE_GLOBALS - R0H_TRACE_LATE_GLOBALS)], data_root, 32);
    }
    // composite.rs: indices count up, every segment before the one that ends the run ends in SystemSplit with no output, and hands its
    // post-state on; a segment after it has no cycles (trace circuit: the rows that close the session) and stands where the run stopped
    if (g.index != i) return done(R0H_RECEIPT_V_CHAIN, i);
    static const uint8_t zero[32] = {0};
    if (i != term && (g.claim.exit_system != 2 || g.claim.exit_user != 0 || memcmp(g.claim.output_digest, zero, 32) != 0)) return done(R0H_RECEIPT_V_CHAIN, i);
    if (i + 1 < n) {
      uint8_t a[32], b[32];
      system_state_digest(g.claim.post, a);
      system_state_digest(rc->segments[i + 1].claim.pre, b);
      if (memcmp(a, b, 32) != 0) return done(R0H_RECEIPT_V_CHAIN, i + 1);
    }
    if (i > term) {
      uint8_t a[32], b[32];
      system_state_digest(g.claim.pre, a);
      system_state_digest(g.claim.post, b);
      if (memcmp(a, b, 32) != 0 || g.seal[10] != 0) return done(R0H_RECEIPT_V_CHAIN, i);
    }
  }
  const r0h_receipt_claim& last = rc->segments[term].claim;
  if (!(last.exit_system <= 1 && last.exit_user == 0)) return done(R0H_RECEIPT_V_EXIT_CODE, term);
  uint8_t out[32];
  R0H_TRY(r0h_output_digest(rc->journal.data(), rc->journal.size(), nullptr, out));
  if (memcmp(out, last.output_digest, 32) != 0) return done(R0H_RECEIPT_V_JOURNAL, term);
  if (trace_circuit) {  // the session (session_verdict): numbers, closing segments, the common challenge; then the balance
    std::vector<SessionLeaf> leaves(n);
    for (size_t i = 0; i < n; i++) {
      const uint32_t* sl = rc->segments[i].seal.data();
      leaves[i] = SessionLeaf{sl, &records[i * R0H_SESSION_RECORD_WORDS + (R0H_TRACE_GLOBALS - R0H_TRACE_LATE_GLOBALS)], sl + R0H_TRACE_GAMMA, sl + R0H_TRACE_SUM};
    }
    const SessionOtherSide other{image, image_public, rc->segments[0].claim.pre.merkle_root, rc->journal.data(), rc->journal.size()};
    const bool balanced = image_public || image;  // with neither, nothing can stand for the image's side: the ELF-free checks, then the image id
    size_t leaf = 0;
    const int v = session_verdict(leaves, term, balanced ? &other : nullptr, &leaf);
    if (v != R0H_RECEIPT_V_OK) return done(v, leaf);
    if (!balanced) {
      if (!image_id) return done(R0H_RECEIPT_V_UNBOUND, 0);
      uint8_t pre[32];
      system_state_digest(rc->segments[0].claim.pre, pre);
      if (memcmp(pre, image_id, 32) != 0) return done(R0H_RECEIPT_V_IMAGE_ID, 0);
      return done(R0H_RECEIPT_V_NEEDS_IMAGE, 0);
    }
  }
  if (!image_id) return done(R0H_RECEIPT_V_UNBOUND, 0);  // `receipt.verify(image_id)` always names the program: without it this is not OK
  uint8_t pre[32];
  system_state_digest(rc->segments[0].claim.pre, pre);
  if (memcmp(pre, image_id, 32) != 0) return done(R0H_RECEIPT_V_IMAGE_ID, 0);
  return done(R0H_RECEIPT_V_OK, 0);
  R0H_GUARD_END
}

// The _on forms: every segment seal receipt_verify_impl can come to verify -- the suite named, the seal long enough to name its trace
// size, a control root known for it: the walk stops before any other -- and `extra` (the image seal; may be nullptr) verified as one
// batch on `ctx`.  checks[i] is segment i's (a segment the walk cannot reach keeps verdict -1 and is never looked at), checks[n] the
// extra one.  Anything the walk itself refuses first (no receipt, a malformed blob) leaves the batch empty and the refusal to the walk.
static const char* receipt_seal_batch(r0h_ctx* ctx, const r0h_receipt* rc, const uint32_t* blob, size_t blob_words, const uint32_t* control_roots, size_t n_roots,
                                      const SealCheck* extra, std::vector<SealCheck>& checks) {
  R0H_TRY(require_poseidon2(ctx, "r0h_receipt_verify_on"));
  std::vector<SealCheck> batch;
  std::vector<size_t> slot;
  r0h_circuit circ;
  const bool walkable = rc && blob && (control_roots || !n_roots) && rc->kind == R0H_RECEIPT_COMPOSITE && !rc->segments.empty();
  if (walkable) {
    const char* err = parse_blob(&circ, blob, blob_words);
    const bool parsed = !err;
    if (err) r0h_free_error(err);  // (the walk parses it again and returns this)
    checks.assign(rc->segments.size() + 1, SealCheck{nullptr, 0, nullptr, 0, nullptr});
    for (size_t i = 0; parsed && circ.n_global >= 8 && i < rc->segments.size(); i++) {
      const r0h_receipt::Segment& g = rc->segments[i];
      const uint32_t* root = nullptr;
      if (segment_seal_root(circ, g, control_roots, n_roots, &root) != R0H_RECEIPT_V_OK) continue;
      batch.push_back(SealCheck{blob, blob_words, g.seal.data(), g.seal.size(), root});
      slot.push_back(i);
    }
  } else {
    checks.assign(1, SealCheck{nullptr, 0, nullptr, 0, nullptr});
  }
  if (extra) {
    batch.push_back(*extra);
    slot.push_back(checks.size() - 1);
  }
  R0H_TRY(verify_seals_batch(ctx, HASH_POSEIDON2, batch.data(), batch.size()));
  for (size_t k = 0; k < batch.size(); k++) checks[slot[k]] = batch[k];
  return nullptr;
}
static void free_check_errors(std::vector<SealCheck>& checks) {
  for (SealCheck& sc : checks)
    if (sc.err) { r0h_free_error(sc.err); sc.err = nullptr; }
}

const char* r0h_receipt_verify_elf_on(r0h_ctx* ctx, const r0h_receipt* rc, const uint32_t* blob, size_t blob_words, const uint32_t* control_roots, size_t n_roots,
                                      const uint8_t* elf, size_t elf_len, int* verdict_out, size_t* segment_out, int* seal_verdict_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && elf, "r0h_receipt_verify_elf_on: NULL argument");
  std::vector<std::pair<uint32_t, uint32_t>> image;
  uint32_t entry = 0;
  uint8_t image_id[32];
  R0H_TRY(elf_image(elf, elf_len, image, &entry, image_id));
  std::vector<SealCheck> checks;
  R0H_TRY(receipt_seal_batch(ctx, rc, blob, blob_words, control_roots, n_roots, nullptr, checks));
  const char* err = receipt_verify_impl(rc, blob, blob_words, control_roots, n_roots, image_id, &image, verdict_out, segment_out, seal_verdict_out, nullptr, &checks);
  free_check_errors(checks);
  return err;
  R0H_GUARD_END
}

const char* r0h_receipt_verify(const r0h_receipt* rc, const uint32_t* blob, size_t blob_words, const uint32_t* control_roots, size_t n_roots,
                               const uint8_t* image_id, int* verdict_out, size_t* segment_out, int* seal_verdict_out) {
  return receipt_verify_impl(rc, blob, blob_words, control_roots, n_roots, image_id, nullptr, verdict_out, segment_out, seal_verdict_out);
}

// `receipt.verify(image_id)` for a trace-circuit session, the program image NOT in hand: the receipt's image proof stands for it.
// Checked: the image seal verifies against the image circuit bound to its control root (derived from the blob when not given), its
// digest is the root in the first claim's pre-state -- whose digest must be image_id --, its challenge is this session's; then
// everything r0h_receipt_verify_elf checks, with the image proof's total as the image's side of the balance.
// One body for r0h_receipt_verify_image (on == nullptr: the image seal verified by the immediate verifier, then the walk) and
// r0h_receipt_verify_image_on (the image seal rides in the batch of the segment seals on `on`).
static const char* receipt_verify_image_impl(r0h_ctx* on, const r0h_receipt* rc, const uint32_t* blob, size_t blob_words, const uint32_t* control_roots, size_t n_roots,
                                             const uint32_t* image_blob, size_t image_blob_words, const uint32_t* image_control_root, const uint8_t* image_id,
                                             int* verdict_out, size_t* segment_out, int* seal_verdict_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(rc && blob && image_blob && verdict_out, "r0h_receipt_verify_image: NULL argument");
  if (segment_out) *segment_out = 0;
  if (seal_verdict_out) *seal_verdict_out = R0H_VERIFY_OK;
  r0h_circuit ic;
  R0H_TRY(parse_blob(&ic, image_blob, image_blob_words));
  R0H_REQUIRE(is_image_circuit(ic), "r0h_receipt_verify_image: the second blob is not the image circuit (circuits/image.r0c)");
  if (rc->image_seal.size() <= R0H_IMAGE_GLOBALS) { *verdict_out = R0H_RECEIPT_V_IMAGE_PROOF; return nullptr; }
  int sv = -1;
  uint32_t po2 = 0, root[8];
  std::vector<SealCheck> checks;  // the batch form's
  if (on) {
    // bound to the caller's control root if there is one; without one the root the seal commits to is held to the one derived from
    // the blob once the seal as such holds -- what the two verifications below come to
    const SealCheck image_check{image_blob, image_blob_words, rc->image_seal.data(), rc->image_seal.size(), image_control_root};
    R0H_TRY(receipt_seal_batch(on, rc, blob, blob_words, control_roots, n_roots, &image_check, checks));
    SealCheck& im = checks.back();
    const char* err = im.err;
    im.err = nullptr;
    sv = im.verdict;
    if (!err && sv == R0H_VERIFY_OK && !image_control_root) {
      err = r0h_control_root_host(image_blob, image_blob_words, nullptr, nullptr, im.po2, root);
      if (!err && memcmp(root, im.code_root, 32) != 0) sv = R0H_VERIFY_CODE_ROOT;
    }
    if (err) { free_check_errors(checks); return err; }
  } else {
    if (!image_control_root) {  // a verifier with the blob derives the root of the size the seal names -- once the seal as such holds
      R0H_TRY(r0h_verify_seal(image_blob, image_blob_words, nullptr, nullptr, rc->image_seal.data(), rc->image_seal.size(), &sv, &po2));
      if (sv == R0H_VERIFY_OK) {
        R0H_TRY(r0h_control_root_host(image_blob, image_blob_words, nullptr, nullptr, po2, root));
        image_control_root = root;
      }
    }
    if (image_control_root)
      R0H_TRY(r0h_verify_seal_bound(image_blob, image_blob_words, nullptr, nullptr, rc->image_seal.data(), rc->image_seal.size(), image_control_root, &sv, &po2, nullptr));
  }
  if (sv != R0H_VERIFY_OK) {
    free_check_errors(checks);
    if (seal_verdict_out) *seal_verdict_out = sv;
    *verdict_out = R0H_RECEIPT_V_IMAGE_PROOF;
    return nullptr;
  }
  const char* err = receipt_verify_impl(rc, blob, blob_words, control_roots, n_roots, image_id, nullptr, verdict_out, segment_out, seal_verdict_out, rc->image_seal.data(),
                                        on ? &checks : nullptr);
  free_check_errors(checks);
  return err;
  R0H_GUARD_END
}

const char* r0h_receipt_verify_image(const r0h_receipt* rc, const uint32_t* blob, size_t blob_words, const uint32_t* control_roots, size_t n_roots,
                                     const uint32_t* image_blob, size_t image_blob_words, const uint32_t* image_control_root, const uint8_t* image_id, int* verdict_out,
                                     size_t* segment_out, int* seal_verdict_out) {
  return receipt_verify_image_impl(nullptr, rc, blob, blob_words, control_roots, n_roots, image_blob, image_blob_words, image_control_root, image_id, verdict_out, segment_out,
                                   seal_verdict_out);
}

const char* r0h_receipt_verify_image_on(r0h_ctx* ctx, const r0h_receipt* rc, const uint32_t* blob, size_t blob_words, const uint32_t* control_roots, size_t n_roots,
                                        const uint32_t* image_blob, size_t image_blob_words, const uint32_t* image_control_root, const uint8_t* image_id,
                                        int* verdict_out, size_t* segment_out, int* seal_verdict_out) {
  R0H_REQUIRE(ctx, "r0h_receipt_verify_image_on: NULL argument");
  return receipt_verify_image_impl(ctx, rc, blob, blob_words, control_roots, n_roots, image_blob, image_blob_words, image_control_root, image_id, verdict_out, segment_out,
                                   seal_verdict_out);
}

const char* r0h_receipt_verify_elf(const r0h_receipt* rc, const uint32_t* blob, size_t blob_words, const uint32_t* control_roots, size_t n_roots, const uint8_t* elf,
                                   size_t elf_len, int* verdict_out, size_t* segment_out, int* seal_verdict_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(elf, "r0h_receipt_verify_elf: NULL argument");
  std::vector<std::pair<uint32_t, uint32_t>> image;
  uint32_t entry = 0;
  uint8_t image_id[32];
  R0H_TRY(elf_image(elf, elf_len, image, &entry, image_id));
  return receipt_verify_impl(rc, blob, blob_words, control_roots, n_roots, image_id, &image, verdict_out, segment_out, seal_verdict_out);
  R0H_GUARD_END
}

// ---- a root of the lift / join tree held to what r0h_receipt_verify_elf / _image hold a receipt to, from the session parts its leaves
// left in it (recursion.cpp: r0h_lift takes them from the seal it verified).  Pure host code; no seal is read.
const char* r0h_trace_seal_session_part(const uint32_t* blob, size_t blob_words, const uint32_t* seal, size_t seal_words, uint32_t part_out[R0H_NODE_SESSION_WORDS]) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(blob && seal && part_out, "r0h_trace_seal_session_part: NULL argument");
  r0h_circuit circ;
  R0H_TRY(parse_blob(&circ, blob, blob_words));
  R0H_REQUIRE(is_trace_circuit(circ), "r0h_trace_seal_session_part: the blob is not the trace circuit (circuits/trace.r0c): only its seals carry a session");
  int sv = -1;
  uint32_t data_root[8];
  R0H_TRY(r0h_verify_seal_roots(blob, blob_words, seal, seal_words, nullptr, &sv, nullptr, data_root));
  R0H_REQUIRE(sv == R0H_VERIFY_OK, "r0h_trace_seal_session_part: the seal does not verify: %s", r0h_verify_reason(sv));
  session_part_of(seal, data_root, part_out);
  return nullptr;
  R0H_GUARD_END
}

static const char* root_verify_session_impl(const char* caller, const uint32_t* blob, size_t blob_words, const r0h_node* node, const uint8_t* journal, size_t journal_len,
                                            const uint8_t* image_id, const std::vector<std::pair<uint32_t, uint32_t>>* image, const uint32_t* image_public,
                                            int* verdict_out, size_t* leaf_out) {
  R0H_REQUIRE(blob && node && (journal || !journal_len) && verdict_out && image_id, "%s: NULL argument", caller);
  if (leaf_out) *leaf_out = 0;
  auto done = [&](int v, size_t leaf) { *verdict_out = v; if (leaf_out) *leaf_out = leaf; return (const char*)nullptr; };
  r0h_circuit circ;
  R0H_TRY(parse_blob(&circ, blob, blob_words));
  R0H_REQUIRE(is_trace_circuit(circ), "%s: the blob is not the trace circuit (circuits/trace.r0c): only its sessions are bound this way", caller);
  R0H_REQUIRE(!node->session.empty() && node->session.size() % R0H_NODE_SESSION_WORDS == 0,
              "%s: the node carries no session part (a leaf below it is no trace-circuit segment, or it arrived without one: r0h_node_new)", caller);
  const size_t n = node->session.size() / R0H_NODE_SESSION_WORDS;
  // a segment's number is a coordinate of its session tuples, and R0H_SESSION_TAG_IMAGE / _JOURNAL sit in the same slot at 2^20 + 1, + 2
  R0H_REQUIRE(n < ((size_t)1 << 20), "%s: %zu leaves: a session has fewer than 2^20 segments (their numbers share a field slot with R0H_SESSION_TAG_IMAGE)", caller, n);
  for (size_t i = 0; i < node->session.size(); i++)
    R0H_REQUIRE(node->session[i] < P, "%s: word %zu of leaf %zu's session part is not a canonical field word", caller, i % R0H_NODE_SESSION_WORDS, i / R0H_NODE_SESSION_WORDS);
  std::vector<SessionLeaf> leaves(n);
  for (size_t i = 0; i < n; i++) {
    const uint32_t* w = &node->session[i * R0H_NODE_SESSION_WORDS];
    leaves[i] = SessionLeaf{w, w + (R0H_TRACE_GLOBALS - R0H_TRACE_LATE_GLOBALS), w + R0H_SESSION_RECORD_WORDS, w + R0H_SESSION_RECORD_WORDS + 16};
  }
  const r0h_receipt_claim& claim = node->claim;
  // the leaves chain: the run starts at the claim's first pc, every leaf starts where its predecessor stopped
  for (size_t i = 0; i < n; i++)
    if (leaves[i].early[8] != (i ? leaves[i - 1].early[9] : enc(claim.pre.pc))) return done(R0H_RECEIPT_V_CHAIN, i);
  // the leaf that ends the run: the first that ends in HALT / PAUSE; it carries the claim's way of ending, exit code and last pc; what
  // follows it has no cycles and stands where the run stopped
  size_t term = n - 1;
  for (size_t i = 0; i < n; i++)
    if (leaves[i].early[11] != 0) { term = i; break; }
  {
    const uint32_t* e = leaves[term].early;
    const uint32_t kind = claim.exit_system == 0 ? 1u : claim.exit_system == 1 ? 2u : 0u, code = kind ? claim.exit_user : 0u;
    if (e[9] != enc(claim.post.pc) || e[11] != enc(kind) || e[12] != enc(kind ? 1u : 0u) || e[13] != enc(code & 0xffffu) || e[14] != enc(code >> 16))
      return done(R0H_RECEIPT_V_CLAIM_MISMATCH, term);
  }
  for (size_t i = term + 1; i < n; i++)
    if (leaves[i].early[10] != 0 || leaves[i].early[11] != 0 || leaves[i].early[8] != leaves[i].early[9]) return done(R0H_RECEIPT_V_CHAIN, i);
  if (!(claim.exit_system <= 1 && claim.exit_user == 0)) return done(R0H_RECEIPT_V_EXIT_CODE, term);
  uint8_t out[32];
  R0H_TRY(r0h_output_digest(journal, journal_len, nullptr, out));
  if (memcmp(out, claim.output_digest, 32) != 0) return done(R0H_RECEIPT_V_JOURNAL, term);
  // the program: the claim's pre-state is the image id -- before the session section, so that another program's ELF is told apart by
  // its id (r0h_receipt_verify_elf reaches the balance first and says R0H_RECEIPT_V_SESSION_SUM for it)
  uint8_t pre[32];
  system_state_digest(claim.pre, pre);
  if (memcmp(pre, image_id, 32) != 0) return done(R0H_RECEIPT_V_IMAGE_ID, 0);
  const SessionOtherSide other{image, image_public, claim.pre.merkle_root, journal, journal_len};
  size_t leaf = 0;
  const int v = session_verdict(leaves, term, &other, &leaf);
  return done(v, leaf);
}

const char* r0h_root_verify_session_elf(const uint32_t* blob, size_t blob_words, const r0h_node* node, const uint8_t* journal, size_t journal_len, const uint8_t* elf,
                                        size_t elf_len, int* verdict_out, size_t* leaf_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(elf, "r0h_root_verify_session_elf: NULL argument");
  std::vector<std::pair<uint32_t, uint32_t>> image;
  uint32_t entry = 0;
  uint8_t image_id[32];
  R0H_TRY(elf_image(elf, elf_len, image, &entry, image_id));
  return root_verify_session_impl("r0h_root_verify_session_elf", blob, blob_words, node, journal, journal_len, image_id, &image, nullptr, verdict_out, leaf_out);
  R0H_GUARD_END
}

const char* r0h_root_verify_session_image(const uint32_t* blob, size_t blob_words, const r0h_node* node, const uint8_t* journal, size_t journal_len,
                                          const uint32_t* image_blob, size_t image_blob_words, const uint32_t* image_control_root, const uint32_t* image_seal,
                                          size_t image_seal_words, const uint8_t* image_id, int* verdict_out, size_t* leaf_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(blob && node && image_blob && image_id && verdict_out && (image_seal || !image_seal_words), "r0h_root_verify_session_image: NULL argument");
  if (leaf_out) *leaf_out = 0;
  r0h_circuit ic;
  R0H_TRY(parse_blob(&ic, image_blob, image_blob_words));
  R0H_REQUIRE(is_image_circuit(ic), "r0h_root_verify_session_image: the second blob is not the image circuit (circuits/image.r0c)");
  if (image_seal_words <= R0H_IMAGE_GLOBALS) { *verdict_out = R0H_RECEIPT_V_IMAGE_PROOF; return nullptr; }
  int sv = -1;
  uint32_t po2 = 0, root[8];
  if (!image_control_root) {  // a verifier with the blob derives the root of the size the seal names -- once the seal as such holds
    R0H_TRY(r0h_verify_seal(image_blob, image_blob_words, nullptr, nullptr, image_seal, image_seal_words, &sv, &po2));
    if (sv == R0H_VERIFY_OK) {
      R0H_TRY(r0h_control_root_host(image_blob, image_blob_words, nullptr, nullptr, po2, root));
      image_control_root = root;
    }
  }
  if (image_control_root) R0H_TRY(r0h_verify_seal_bound(image_blob, image_blob_words, nullptr, nullptr, image_seal, image_seal_words, image_control_root, &sv, &po2, nullptr));
  if (sv != R0H_VERIFY_OK) { *verdict_out = R0H_RECEIPT_V_IMAGE_PROOF; return nullptr; }
  return root_verify_session_impl("r0h_root_verify_session_image", blob, blob_words, node, journal, journal_len, image_id, nullptr, image_seal, verdict_out, leaf_out);
  R0H_GUARD_END
}

}  // extern "C"
