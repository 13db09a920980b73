// The two hash suites on the host: what the transcript (prover.hip), the verifier (verify.cpp) and a caller's own transcript hashing
// (r0h_hash_pair_host / r0h_hash_elems_host) run.  Poseidon2 is the code of ctx.cpp behind the suite interface, word for word what
// the sequencer did before there was a second suite.  SHA-256 is recalled from risc0-zkp core/hash/sha (`Sha256HashSuite`,
// `Sha256Rng`) and risc0-sys sha256.h: unpinned (the reference vendors neither); tests/sha_suite_ref.py is normative here.
//
// SHA-256 suite: a digest is eight u32 words, word j = bswap32 of SHA-256 state word j (the digest's bytes in memory are the standard
// big-endian byte order); message word i of a compression = bswap32 of input word i.
//   hash_pair(a, b)        one compression of the IV over the 16 words a || b: no padding, no length
//   hash_elems(words, n)   risc0 `hash_raw_data_slice`: 16-word blocks chained from the IV, the last partial block zero-filled, no
//                          length block; the words are the 32-bit words the buffers hold (Montgomery form); n = 0 gives the IV
//   Sha256Rng              pool0 = SHA-256("Hello"), pool1 = SHA-256("World") (padded hashes, as digests); mix(d): pool0 ^= d, step;
//                          step: pool0 = hash_pair(pool0, pool1), pool1 = hash_pair(pool0, pool1), pool_used = 0; random_u32 steps
//                          when the eight words of pool0 are used up; bits(b) = random_u32 & (2^b - 1); a field element folds six
//                          draws: val = ((val << 32) + next) mod p
#include "internal.hpp"
#include "receipt_types.hpp"

namespace r0h {
namespace {

inline uint32_t bswap(uint32_t x) { return __builtin_bswap32(x); }

// one compression: `st` in the hash's own word order, `in` sixteen input words (byte-swapped into message words here)
void sha_compress(uint32_t st[8], const uint32_t* in) {
  uint32_t w[16];
  for (int i = 0; i < 16; i++) w[i] = bswap(in[i]);
  sha256_compress(st, w);
}

struct P2Rng : SuiteRng {
  const P2Consts* k;
  uint32_t cells[P2_CELLS];
  uint32_t pool_used = 0;
  explicit P2Rng(const P2Consts* kk) : k(kk) { memset(cells, 0, sizeof cells); }
  void mix(const uint32_t digest[8]) override {
    if (pool_used != 0) { p2_mix_host(*k, cells); pool_used = 0; }
    for (int i = 0; i < 8; i++) cells[i] = add(cells[i], digest[i]);  // digests come from the device or the host sponge: canonical
    p2_mix_host(*k, cells);
  }
  uint32_t elem() override {
    if (pool_used == P2_RATE) { p2_mix_host(*k, cells); pool_used = 0; }
    return cells[pool_used++];
  }
  uint32_t bits(uint32_t n) override {
    uint32_t val = dec(elem());
    for (int i = 0; i < 3; i++) { uint32_t nv = dec(elem()); if (val == 0) val = nv; }
    return val & (uint32_t)(((uint64_t)1 << n) - 1);
  }
  size_t state(uint32_t* out) const override {
    memcpy(out, cells, sizeof cells);
    out[P2_CELLS] = pool_used;
    return P2_CELLS + 1;
  }
};
struct P2Suite : HashSuite {
  const P2Consts* k;
  explicit P2Suite(const P2Consts* kk) : k(kk) {}
  int fn() const override { return HASH_POSEIDON2; }
  void hash_pair(const uint32_t* left, const uint32_t* right, uint32_t* out) const override {
    uint32_t st[P2_CELLS] = {0};
    memcpy(st, left, 32);
    memcpy(st + 8, right, 32);
    p2_mix_host(*k, st);
    memcpy(out, st, 32);
  }
  void hash_elems(const uint32_t* words, size_t n, uint32_t digest[8]) const override { p2_hash_elems_host(*k, words, n, digest); }
  bool digests_are_elems() const override { return true; }
  std::unique_ptr<SuiteRng> rng() const override { return std::unique_ptr<SuiteRng>(new P2Rng(k)); }
};

struct ShaRng : SuiteRng {
  uint32_t pool0[8], pool1[8];
  uint32_t pool_used = 0;
  ShaRng() {
    sha256("Hello", 5, (uint8_t*)pool0);
    sha256("World", 5, (uint8_t*)pool1);
  }
  void step() {
    sha_hash_pair_host(pool0, pool1, pool0);
    sha_hash_pair_host(pool0, pool1, pool1);
    pool_used = 0;
  }
  uint32_t random_u32() {
    if (pool_used == 8) step();
    return pool0[pool_used++];
  }
  void mix(const uint32_t digest[8]) override {
    for (int i = 0; i < 8; i++) pool0[i] ^= digest[i];
    step();
  }
  uint32_t elem() override {
    uint64_t val = 0;
    for (int i = 0; i < 6; i++) val = ((val << 32) + random_u32()) % P;
    return enc((uint32_t)val);
  }
  uint32_t bits(uint32_t n) override { return random_u32() & (uint32_t)(((uint64_t)1 << n) - 1); }
  size_t state(uint32_t* out) const override {
    memcpy(out, pool0, 32);
    memcpy(out + 8, pool1, 32);
    out[16] = pool_used;
    return 17;
  }
};
struct ShaSuite : HashSuite {
  int fn() const override { return HASH_SHA256; }
  void hash_pair(const uint32_t* left, const uint32_t* right, uint32_t* out) const override { sha_hash_pair_host(left, right, out); }
  void hash_elems(const uint32_t* words, size_t n, uint32_t digest[8]) const override { sha_hash_elems_host(words, n, digest); }
  bool digests_are_elems() const override { return false; }
  std::unique_ptr<SuiteRng> rng() const override { return std::unique_ptr<SuiteRng>(new ShaRng()); }
};

}  // namespace

void sha_hash_pair_host(const uint32_t* left, const uint32_t* right, uint32_t* out) {
  uint32_t st[8], in[16];
  memcpy(st, SHA_IV, 32);
  memcpy(in, left, 32);
  memcpy(in + 8, right, 32);
  sha_compress(st, in);
  for (int i = 0; i < 8; i++) out[i] = bswap(st[i]);
}
void sha_hash_elems_host(const uint32_t* words, size_t n, uint32_t digest[8]) {
  uint32_t st[8];
  memcpy(st, SHA_IV, 32);
  size_t i = 0;
  for (; i + 16 <= n; i += 16) sha_compress(st, words + i);
  if (i < n) {
    uint32_t in[16] = {0};
    memcpy(in, words + i, (n - i) * 4);
    sha_compress(st, in);
  }
  for (int j = 0; j < 8; j++) digest[j] = bswap(st[j]);
}

const char* hashfn_name(int fn) { return fn == HASH_SHA256 ? "sha-256" : "poseidon2"; }
const char* hashfn_parse(const char* caller, const char* name, int* fn_out) {
  R0H_REQUIRE(name, "%s: the hash function's name is NULL", caller);
  if (!strcmp(name, "poseidon2")) *fn_out = HASH_POSEIDON2;
  else if (!strcmp(name, "sha-256")) *fn_out = HASH_SHA256;
  else return make_error("%s: unknown hash function \"%.32s\" (\"poseidon2\" and \"sha-256\" are the suites)", caller, name);
  return nullptr;
}
std::unique_ptr<HashSuite> make_suite(int fn, const P2Consts* k) {
  if (fn == HASH_SHA256) return std::unique_ptr<HashSuite>(new ShaSuite());
  return std::unique_ptr<HashSuite>(new P2Suite(k));
}
const char* require_poseidon2(const r0h_ctx* ctx, const char* caller) {
  R0H_REQUIRE(ctx && ctx->hashfn == HASH_POSEIDON2,
              "%s: the context's hash suite is %s; receipts, sessions, image proofs and recursion nodes are poseidon2 only "
              "(r0h_ctx_set_hashfn(ctx, \"poseidon2\"))", caller, ctx ? hashfn_name(ctx->hashfn) : "unset (NULL context)");
  return nullptr;
}

}  // namespace r0h

using namespace r0h;

extern "C" {

const char* r0h_ctx_set_hashfn(r0h_ctx* ctx, const char* name) {
  R0H_REQUIRE(ctx, "r0h_ctx_set_hashfn: NULL argument");
  int fn = 0;
  R0H_TRY(hashfn_parse("r0h_ctx_set_hashfn", name, &fn));
  if (fn != ctx->hashfn) ctx_code_commits_drop(ctx, nullptr);  // CODE trees hashed under the suite that is left
  ctx->hashfn = fn;
  return nullptr;
}
const char* r0h_ctx_hashfn(const r0h_ctx* ctx) { return ctx ? hashfn_name(ctx->hashfn) : "poseidon2"; }

const char* r0h_hash_pair_host(const char* hashfn, const uint32_t a[8], const uint32_t b[8], uint32_t out[8]) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(a && b && out, "r0h_hash_pair_host: NULL argument");
  int fn = 0;
  R0H_TRY(hashfn_parse("r0h_hash_pair_host", hashfn, &fn));
  if (fn == HASH_POSEIDON2)
    for (int i = 0; i < 8; i++) R0H_REQUIRE(a[i] < P && b[i] < P, "r0h_hash_pair_host: word %d is not a canonical field element", i);
  make_suite(fn, &p2_default())->hash_pair(a, b, out);
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_hash_elems_host(const char* hashfn, const uint32_t* words, size_t n, uint32_t out[8]) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE((words || n == 0) && out, "r0h_hash_elems_host: NULL argument");
  int fn = 0;
  R0H_TRY(hashfn_parse("r0h_hash_elems_host", hashfn, &fn));
  if (fn == HASH_POSEIDON2)
    for (size_t i = 0; i < n; i++) R0H_REQUIRE(words[i] < P, "r0h_hash_elems_host: word %zu is not a canonical field element", i);
  make_suite(fn, &p2_default())->hash_elems(words, n, out);
  return nullptr;
  R0H_GUARD_END
}

}  // extern "C"
