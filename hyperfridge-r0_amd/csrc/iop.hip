// The Fiat-Shamir transcript's generator on the device: a state in device memory (a block from the context's pool) and one-wave kernels
// that run the suite's generator over it (hash_suite_device.hpp `Transcript`).  What WriteIop (prover.hip) does on the host with
// commit / commit_elems / rng.ext / rng.bits, in stream order and without a word crossing to the host: digests are read from device
// buffers (a tree's root is its node 1), challenges are written to device buffers, where the kernels that need them read them
// (r0h_fri_fold_buf, merkle_open).  Only r0h_iop_set_state and r0h_iop_state block: they are the hand-over between a host generator
// (SuiteRng::state) and this one.
//
// The chain is sequential and latency-bound, so every kernel here is one workgroup of one wave.  Under Poseidon2 a permutation is
// spread over the 24 lanes of a half-wave (p2_mix_lanes); under SHA-256 every lane runs the same compressions.
#include "hash_suite_device.hpp"

struct r0h_iop {
  r0h_ctx* ctx = nullptr;
  int hashfn = 0;      // the suite it was made under: refused once the context is on another
  r0h::DevBuf state;   // Transcript::state_words words
};

namespace r0h {

template <class T>
__global__ __launch_bounds__(64) void iop_commit_kernel(uint32_t* state, const uint32_t* digest, typename T::Consts k) {
  typename T::Rng rng(state, k);
  rng.mix(digest);
  rng.store(state);
}

template <class T>
__global__ __launch_bounds__(64) void iop_commit_elems_kernel(uint32_t* state, const uint32_t* words, uint32_t n, typename T::Consts k) {
  __shared__ uint32_t digest[8];
  T::hash_slice(digest, words, n, k);
  typename T::Rng rng(state, k);
  rng.mix(digest);
  rng.store(state);
}

// out[0 .. n_words) = n_words field elements in a row (an extension element is four of them)
template <class T>
__global__ __launch_bounds__(64) void iop_draw_kernel(uint32_t* state, uint32_t* out, uint32_t n_words, typename T::Consts k) {
  typename T::Rng rng(state, k);
  for (uint32_t i = 0; i < n_words; i++) {
    const uint32_t v = rng.elem();
    if (threadIdx.x == 0) out[i] = v;
  }
  rng.store(state);
}

// The loop of the sequencer's query step: per query pos = bits(log2 domain) % domain; from the fifth tree on pos %= rows, carried on
// from tree to tree.  idx[t][q]; lane t writes tree t's row.
constexpr uint32_t IOP_MAX_TREES = 16;
struct IopTreeRows { uint32_t rows[IOP_MAX_TREES]; };
template <class T>
__global__ __launch_bounds__(64) void iop_queries_kernel(uint32_t* state, uint32_t* idx, uint32_t log_domain, uint32_t domain, IopTreeRows tr,
                                                          uint32_t n_trees, uint32_t n_queries, typename T::Consts k) {
  typename T::Rng rng(state, k);
  const uint32_t t = threadIdx.x;
  for (uint32_t q = 0; q < n_queries; q++) {
    uint32_t pos = rng.bits(log_domain) % domain;
    if (t < n_trees) {
#pragma unroll
      for (uint32_t j = 4; j < IOP_MAX_TREES; j++)  // (constant indices: the rows stay kernel arguments)
        if (j <= t) pos %= tr.rows[j];
      idx[(size_t)t * n_queries + q] = pos;
    }
  }
  rng.store(state);
}

// f(T{}) for the transcript of the context's suite
template <class F>
static auto with_transcript(const r0h_ctx* ctx, F&& f) {
  return with_suite(ctx, [&](auto suite) { return f(typename decltype(suite)::Transcript{}); });
}
static size_t iop_state_words(int hashfn) { return hashfn == HASH_SHA256 ? ShaTranscript::state_words : P2Transcript::state_words; }

static const char* iop_usable(const r0h_iop* iop, const char* caller) {
  R0H_REQUIRE(iop, "%s: the transcript handle is NULL", caller);
  R0H_REQUIRE(iop->hashfn == iop->ctx->hashfn, "%s: the transcript was made under the %s hash suite, its context is now on %s", caller,
              hashfn_name(iop->hashfn), hashfn_name(iop->ctx->hashfn));
  return nullptr;
}
// words [word_offset, + n) of `buf`, by the caller's name
static const char* iop_window(const char* caller, const r0h_buf* buf, size_t word_offset, size_t n, const uint32_t** at) {
  R0H_REQUIRE(buf, "%s: the buffer is NULL", caller);
  R0H_REQUIRE(word_offset <= buf->bytes / 4 && n <= buf->bytes / 4 - word_offset, "%s: words [%zu, +%zu) outside a buffer of %zu words", caller, word_offset, n,
              buf->bytes / 4);
  *at = u32(buf) + word_offset;
  return nullptr;
}
static const char* iop_check_state(const char* caller, int hashfn, const uint32_t* words, size_t n) {
  const size_t want = iop_state_words(hashfn);
  R0H_REQUIRE(n == want, "%s: the %s generator's state is %zu words, not %zu", caller, hashfn_name(hashfn), want, n);
  if (hashfn == HASH_POSEIDON2)
    for (int i = 0; i < P2_CELLS; i++) R0H_REQUIRE(words[i] < P, "%s: cell %d is not a canonical field element", caller, i);
  const uint32_t limit = hashfn == HASH_SHA256 ? ShaTranscript::pool_limit : P2Transcript::pool_limit;
  R0H_REQUIRE(words[n - 1] <= limit, "%s: pool_used %u is above %u", caller, words[n - 1], limit);
  return nullptr;
}

// A transcript on `ctx` that starts from a host generator's state, which goes up in stream order (no wait): r0h_iop_new with a fresh
// generator, the sequencer's hand-over with the proof's own (prover.hip)
const char* iop_make(r0h_ctx* ctx, const SuiteRng& rng, r0h_iop** out) {
  uint32_t words[SUITE_RNG_MAX_WORDS];
  const size_t n = rng.state(words);
  return iop_make_words(ctx, words, n, out);
}
// ... from the words of such a state, kept from an earlier moment of the host generator (SuiteRng::state)
const char* iop_make_words(r0h_ctx* ctx, const uint32_t* words, size_t n, r0h_iop** out) {
  std::unique_ptr<r0h_iop> iop(new r0h_iop());
  iop->ctx = ctx;
  iop->hashfn = ctx->hashfn;
  R0H_TRY(iop_check_state("r0h_iop_new", iop->hashfn, words, n));
  R0H_TRY(iop->state.alloc(ctx, n * 4));
  R0H_TRY(stage_h2d(ctx, iop->state->ptr, words, n * 4));
  *out = iop.release();
  return nullptr;
}

// n_words field elements in a row into words [word_offset, +n_words) of `out` (an extension element is four of them; the accumulation
// mix of a circuit is n_mix of them)
const char* iop_draw_words(r0h_iop* iop, r0h_buf* out, size_t word_offset, size_t n_words) {
  R0H_TRY(iop_usable(iop, "r0h_iop_draw_ext"));
  R0H_REQUIRE(n_words < ((size_t)1 << 30), "r0h_iop_draw_ext: %zu words are more than one call draws", n_words);
  const uint32_t* at = nullptr;
  R0H_TRY(iop_window("r0h_iop_draw_ext", out, word_offset, n_words, &at));
  if (!n_words) return nullptr;
  r0h_ctx* ctx = iop->ctx;
  return with_transcript(ctx, [&](auto t) {
    using T = decltype(t);
    KScope ks(ctx, T::draw_kernel, (double)n_words * 4);
    hipLaunchKernelGGL(iop_draw_kernel<T>, dim3(1), dim3(64), 0, ctx->stream, u32(iop->state.get()), const_cast<uint32_t*>(at), (uint32_t)n_words, T::consts(ctx));
    return launch_ok(T::draw_kernel);
  });
}

}  // namespace r0h

using namespace r0h;

extern "C" {

const char* r0h_iop_new(r0h_ctx* ctx, r0h_iop** out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && out, "r0h_iop_new: NULL argument");
  R0H_TRY_HIP(hipSetDevice(ctx->device));
  const std::unique_ptr<SuiteRng> fresh = make_suite(ctx->hashfn, &ctx->p2_host)->rng();
  return iop_make(ctx, *fresh, out);
  R0H_GUARD_END
}
const char* r0h_iop_free(r0h_iop* iop) {
  delete iop;  // the state goes back to its context's pool, behind whatever still reads it in stream order
  return nullptr;
}

const char* r0h_iop_set_state(r0h_iop* iop, const uint32_t* words, size_t n) {
  R0H_GUARD_BEGIN
  R0H_TRY(iop_usable(iop, "r0h_iop_set_state"));
  R0H_REQUIRE(words, "r0h_iop_set_state: NULL argument");
  R0H_TRY(iop_check_state("r0h_iop_set_state", iop->hashfn, words, n));
  return r0h_buf_h2d(iop->ctx, iop->state.get(), 0, words, n * 4);
  R0H_GUARD_END
}
const char* r0h_iop_state(r0h_iop* iop, uint32_t* words_out, size_t capacity, size_t* n_out) {
  R0H_GUARD_BEGIN
  R0H_TRY(iop_usable(iop, "r0h_iop_state"));
  R0H_REQUIRE(n_out, "r0h_iop_state: NULL argument");
  *n_out = iop_state_words(iop->hashfn);
  R0H_REQUIRE(words_out && capacity >= *n_out, "r0h_iop_state: the state is %zu words, capacity is %zu", *n_out, capacity);
  return r0h_buf_d2h(iop->ctx, iop->state.get(), 0, words_out, *n_out * 4);
  R0H_GUARD_END
}

const char* r0h_iop_commit(r0h_iop* iop, const r0h_buf* buf, size_t word_offset) {
  R0H_GUARD_BEGIN
  R0H_TRY(iop_usable(iop, "r0h_iop_commit"));
  const uint32_t* digest = nullptr;
  R0H_TRY(iop_window("r0h_iop_commit", buf, word_offset, 8, &digest));
  r0h_ctx* ctx = iop->ctx;
  return with_transcript(ctx, [&](auto t) {
    using T = decltype(t);
    KScope ks(ctx, T::commit_kernel, 32);
    hipLaunchKernelGGL(iop_commit_kernel<T>, dim3(1), dim3(64), 0, ctx->stream, u32(iop->state.get()), digest, T::consts(ctx));
    return launch_ok(T::commit_kernel);
  });
  R0H_GUARD_END
}

const char* r0h_iop_commit_elems(r0h_iop* iop, const r0h_buf* buf, size_t word_offset, size_t n) {
  R0H_GUARD_BEGIN
  R0H_TRY(iop_usable(iop, "r0h_iop_commit_elems"));
  const uint32_t* words = nullptr;
  R0H_TRY(iop_window("r0h_iop_commit_elems", buf, word_offset, n, &words));
  R0H_REQUIRE(n < ((size_t)1 << 31), "r0h_iop_commit_elems: %zu words are more than a slice hash takes", n);
  r0h_ctx* ctx = iop->ctx;
  return with_transcript(ctx, [&](auto t) {
    using T = decltype(t);
    KScope ks(ctx, T::commit_elems_kernel, (double)n * 4);
    hipLaunchKernelGGL(iop_commit_elems_kernel<T>, dim3(1), dim3(64), 0, ctx->stream, u32(iop->state.get()), words, (uint32_t)n, T::consts(ctx));
    return launch_ok(T::commit_elems_kernel);
  });
  R0H_GUARD_END
}

const char* r0h_iop_draw_ext(r0h_iop* iop, r0h_buf* out, size_t word_offset, size_t count) {
  R0H_GUARD_BEGIN
  R0H_TRY(iop_usable(iop, "r0h_iop_draw_ext"));
  R0H_REQUIRE(count < ((size_t)1 << 28), "r0h_iop_draw_ext: %zu elements are more than one call draws", count);
  return iop_draw_words(iop, out, word_offset, 4 * count);
  R0H_GUARD_END
}

const char* r0h_iop_draw_queries(r0h_iop* iop, uint32_t domain, const uint32_t* tree_rows, uint32_t n_trees, uint32_t n_queries, r0h_buf* idx_out,
                                 size_t word_offset) {
  R0H_GUARD_BEGIN
  R0H_TRY(iop_usable(iop, "r0h_iop_draw_queries"));
  R0H_REQUIRE(tree_rows, "r0h_iop_draw_queries: NULL argument");
  R0H_REQUIRE(domain && (domain & (domain - 1)) == 0, "r0h_iop_draw_queries: domain %u is not a power of two", domain);
  R0H_REQUIRE(n_trees >= 1 && n_trees <= IOP_MAX_TREES, "r0h_iop_draw_queries: %u trees outside [1, %u]", n_trees, IOP_MAX_TREES);
  IopTreeRows tr = {{0}};
  for (uint32_t t = 0; t < n_trees; t++) {
    R0H_REQUIRE(tree_rows[t], "r0h_iop_draw_queries: tree %u has no rows", t);
    tr.rows[t] = tree_rows[t];
  }
  const uint32_t* at = nullptr;
  R0H_TRY(iop_window("r0h_iop_draw_queries", idx_out, word_offset, (size_t)n_trees * n_queries, &at));
  if (!n_queries) return nullptr;
  r0h_ctx* ctx = iop->ctx;
  uint32_t log_domain = 0;
  while ((1u << log_domain) < domain) log_domain++;
  return with_transcript(ctx, [&](auto t) {
    using T = decltype(t);
    KScope ks(ctx, T::queries_kernel, (double)n_trees * n_queries * 4);
    hipLaunchKernelGGL(iop_queries_kernel<T>, dim3(1), dim3(64), 0, ctx->stream, u32(iop->state.get()), const_cast<uint32_t*>(at), log_domain, domain, tr, n_trees,
                       n_queries, T::consts(ctx));
    return launch_ok(T::queries_kernel);
  });
  R0H_GUARD_END
}

}  // extern "C"
