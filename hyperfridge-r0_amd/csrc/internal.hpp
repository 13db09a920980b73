// Internal definitions shared by the translation units of libr0hip.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "../../include/r0hip.h"
#include "fp.hpp"

namespace r0h {

const char* make_error(const char* fmt, ...);

#define R0H_TRY_HIP(expr)                                                                              \
  do {                                                                                                 \
    hipError_t e__ = (expr);                                                                           \
    if (e__ != hipSuccess) return r0h::make_error("%s:%d: %s: %s", __FILE__, __LINE__, #expr, hipGetErrorString(e__)); \
  } while (0)
#define R0H_TRY(expr)                \
  do {                               \
    const char* m__ = (expr);        \
    if (m__) return m__;             \
  } while (0)
#define R0H_REQUIRE(cond, ...)                        \
  do {                                                \
    if (!(cond)) return r0h::make_error(__VA_ARGS__); \
  } while (0)
#define R0H_GUARD_BEGIN try {
#define R0H_GUARD_END \
  }                   \
  catch (const std::exception& ex) { return r0h::make_error("exception: %s", ex.what()); } \
  catch (...) { return r0h::make_error("unknown exception"); }

constexpr int P2_CELLS = 24, P2_RATE = 16, P2_OUT = 8, P2_HALF_FULL = 4, P2_PARTIAL = 21, P2_ROUNDS = 29;
constexpr int P2_PART_SIGMA_WORDS = (P2_PARTIAL - 1) * (P2_CELLS - 1) + (P2_PARTIAL - 1) * P2_PARTIAL / 2;  // sum_{r=1}^{20} (23 + r) = 670
constexpr uint32_t TW_BITS = 11;            // two-level twiddle tables of 2^11 entries each
constexpr uint32_t TW_SIZE = 1u << TW_BITS;
constexpr uint32_t TWL_BITS = 13;           // in-chunk twiddle table: ROU[13]^i, i < 2^12 (chunks of up to 2^13 words)
constexpr uint32_t TW_TOP = 22;             // the two-level tables hold powers of ROU[22]: every transform of the default segment size
constexpr uint32_t TWB_BITS = 13;           // second table pair for domains above 2^22: powers of ROU[26], 2^13 entries each
constexpr uint32_t TWB_SIZE = 1u << TWB_BITS;
constexpr uint32_t MAX_DOMAIN_PO2 = 26;     // 2^R0H_MAX_PO2 rows x INV_RATE
// Per context: one po2 = 20 segment parks about 8 GiB, one of 2^24 rows about 130 GiB.  What exceeds the limit is released on
// free; an allocation the device refuses drains the context's own pool and is tried once more (buf_alloc_pooled).
constexpr size_t POOL_LIMIT = (size_t)192 << 30;

// Device-resident Poseidon2 tables (Montgomery form).
struct P2Consts {
  uint32_t rc_full[2 * P2_HALF_FULL][P2_CELLS];
  uint32_t rc_partial[P2_PARTIAL];
  uint32_t diag[P2_CELLS];        // Montgomery form of (mu_i - 1)
  uint32_t diag_canon[P2_CELLS];  // canonical (mu_i - 1) and its Shoup companion floor(w 2^32 / p): constant products
  uint32_t diag_shoup[P2_CELLS];
  // Partial rounds with the linear layer of lanes 1..23 deferred (poseidon2_device.hpp): with D_i = mu_i - 1 and
  // kappa_k = sum_{i>=1} D_i^k, all in Montgomery form,
  //   part_sigma: for r = 1..20 the row [D_1^r .. D_23^r, kappa_{r-1}, kappa_{r-2}, .., kappa_0]   (23 + r words each)
  //   part_final: for i = 1..23 the row [D_i^21, D_i^20, .., D_i^0]
  // The kernels' tight correction schedule for these 43 dot products is derived from the compiled-in diagonal
  // (poseidon2_dot_schedule.hpp); whether it covers the words that stand here is found by fill_p2 and kept BESIDE the table
  // (r0h_ctx::p2_tight), not in it: the bytes that are uploaded and compared (ctx_helper, ctx_code_commit) are the table alone.
  uint32_t part_sigma[P2_PART_SIGMA_WORDS];
  uint32_t part_final[(P2_CELLS - 1) * (P2_PARTIAL + 1)];
};

// Optional per-kernel timing (HIP events on the context's stream around every launch of a named kernel family).
struct KTimer {
  std::vector<hipEvent_t> ev;  // start/stop pairs
  size_t used = 0;
  double alg_bytes = 0;        // algorithmic HBM bytes of the recorded launches
};

// The per-phase device time of a proof (ctx.cpp: profile_phase, profile_close).  `names` and `events` belong to the proof in flight;
// r0h_last_profile reports the last profile that was closed, names and times of one length, whatever has been begun since.
struct Profile {
  std::vector<const char*> names;  // static strings, "end" among them once closed
  std::vector<hipEvent_t> events;  // events[i], events[i+1] bracket phase i
  std::vector<const char*> closed_names;
  std::vector<float> closed_ms;
  bool continued = false;  // the next proof that begins adds its phases to `names` instead of starting over (session.cpp: replay_segment)
};

}  // namespace r0h

struct r0h_ctx {
  int device = 0;
  int refs = 1;  // the handle itself + every live buffer / circuit: teardown happens when the last one goes
  int n_cu = 0;  // the device's compute units, asked once by whoever sizes a persistent grid (logup_tape.hpp cu_count)

  hipStream_t stream = nullptr;
  // twiddles: tw_lo[d][i] = w^i, tw_hi[d][i] = w^(i*2^11) with w = ROU_{FWD,REV}[22]; d = 0 forward, 1 inverse
  uint32_t* tw_lo[2] = {nullptr, nullptr};
  uint32_t* tw_hi[2] = {nullptr, nullptr};
  // local table: tw12[d][i] = ROU[TWL_BITS]^i for i < 2^(TWL_BITS - 1) = 4096 (the name is from when chunks ended at 2^12)
  uint32_t* tw12[2] = {nullptr, nullptr};
  // the same for w = ROU_{FWD,REV}[26] with 2^13 entries per level: outer pass of transforms above 2^22 points
  uint32_t* twb_lo[2] = {nullptr, nullptr};
  uint32_t* twb_hi[2] = {nullptr, nullptr};
  uint32_t* pow3_lo = nullptr;  // 3^i, i < 2^11
  uint32_t* pow3_hi = nullptr;  // 3^(i*2^11), i < 2^11 (covers exponents < 2^22)
  uint32_t* pow3_top = nullptr; // 3^(i*2^22), i < 16 (exponents up to 2^26)
  r0h::P2Consts* p2 = nullptr;  // device
  r0h::P2Consts p2_host;
  bool p2_tight = false;        // the tight dot-product schedule covers p2_host (fill_p2): which Poseidon2 kernels with_suite launches
  int hashfn = 0;              // r0h::HashFn: the suite hash_rows / hash_fold / the sequencer follow (r0h_ctx_set_hashfn)
  void* pinned = nullptr;       // pinned host staging ring for small parameter uploads
  size_t pinned_bytes = 0, pinned_off = 0;
  std::multimap<size_t, void*> pool;  // cached device allocations of the sequencer, by size (stream-ordered reuse)
  size_t pool_bytes = 0;              // bytes parked in the pool; above POOL_LIMIT blocks are released instead
  r0h::Profile prof;
  r0h_session_stats session = {0, 0, 0, 0, 0, 0, 0};  // stage timing of the last r0h_prove_elf
  const r0h_circuit* image_circuit = nullptr;  // r0h_ctx_set_image_circuit: sessions on this context attach an image proof to their receipts
  uint64_t session_resident_limit = 0;  // r0h_ctx_set_session_resident_limit (0: an eighth of the device's memory)
  uint64_t session_device_limit = 0;    // r0h_ctx_set_session_device_limit (0: none)
  uint64_t session_device[4] = {0, 0, 0, 0};  // r0h_last_session_device: evicted, replayed, peak count, peak bytes in rows handles
  uint32_t session_tree_tops = 0;       // r0h_ctx_set_session_tree_tops: levels an evicted segment's DATA tree top stops above the leaves (0: no tops kept)
  uint64_t session_tops[3] = {0, 0, 0}; // r0h_last_session_tree_tops: replayed from their top, peak bytes in tops, levels in force
  std::atomic<uint64_t> session_held{0};  // r0h_ctx_session_held_bytes: what unfinished sessions of this context hold (their lanes add and subtract)
  void* session_rows = nullptr;   // session.cpp: the preflight row buffers of r0h_prove_elf, page-locked, kept from one call to the next (session_rows_free)
  std::vector<r0h_ctx*> helpers;  // further contexts of the same device, made on demand by r0h_prove_elf for its extra prover lanes; they go with this one
  bool check_witness = false;     // r0h_ctx_set_check_witness: the sequencer runs r0h_check_witness on every segment before it commits ACCUM
  bool check_balance = false;     // r0h_ctx_set_check_balance: the sequencer runs r0h_logup_check_balance on every segment before it commits DATA
  bool check_session = false;     // r0h_ctx_set_check_session: r0h_session_finish checks the session balance of all segments before it derives the challenge
  uint64_t balance_stats[3] = {0, 0, 0};  // the last r0h_logup_check_balance: tuples, inserts that reached the global table, its slots
  bool device_transcript = false;  // r0h_ctx_set_device_transcript: fri_commit and queries run on the device generator (prover.hip), one read-back for both
  bool device_finish = false;  // r0h_ctx_set_device_finish: steps 3-8 of proof_finish run on the device generator (prover.hip), one read-back for all of them
  int session_enqueue = -1;    // r0h_ctx_set_session_enqueue: phase 2 of a session from the calling thread alone (session.cpp); -1: as R0H_SESSION_ENQUEUE says
  int session_enqueue_begin = -1;  // r0h_ctx_set_session_enqueue_begin: phase 1 from the calling thread as well, the image proof enqueued (session.cpp); -1: as R0H_SESSION_ENQUEUE_BEGIN says
  uint64_t session_phase1[4] = {0, 0, 0, 0};  // r0h_last_session_phase1: host threads started for phase 1, blocking waits in it, segments, evictions
  int merkle_fused_tops = -1;  // r0h_ctx_set_merkle_fused_tops: r0h_merkle_build ends in r0h_hash_fold_top (merkle.hip); -1: as R0H_MERKLE_FUSED_TOPS says
  uint64_t session_phase2[4] = {0, 0, 0, 0};  // r0h_last_session_phase2: host threads, blocking waits, of them ring wraps, of them replays + image proof
  std::atomic<uint64_t> ring_waits{0};      // of blocking_waits: the times stage_h2d waited because the pinned ring had wrapped around
  std::atomic<uint64_t> blocking_waits{0};  // r0h_ctx_blocking_waits: the times the library has waited for this context's stream (ctx_wait)
  bool ktime_on = false;
  std::map<std::string, r0h::KTimer> ktimers;
  // The committed CODE groups of the circuits loaded on this context, by (circuit, po2, hash suite): CODE depends on nothing else, so
  // the sessions of a context commit each once (ctx_code_commit).  The lanes of a session share it under the mutex.  Every entry holds
  // references on the context that made it (this one or one of its helpers), so the entries go explicitly: with their circuit
  // (r0h_circuit_free), when the suite changes (r0h_ctx_set_hashfn) and at r0h_ctx_destroy, before the reference count is looked at.
  // `table`: the Poseidon2 constants the tree was hashed with.  Shared: a session holds its segments' commitments from begin to finish,
  // so an entry that is dropped meanwhile (suite changed, circuit freed, context destroyed) is freed when the last such session lets go.
  struct CodeCommitEntry { std::shared_ptr<r0h_code_commit> cc; r0h::P2Consts table; };
  std::mutex code_commits_mu;
  std::map<std::tuple<const r0h_circuit*, uint32_t, int>, CodeCommitEntry> code_commits;
};

struct r0h_buf {
  r0h_ctx* ctx = nullptr;
  void* ptr = nullptr;
  size_t bytes = 0;
  r0h_buf* parent = nullptr;  // slices keep their parent alive
  int refs = 1;
  bool owned = true;
  bool pooled = false;  // memory returns to the context's pool instead of hipFree
};

namespace r0h {
inline uint32_t* u32(const r0h_buf* b) { return (uint32_t*)b->ptr; }
// the refusal shared by the entry points that name device words as (buffer, word offset), r0h_fri_fold_buf's wording
inline const char* require_words_in(const char* caller, const char* what, const r0h_buf* b, size_t word_offset, size_t n_words) {
  const size_t have = b->bytes / 4;
  R0H_REQUIRE(word_offset <= have && n_words <= have - word_offset, "%s: the %s at words [%zu, +%zu) ends beyond a buffer of %zu words", caller, what, word_offset, n_words,
              have);
  return nullptr;
}
// RAII bracket around the launches of one kernel family; no-op unless r0h_kernel_timing(ctx, 1) was called
struct KScope {
  r0h_ctx* ctx;
  KTimer* t = nullptr;
  KScope(r0h_ctx* c, const char* name, double alg_bytes) : ctx(c) {
    // every operation opens a scope before it launches: also the place where the calling thread is pointed at the context's
    // device (a host thread may drive contexts on several devices; allocations and function attributes go to the current one)
    (void)hipSetDevice(c->device);
    if (!c->ktime_on) return;
    t = &c->ktimers[name];
    if (t->ev.size() < t->used + 2) {
      hipEvent_t a, b;
      (void)hipEventCreate(&a);
      (void)hipEventCreate(&b);
      t->ev.push_back(a);
      t->ev.push_back(b);
    }
    t->alg_bytes += alg_bytes;
    (void)hipEventRecord(t->ev[t->used], c->stream);
  }
  ~KScope() {
    if (!t) return;
    (void)hipEventRecord(t->ev[t->used + 1], ctx->stream);
    t->used += 2;
  }
};
// hipStreamSynchronize on the context's stream, counted: every place the library blocks on a context goes through here
inline hipError_t ctx_wait(r0h_ctx* ctx) {
  ctx->blocking_waits++;
  return hipStreamSynchronize(ctx->stream);
}
// stream-ordered upload of a small host array through the pinned ring (the caller's memory may die on return)
const char* stage_h2d(r0h_ctx* ctx, void* dst_device, const void* src_host, size_t bytes);
// device buffer from the context's pool: no hipMalloc / hipFree (and no implicit device sync) in steady state
const char* buf_alloc_pooled(r0h_ctx* ctx, size_t bytes, r0h_buf** out);
// Owner of one device buffer -- pooled, if alloc() made it: back to its context's pool when the owner goes, or at reset(), where the
// block has to be back before what follows (the next allocation of that size reuses it in stream order); release() hands the pointer on.
struct BufFree { void operator()(r0h_buf* b) const { r0h_buf_free(b); } };
struct DevBuf : std::unique_ptr<r0h_buf, BufFree> {
  const char* alloc(r0h_ctx* ctx, size_t bytes) {
    r0h_buf* b = nullptr;
    R0H_TRY(buf_alloc_pooled(ctx, bytes, &b));
    reset(b);
    return nullptr;
  }
};
// bytes [offset_bytes, +bytes) of `b` as a buffer that owns nothing and is never freed; throws std::out_of_range outside `b`
r0h_buf buf_view(const r0h_buf* b, size_t offset_bytes, size_t bytes);
// A phase of the context's profile opens here, by name (an event on the context's stream); profile_close ends the last one, waits
// for the stream and makes the phases recorded since the last proof began what r0h_last_profile reports.  Host only.
void profile_phase(r0h_ctx* ctx, const char* name);
const char* profile_close(r0h_ctx* ctx);
// profile_close in two halves, for a proof that is enqueued and collected later: profile_end marks the end of the last phase in stream
// order (no wait); profile_collect waits for the stream and closes the profile.  profile_close is one after the other.
void profile_end(r0h_ctx* ctx);
const char* profile_collect(r0h_ctx* ctx);
// after a kernel launch: the launch error, if any, as "<what>: launch failed: <hip text>"
const char* launch_ok(const char* what);
// inverse NTT with the coset shift f(x) -> f(3x) optionally fused into its last pass (sequencer path)
const char* interpolate_ntt(r0h_ctx* ctx, r0h_buf* io, const r0h_buf* src, uint32_t count, uint32_t po2, bool zk_shift);  // src may be io
// batch_evaluate_any over coefficients stored in natural or bit-reversed order (the sequencer keeps them bit-reversed)
const char* evaluate_any(r0h_ctx* ctx, const r0h_buf* coeffs, uint32_t po2, const uint32_t* which, const uint32_t* xs, uint32_t n_eval,
                         r0h_buf* out, bool bitrev_coeffs);
// The forms of four launchers that take a challenge where the device's transcript left it (prover.hip, r0h_ctx_set_device_finish).  None
// of them waits for the stream.  `d_points` is a table of extension points in device memory, four words each; requests and jobs name their
// point by its index in it.
//   ext_powers                out[4k .. 4k + 4) = base^(exps ? exps[k] : k), k < n: a lane per power, square-and-multiply (device pointers)
//   eval_check_dev            r0h_eval_check with poly_mix read from four device words: the power words of the parameter block are filled by ext_powers;
//                             with d_late / d_mix the late public inputs and the mix words of the block are copied from there, device to device
//                             (r0h_proof_late_device: the host words in their places are not read by the kernels)
//   evaluate_any_points       evaluate_any whose request k is (which[k], pt_idx[k]): grouped by point index, `pts` copied device to device
//   mix_poly_coeffs_dev       r0h_mix_poly_coeffs whose column c is weighed by mix^(first_exp + c), mix read from four device words
//   poly_divide_batch_points  poly_divide_batch whose job j divides by (x - point pt_idx[j]): the job table's w, w^E, w^chunk are filled on the
//                             device, and d_report (one device word) becomes 0, or 1 + the first job, in the order given, whose remainder is not zero
// Each is callable on its own through the C ABI, its device words named as (buffer, word offset) (include/r0hip.h, next to r0h_fri_fold_buf):
//   ext_powers -> r0h_ext_powers_buf                 evaluate_any_points -> r0h_batch_evaluate_any_points (natural-order coefficients)
//   eval_check_dev -> r0h_eval_check_mixbuf (without the late words)      mix_poly_coeffs_dev -> r0h_mix_poly_coeffs_mixbuf
//   poly_divide_batch -> r0h_poly_divide_batch       poly_divide_batch_points -> r0h_poly_divide_batch_points
// and so are the small kernels of steps 5 and 6 in prover.hip: r0h_deep_points_buf, r0h_poly_interpolate_regs, r0h_deep_subtract_heads.
const char* ext_powers(r0h_ctx* ctx, uint32_t* d_out, const uint32_t* d_base, const uint32_t* d_exps, uint32_t n);
const char* eval_check_dev(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* eval_accum, const r0h_buf* eval_code, const r0h_buf* eval_data,
                           const uint32_t* global, const uint32_t* mix, const uint32_t* d_poly_mix, r0h_buf* check, const uint32_t* d_late = nullptr,
                           const uint32_t* d_mix = nullptr);
const char* evaluate_any_points(r0h_ctx* ctx, const r0h_buf* coeffs, uint32_t po2, const uint32_t* which, const uint32_t* pt_idx, uint32_t n_eval, const uint32_t* d_points,
                                uint32_t n_points, r0h_buf* out, bool bitrev_coeffs);
const char* mix_poly_coeffs_dev(r0h_ctx* ctx, r0h_buf* combos, uint32_t first_exp, const uint32_t* d_mix, const r0h_buf* input, const uint32_t* combo_of, uint32_t input_count,
                                uint32_t po2);
const char* poly_divide_batch_points(r0h_ctx* ctx, r0h_buf* polys, uint32_t n, const uint32_t* poly_idx, const uint32_t* pt_idx, uint32_t n_jobs, const uint32_t* d_points,
                                     uint32_t n_points, uint32_t* d_report);
// in-place bit reversal of `count` columns of 2^po2 extension elements (16-byte units)
const char* bit_reverse_ext(r0h_ctx* ctx, r0h_buf* io, uint32_t count, uint32_t po2);
// per-device kernel attributes of the NTT family (LDS limits); called by r0h_ctx_create with the device current
const char* ntt_init_device();
// batched synthetic division (DEEP step): job j divides polynomial poly_idx[j] of `polys` by (x - points[4j..]); one read-back
const char* poly_divide_batch(r0h_ctx* ctx, r0h_buf* polys, uint32_t n, const uint32_t* poly_idx, const uint32_t* points, uint32_t n_jobs, uint32_t* remainders_host);
// 2^po2 packed extension elements at `packed` (what r0h_prefix_products / r0h_prefix_sums leave) into the four columns of 2^po2 words
// at `cols`: how the product accumulators (circuit.hip) and the log-derivative ones (logup.hip) reach the ACCUM group (device pointers)
const char* unpack_ext_columns(r0h_ctx* ctx, uint32_t* cols, const uint32_t* packed, uint32_t po2);
// the CODE launch of r0h_witgen alone: the fixed CODE columns of `c` at 2^po2 rows into `code` (stream-ordered, not synchronised)
const char* witgen_code(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, r0h_buf* code);
// the committed CODE group of `c` at 2^po2 rows: CODE from the pool, witgen_code, r0h_code_commit_new
const char* code_commit_of(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, r0h_code_commit** out);
// the same, made once and kept by the circuit's context (r0h_ctx::code_commits): committed on `lane` -- the caller's own context of that
// device -- when it is missing, or was made under other Poseidon2 constants.  The caller shares it with the cache for as long as it
// keeps `out`.
const char* ctx_code_commit(r0h_ctx* lane, const r0h_circuit* c, uint32_t po2, std::shared_ptr<r0h_code_commit>* out);
// takes the cached commitments of `c` on `ctx`, or all of them (c == nullptr), out of the cache: freed here, or by the last session
// that still holds them
void ctx_code_commits_drop(r0h_ctx* ctx, const r0h_circuit* c);
// rv32im.cpp: the preflight rows of segment i are moved out of the machine (the session proves them while the guest runs on)
void vm_take_trace(r0h_vm* vm, size_t i, std::vector<r0h_preflight_row>& rows, std::vector<r0h_preflight_bound>& bounds);
void vm_recycle_trace(r0h_vm* vm, std::vector<r0h_preflight_row>& rows, std::vector<r0h_preflight_bound>& bounds);
void vm_take_spares(r0h_vm* vm, std::vector<std::vector<r0h_preflight_row>>& rows, std::vector<std::vector<r0h_preflight_bound>>& bounds);
// trace.hip: r0h_trace_rows_upload without its wait: the caller keeps `rows` and `bounds` as they are until the copies have run
const char* trace_rows_upload_enqueue(r0h_ctx* ctx, const r0h_preflight_row* rows, size_t n_rows, const r0h_preflight_bound* bounds, size_t n_bounds, uint32_t po2,
                                      const r0h_trace_segment* segment, r0h_trace_rows** rows_out, uint32_t* globals_out);
void session_rows_free(r0h_ctx* ctx);  // session.cpp: unpins and frees the row buffers a context kept (ctx teardown, device still alive)
// the k-th helper context of `ctx` (same device, same Poseidon2 table), created on first use and kept until ctx goes
const char* ctx_helper(r0h_ctx* ctx, size_t k, r0h_ctx** out);
void ctx_retain(r0h_ctx* ctx);
void ctx_release(r0h_ctx* ctx);
// Prover lanes (sessions: session.cpp; the lift / join tree: recursion.cpp).  Lane 0 on the calling thread, the others on threads of
// their own; the first error is kept (and `on_error` told), later ones are freed; every thread has been joined when this returns.
template <class Fn, class OnError>
const char* run_lanes(const std::vector<r0h_ctx*>& lanes, Fn fn, OnError on_error) {
  std::atomic<const char*> first(nullptr);
  auto lane = [&](r0h_ctx* lctx) {
    const char* err = nullptr;
    try {
      err = fn(lctx);
    } catch (const std::exception& ex) {
      err = make_error("exception in a prover lane: %s", ex.what());
    } catch (...) {
      err = make_error("unknown exception in a prover lane");
    }
    if (!err) return;
    const char* none = nullptr;
    if (!first.compare_exchange_strong(none, err)) r0h_free_error(err);
    on_error();
  };
  std::vector<std::thread> workers;
  for (size_t k = 1; k < lanes.size(); k++) workers.emplace_back(lane, lanes[k]);
  lane(lanes[0]);
  for (std::thread& t : workers) t.join();
  return first;
}
// host Poseidon2 (transcript only): permutation over 24 Montgomery words with the context's table
void p2_mix_host(const P2Consts& k, uint32_t* cells);
// table from canonical round constants [29][24] and canonical (mu_i - 1) [24]; the compiled-in risc0 table, filled on first use.
// Returns whether the kernels' tight dot-product schedule covers the table just filled (walked in exact integers): true for the
// compiled-in diagonal, and for any other whose words keep every bound; otherwise the kernels of the safe schedule are launched.
bool fill_p2(P2Consts& k, const uint32_t* rc, const uint32_t* diag_m1);
const P2Consts& p2_default();
void p2_hash_elems_host(const P2Consts& k, const uint32_t* elems, size_t n, uint32_t digest[8]);
void p2_sponge_rows_host(const P2Consts& k, const uint32_t* words, size_t n_words, uint32_t* cols, size_t stride, size_t* rows_used);
// the digest of p2_hash_elems_host and (states != nullptr) the 24 words every permutation of the chain starts from, before its external layer
void p2_sponge_chain_host(const P2Consts& k, const uint32_t* elems, size_t n, uint32_t digest[8], std::vector<uint32_t>* states);

// ---- hash suites (risc0 `HashSuite`: the Merkle hash and the transcript's generator go together).  Two of them: Poseidon2 over
// BabyBear words, and SHA-256 as recalled from risc0-zkp core/hash/sha (`Sha256HashSuite`, `Sha256Rng`) and risc0-sys sha256.h --
// unpinned like everything risc0-specific here (the reference vendors neither); tests/sha_suite_ref.py is this repository's norm.
enum HashFn { HASH_POSEIDON2 = 0, HASH_SHA256 = 1 };
const char* hashfn_name(int fn);                                   // "poseidon2" / "sha-256"
const char* hashfn_parse(const char* caller, const char* name, int* fn_out);  // any other name is an error
// the transcript's generator: what WriteIop (prover.hip) and SealReader (verify.cpp) draw their challenges from
struct SuiteRng {
  virtual ~SuiteRng() {}
  virtual void mix(const uint32_t digest[8]) = 0;
  virtual uint32_t elem() = 0;            // a field element, Montgomery form
  virtual uint32_t bits(uint32_t n) = 0;  // an n-bit query index
  // the generator's words as the device form holds them (r0h_iop_set_state): Poseidon2 the 24 cells and pool_used, SHA-256 pool0,
  // pool1 and pool_used; at most SUITE_RNG_MAX_WORDS of them
  virtual size_t state(uint32_t* words_out) const = 0;
  Fp4 ext() { Fp4 r; for (int i = 0; i < 4; i++) r.e[i] = elem(); return r; }
};
constexpr size_t SUITE_RNG_MAX_WORDS = 25;
// the host side of a suite: hashing of pairs and of word slices (what the device kernels of the suite compute per node / per row)
struct HashSuite {
  virtual ~HashSuite() {}
  virtual int fn() const = 0;
  virtual void hash_pair(const uint32_t* left, const uint32_t* right, uint32_t* out) const = 0;
  virtual void hash_elems(const uint32_t* words, size_t n, uint32_t digest[8]) const = 0;
  virtual bool digests_are_elems() const = 0;  // Poseidon2: every digest word is a field element; SHA-256: any 32-bit value
  virtual std::unique_ptr<SuiteRng> rng() const = 0;
};
// `k` is read by the Poseidon2 suite only and must outlive it (a context's table, or the caller's)
std::unique_ptr<HashSuite> make_suite(int fn, const P2Consts* k);
// SHA-256 suite on the host (hash_suite.cpp): digests are 8 words whose bytes in memory are the standard big-endian SHA-256 bytes
void sha_hash_pair_host(const uint32_t* left, const uint32_t* right, uint32_t* out);
void sha_hash_elems_host(const uint32_t* words, size_t n, uint32_t digest[8]);
// The device side of both suites is hash_suite_device.hpp; r0h_hash_rows / r0h_hash_fold / r0h_hash_fold_top / r0h_merkle_build are in merkle.hip, with the
// two shape checks the Merkle entry points share: "<caller>: rows n is not a power of two" and "<caller>: query q opens row r of an
// n-row tree" for the first idx_host[q] >= rows.
const char* require_pow2_rows(const char* caller, uint32_t rows);
const char* require_rows_in_tree(const char* caller, const uint32_t* idx_host, uint32_t n_q, uint32_t rows);
// merkle_top.hip: packed openings (device pointers, stream-ordered): per query the `cols` values of row d_idx[q], then the sibling
// digests up to the layer a seal carries.  merkle_open: out of a tree held in full, all 2 * rows nodes (no hashing, no suite).
// The rest: a tree kept as its top (digests [0, 2 * rows >> levels)) and the openings made from it under the context's suite.
// merkle_top_copy: r0h_merkle_top under the caller's name.  merkle_open_top: `report` (two device words, reset here) receives
// the count of queries whose subtree does not hash to the top's node and the lowest such query;
// merkle_open_top_verdict makes the caller's error of it ("<caller>: tree top does not match the matrix under query q (row r)").
const char* merkle_open(r0h_ctx* ctx, uint32_t* out, const uint32_t* matrix, const uint32_t* nodes, const uint32_t* d_idx, uint32_t n_q, uint32_t rows, uint32_t cols);
const char* merkle_top_copy(r0h_ctx* ctx, const r0h_buf* nodes, uint32_t rows, uint32_t levels, r0h_buf* top_out, const char* caller);
const char* merkle_open_top(r0h_ctx* ctx, uint32_t* out, const uint32_t* matrix, const uint32_t* top, uint32_t levels, const uint32_t* d_idx, uint32_t n_q, uint32_t rows,
                            uint32_t cols, uint32_t* report);
const char* merkle_open_top_verdict(const char* caller, const uint32_t report[2], const uint32_t* idx_host);
// merkle_climb.hip: packed openings (`cols` values, then `path` sibling digests) hashed from the row up to the node `path` levels above
// it, under the context's suite.  A job names its opening by word offset into one buffer; reached_host[j][8] is the digest job j reaches.
// merkle_climb: the openings are on the device already; merkle_climb_spans: they lie in host memory and go up back to back through the
// staging helpers (offsets count from the first span's first word).  One launch on the context's stream; both block until the digests
// are back.  upload_bytes_out (optional): what went to the device, openings and job table.
struct ClimbJob { uint32_t offset, cols, path, row; };
struct ClimbSpan { const uint32_t* w; size_t n; };
const char* merkle_climb(r0h_ctx* ctx, const uint32_t* d_words, size_t n_words, const ClimbJob* jobs, size_t n_jobs, uint32_t* reached_host);
const char* merkle_climb_spans(r0h_ctx* ctx, const ClimbSpan* spans, size_t n_spans, const ClimbJob* jobs, size_t n_jobs, uint32_t* reached_host, size_t* upload_bytes_out);
// verify.cpp: a batch of seals verified with their Merkle openings collected and hashed together -- on `ctx` (one upload, one launch of
// merkle_climb_kernel, suite and Poseidon2 table the context's) or, ctx == nullptr, on the host under `host_hashfn` with the compiled-in
// table.  Every comparison and every verdict is the host's; verdict and reason are the immediate verifier's for every input.  Per seal:
// `err` (a malformed blob, a non-canonical expected root: what the single-seal entry points return as their error; owned by the caller)
// or verdict, po2, and the CODE / DATA roots the transcript recomputes.
struct SealCheck {
  const uint32_t* blob; size_t blob_words; const uint32_t* seal; size_t seal_words; const uint32_t* expected_code_root;  // in
  const char* err = nullptr;
  int verdict = -1;
  uint32_t po2 = 0, code_root[8] = {0}, data_root[8] = {0};
};
const char* verify_seals_batch(r0h_ctx* ctx, int host_hashfn, SealCheck* seals, size_t n, size_t* upload_bytes_out = nullptr);
// iop.hip: a device transcript that starts from a host generator's state, uploaded in stream order (no wait, unlike r0h_iop_set_state)
const char* iop_make(r0h_ctx* ctx, const SuiteRng& rng, r0h_iop** out);
const char* iop_make_words(r0h_ctx* ctx, const uint32_t* state_words, size_t n, r0h_iop** out);  // from SuiteRng::state words kept earlier
const char* iop_draw_words(r0h_iop* iop, r0h_buf* out, size_t word_offset, size_t n_words);        // r0h_iop_draw_ext by the word
// receipts, sessions, image proofs and recursion nodes name Poseidon2 only: their entry points refuse a context on another suite
const char* require_poseidon2(const r0h_ctx* ctx, const char* caller);
}  // namespace r0h
