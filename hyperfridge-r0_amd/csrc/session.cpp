// `Prover::prove(env, elf)` in the shape hyperfridge calls it (host/src/main.rs:420-423): execute the guest, cut the run
// into segments, prove every segment, assemble the composite receipt.  risc0-zkvm 3.0.5 `LocalProver::prove` = executor
// (`ExecutorImpl::run` -> Session{segments}) + `prove_session` (one `prove_segment` per segment) + CompositeReceipt.
//
// What each stage is here: the executor is csrc/rv32im.cpp (RV32IM by the specification; this library's ecall ABI and cycle model,
// see there); `prove_segment` is the device-resident sequencer (csrc/prover.hip) at the trace size the segment needs; the claim of
// every segment (system states from the run, exit code, the journal's output digest on the last one) is bound to its seal through
// the public inputs (csrc/claim.cpp).
//
// With the trace circuit (circuits/trace.r0c, ProtocolInfo "R0HIP_TRACE:v5__") the seal of a segment attests THAT segment: the
// executor keeps one compact row per cycle plus one per address touched, the device expands them into the DATA group
// (csrc/trace.hip: 72 bytes per cycle cross PCIe, not the 552 bytes of an expanded row), and the proof is over those columns --
// contiguity, every instruction's semantics and memory consistency as include/r0hip.h lists them.  The guest runs ahead on its
// own host thread; two prover lanes (the caller's context and a helper context of the same device) take the segments as they
// are cut.
//
// A session is proved in TWO PHASES, because its segments are tied together by one argument (the session-wide memory
// argument): phase 1 commits the DATA group of every segment and keeps the proofs in flight (288 GB of HBM hold dozens of 3 GB
// commitments); the session challenge is derived from all the DATA roots (and the segments' early public inputs); phase 2 gives
// every proof its late public inputs -- the challenge and the segment's sum under it -- and finishes it.  Ranks that share a
// session exchange 28 words per segment between the phases (r0h_session_begin / _records / _finish; one rank: r0h_prove_elf).
// A session with a device limit (r0h_ctx_set_session_device_limit) keeps the segments beyond it as their compact rows alone and
// commits them a second time in phase 2 (commit_rows, replay_segment): its length is not bounded by the device's memory.
// With r0h_ctx_set_session_tree_tops such a segment also keeps the top of its DATA tree and is committed again without hashing
// (r0h_proof_begin_committed_top); that its rows still belong to the top is then checked where its proof opens the tree, not by
// comparing roots.
// With any other circuit the witness is the blob's synthetic column program with the claim planted: the seal then proves "a
// satisfying trace of the loaded circuit exists whose public inputs name this claim", not "this program ran".
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#include "circuit.hpp"
#include "receipt_types.hpp"

using namespace r0h;

namespace {
using Clock = std::chrono::steady_clock;
double seconds(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }

struct Produced {  // a segment as the executor thread hands it over
  size_t index = 0;
  r0h_vm_segment info;
  r0h_receipt_claim claim;
  std::vector<r0h_preflight_row> rows;
  std::vector<r0h_preflight_bound> bounds;
};

uint32_t trace_size(uint64_t rows) {
  uint32_t po2 = 9;  // the sequencer's smallest trace
  while (((uint64_t)1 << po2) < rows) po2++;
  return po2;
}

// Row buffers a context keeps between sessions (r0h_prove_elf): vectors with their heap blocks, some of them page-locked.
struct RowPool {
  std::mutex mu;  // held by the session that has the buffers
  std::vector<std::vector<r0h_preflight_row>> rows;
  std::vector<std::vector<r0h_preflight_bound>> bounds;
  std::map<const void*, size_t> pinned;
  ~RowPool() { settle(0); }  // unpins every block, then frees them
  void unpin(const void* p) {
    auto it = pinned.find(p);
    if (it == pinned.end()) return;
    (void)hipHostUnregister(const_cast<void*>(p));
    pinned.erase(it);
  }
  // keep at most `cap` row buffers (pinned ones first); a pinned block that is not among them is unpinned BEFORE its vector is freed
  void settle(size_t cap) {
    rows.erase(std::remove_if(rows.begin(), rows.end(), [](const std::vector<r0h_preflight_row>& r) { return !r.capacity(); }), rows.end());
    std::stable_sort(rows.begin(), rows.end(), [&](const std::vector<r0h_preflight_row>& a, const std::vector<r0h_preflight_row>& b) {
      return (pinned.count(a.data()) != 0) > (pinned.count(b.data()) != 0);
    });
    const size_t keep = std::min(cap, rows.size());
    for (auto it = pinned.begin(); it != pinned.end();) {
      bool alive = false;
      for (size_t k = 0; k < keep; k++) alive = alive || rows[k].data() == it->first;
      if (alive) { ++it; continue; }
      (void)hipHostUnregister(const_cast<void*>(it->first));
      it = pinned.erase(it);
    }
    rows.resize(keep);
    if (bounds.size() > cap) bounds.resize(cap);
  }
};
RowPool* pool_of(r0h_ctx* ctx) {
  if (!ctx->session_rows) ctx->session_rows = new RowPool();
  return (RowPool*)ctx->session_rows;
}

// The row buffers of one session call.  They are recycled, so there are a handful of them in a run; each is page-locked the first
// time it is seen (hipHostRegister): the 72 MiB of a segment then cross PCIe by DMA at the link's rate instead of through a staging
// copy.  Pinning 72 MiB costs tens of milliseconds and a fresh buffer as much again in page faults, so the buffers stay with the
// context from one call to the next (RowPool): a second run starts with warm, pinned buffers.  While another session on the context
// has them, this one pins buffers of its own, all of which are unpinned and freed when the call returns.
class RowBuffers {
 public:
  explicit RowBuffers(RowPool* shared) {  // the context's pool (NULL: none), used if no other session has it
    if (shared) lock_ = std::unique_lock<std::mutex>(shared->mu, std::try_to_lock);
    if (lock_.owns_lock()) pool_ = shared;
  }
  // last run's buffers go to the machine, if they have this run's size (the executor reserves min(2^po2, 2^22) rows)
  void lend(r0h_vm* vm, uint32_t segment_po2) {
    const size_t need = (size_t)std::min<uint64_t>((uint64_t)1 << segment_po2, (uint64_t)1 << 22);
    for (size_t k = 0; k < pool_->rows.size(); k++) {
      std::vector<r0h_preflight_bound> b;
      if (k < pool_->bounds.size()) b.swap(pool_->bounds[k]);
      if (pool_->rows[k].capacity() >= need && pool_->rows[k].capacity() <= 2 * need) vm_recycle_trace(vm, pool_->rows[k], b);
      else pool_->unpin(pool_->rows[k].data());
    }
    pool_->rows.clear();
    pool_->bounds.clear();
  }
  void pin(const void* p, size_t bytes) {  // (any lane)
    if (!p || !bytes) return;
    std::lock_guard<std::mutex> lk(pin_mu_);
    auto it = pool_->pinned.find(p);
    if (it != pool_->pinned.end() && it->second >= bytes) return;
    pool_->unpin(p);
    if (hipHostRegister(const_cast<void*>(p), bytes, hipHostRegisterDefault) == hipSuccess) pool_->pinned[p] = bytes;
    else (void)hipGetLastError();  // pageable memory still works, only slower
  }
  // the hand-back, once the executor thread is gone: every buffer the machine holds; what is pinned but not kept is unpinned
  // before its memory is freed
  void take_spares(r0h_vm* vm) {
    vm_take_spares(vm, pool_->rows, pool_->bounds);
    pool_->settle(6);
  }

 private:
  RowPool own_;
  std::unique_lock<std::mutex> lock_;
  RowPool* pool_ = &own_;
  std::mutex pin_mu_;
};

struct VmFree { void operator()(r0h_vm* vm) const { r0h_vm_free(vm); } };

// The executor's side of a session: the guest runs ahead on a thread of its own and a few finished segments wait for a prover lane
// (a 2^20-cycle segment holds 72 MiB of rows).  Only this class locks `mu_`.  It is destroyed before the row buffers it was given:
// the thread is told to stop and joined, then every row buffer goes back, then the queues and the machine go.
class Feed {
 public:
  struct GiveBack { Feed* feed; void operator()(Produced* p) const { feed->give_back(p); } };
  using Segment = std::unique_ptr<Produced, GiveBack>;  // in a lane's hands: whatever leaves the lane's iteration, it comes back
  struct Run {  // what the executor thread leaves behind; read after join()
    int exit_kind = R0H_VM_LIMIT;
    uint32_t exit_code = 0;
    double executor_s = 0;
    r0h_system_state first_pre{};  // of segment 0: the image id
    r0h_vm* vm = nullptr;        // finished: the machine is the caller's again
  };

  Feed(RowBuffers& rows, const r0h_vm_limits& lim, uint32_t part, uint32_t parts) : rows_(rows), lim_(lim), trace_mode_(lim.keep_trace != 0), part_(part), parts_(parts) {}
  ~Feed() {
    stop();
    join();
    if (producer_err_) r0h_free_error(producer_err_);
    if (!vm_) return;
    for (auto& p : queue_) vm_recycle_trace(vm_.get(), p->rows, p->bounds);  // (the machine is this thread's again)
    for (auto& p : returned_) vm_recycle_trace(vm_.get(), p->rows, p->bounds);
    rows_.take_spares(vm_.get());
  }
  const char* start(const uint8_t* elf, size_t elf_len, const uint32_t* input_words, size_t n_input) {
    r0h_vm* vm = nullptr;
    R0H_TRY(r0h_vm_new(&vm));
    vm_.reset(vm);
    R0H_TRY(r0h_vm_load_elf(vm, elf, elf_len));
    R0H_TRY(r0h_vm_set_input(vm, input_words, n_input));
    rows_.lend(vm, lim_.segment_po2);  // (before the executor thread exists: the machine is still this thread's)
    thread_ = std::thread(&Feed::execute, this);
    return nullptr;
  }
  // finished segments that may wait for a prover lane: 2 until the lanes are known, then one more than there are lanes
  void set_lanes(size_t n) {
    std::lock_guard<std::mutex> lk(mu_);
    queue_depth_ = n + 1;
    cv_.notify_all();
  }
  // the next segment for a lane; `seg` stays empty when there is none left or the session was stopped; the executor's error goes
  // to exactly one lane
  const char* next(Segment& seg) {
    std::unique_lock<std::mutex> lk(mu_);
    while (queue_.empty() && !producer_done_ && !stop_) cv_.wait(lk);
    if (stop_) return nullptr;
    if (queue_.empty()) return std::exchange(producer_err_, nullptr);
    seg = Segment(queue_.front().release(), GiveBack{this});
    queue_.pop_front();
    cv_.notify_all();
    return nullptr;
  }
  // a proved segment on its way back: the executor refills its row buffers (they may be page-locked: the pool unpins what it drops)
  void give_back(Produced* p) {
    std::unique_ptr<Produced> seg(p);
    if (!trace_mode_) return;
    std::lock_guard<std::mutex> lk(mu_);
    returned_.push_back(std::move(seg));
  }
  void stop() {  // the lanes and the executor leave at their next look
    std::lock_guard<std::mutex> lk(mu_);
    stop_ = true;
    cv_.notify_all();
  }
  const Run& join() {
    if (thread_.joinable()) thread_.join();
    run_.vm = vm_.get();
    return run_;
  }

 private:
  void execute() {
    r0h_vm* vm = vm_.get();
    const char* err = nullptr;
    try {
      size_t handed = 0;
      for (int finished = 0; !finished && !err;) {
        std::vector<std::unique_ptr<Produced>> back;
        {
          std::unique_lock<std::mutex> lk(mu_);
          while (!stop_ && queue_.size() >= queue_depth_) cv_.wait(lk);
          if (stop_) break;
          back.swap(returned_);
        }
        for (auto& b : back) vm_recycle_trace(vm, b->rows, b->bounds);
        const Clock::time_point t0 = Clock::now();
        err = r0h_vm_run_segment(vm, &lim_, &finished, &run_.exit_kind, &run_.exit_code);
        run_.executor_s += seconds(t0, Clock::now());
        if (err) break;
        // (the end of the run may have cut more than one segment: the last cycles and the rows that close the session)
        for (; handed < r0h_vm_n_segments(vm) && !err; handed++) {
          std::unique_ptr<Produced> p(new Produced());
          const size_t i = handed;
          err = r0h_vm_segment_info(vm, i, &p->info);
          if (!err) err = r0h_vm_segment_claim(vm, i, &p->claim);
          if (err) break;
          p->index = i;
          if (i == 0) run_.first_pre = p->info.pre;
          if (trace_mode_) vm_take_trace(vm, i, p->rows, p->bounds);
          const bool own = i % parts_ == part_;
          std::unique_lock<std::mutex> lk(mu_);
          while (own && !stop_ && queue_.size() >= queue_depth_ + 2) cv_.wait(lk);
          if (!own || stop_) vm_recycle_trace(vm, p->rows, p->bounds);  // another rank's, or nobody left to take it: straight back to the machine
          if (stop_) break;
          if (!own) continue;
          queue_.push_back(std::move(p));
          cv_.notify_all();
        }
      }
    } catch (const std::exception& ex) {
      err = make_error("exception in the executor: %s", ex.what());
    } catch (...) {
      err = make_error("unknown exception in the executor");
    }
    std::lock_guard<std::mutex> lk(mu_);
    producer_err_ = err;
    producer_done_ = true;
    cv_.notify_all();
  }

  RowBuffers& rows_;
  const r0h_vm_limits lim_;
  const bool trace_mode_;
  const uint32_t part_, parts_;
  std::unique_ptr<r0h_vm, VmFree> vm_;
  Run run_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<std::unique_ptr<Produced>> queue_;
  std::vector<std::unique_ptr<Produced>> returned_;  // proved segments on their way back
  bool producer_done_ = false, stop_ = false;
  size_t queue_depth_ = 2;
  const char* producer_err_ = nullptr;
  std::thread thread_;
};

}  // namespace

namespace r0h {
void session_rows_free(r0h_ctx* ctx) {
  delete (RowPool*)ctx->session_rows;
  ctx->session_rows = nullptr;
}
}  // namespace r0h


// the record a segment contributes to the session challenge: its early public inputs, then the root of its DATA commitment
constexpr uint32_t RECORD_WORDS = (R0H_TRACE_GLOBALS - R0H_TRACE_LATE_GLOBALS) + 8;
static_assert(RECORD_WORDS == R0H_SESSION_RECORD_WORDS, "R0H_SESSION_RECORD_WORDS out of step");

struct ProofAbort { void operator()(r0h_proof* p) const { r0h_proof_abort(p); } };
struct RowsFree { void operator()(r0h_trace_rows* h) const { r0h_trace_rows_free(h); } };

// What a pending segment adds to r0h_ctx_session_held_bytes of the session's context: taken back when the segment goes, however it goes.
class Held {
 public:
  Held() {}
  Held(Held&& o) noexcept : ctx_(std::exchange(o.ctx_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
  Held& operator=(Held&& o) noexcept {
    if (this != &o) {
      set(nullptr, 0);
      ctx_ = std::exchange(o.ctx_, nullptr);
      bytes_ = std::exchange(o.bytes_, 0);
    }
    return *this;
  }
  ~Held() { set(nullptr, 0); }
  void set(r0h_ctx* ctx, uint64_t bytes) {
    if (ctx_) ctx_->session_held -= bytes_;
    ctx_ = bytes ? ctx : nullptr;
    bytes_ = ctx_ ? bytes : 0;
    if (ctx_) ctx_->session_held += bytes_;
  }

 private:
  r0h_ctx* ctx_ = nullptr;  // the session's context: the session holds a reference for as long as it has segments
  uint64_t bytes_ = 0;
};

struct Pending {  // a segment between the phases: committed, waiting for the session challenge
  size_t index = 0;
  r0h_ctx* lctx = nullptr;
  std::shared_ptr<r0h_code_commit> cc_held;  // shared with the context's cache (ctx_code_commit); before `proof`: it outlives the proof that reads it
  DevBuf data;
  std::unique_ptr<r0h_proof, ProofAbort> proof;  // in flight (after `data`: it goes first)
  // a session with a device limit: the compact rows on the device, from which the segment is committed again once it has been evicted
  // (a block of its own from the lane's pool: no order towards `data` and `proof`)
  std::unique_ptr<r0h_trace_rows, RowsFree> rows;
  bool evicted = false;  // `proof` and `data` were given up after phase 1: `rows`, `global`, `root`, `claim`, `po2` and the CODE commitment stay
  uint64_t rows_bytes = 0;
  DevBuf top;  // r0h_ctx_set_session_tree_tops: an evicted segment's DATA tree top (from the lane's pool, like `rows`)
  Held held;
  r0h_code_commit* cc = nullptr;
  uint32_t po2 = 0;
  std::vector<uint32_t> global;
  uint32_t root[8] = {0};
  r0h_receipt_claim claim;
  std::vector<uint32_t> seal;  // other circuits: proved at once
  bool done = false;
};

struct r0h_session {
  r0h_ctx* ctx = nullptr;
  const r0h_circuit* c = nullptr;
  bool trace_mode = false;
  uint32_t part = 0, parts = 1;
  size_t n_segments = 0;
  std::mutex result_mu;  // the lanes share `pending`, `stats`, `resident_evaluations`, `device`
  std::vector<Pending> pending;  // this rank's segments, by index
  std::vector<uint8_t> journal;
  std::vector<uint8_t> elf;  // kept for the image proof (r0h_ctx_set_image_circuit) and for the session check's verifier side
  bool check_session = false;  // r0h_ctx_set_check_session was on when the session began
  bool enqueue_begin = false;  // r0h_ctx_set_session_enqueue_begin (or R0H_SESSION_ENQUEUE_BEGIN=1): phase 1 on the calling thread too, the image proof enqueued; implies `enqueue`
  bool enqueue = false;        // r0h_ctx_set_session_enqueue (or R0H_SESSION_ENQUEUE=1) was on when the session began: phase 2 on the calling thread alone
  uint8_t image_id[32] = {0};
  uint64_t cycles = 0;
  r0h_session_stats stats = {0, 0, 0, 0, 0, 0, 0};
  uint64_t resident_limit = 0, resident_evaluations = 0;  // bytes of DATA evaluations kept between the phases (r0h_ctx_set_session_resident_limit)
  // r0h_ctx_set_session_device_limit: `counted` is what the segments that stay committed keep on the device (witness, proof, rows
  // handle), the value held against the limit; `rows_held` the bytes in rows handles, evicted segments' included
  // r0h_ctx_set_session_tree_tops: `tops_levels` (0: none kept), the bytes in kept tops, the segments replayed from theirs
  struct Device {
    uint64_t limit = 0, counted = 0, counted_peak = 0, rows_held = 0, rows_peak = 0, evicted = 0, replayed = 0;
    uint32_t tops_levels = 0;
    uint64_t tops_held = 0, tops_peak = 0, replayed_from_top = 0;
  } device;
  Clock::time_point t_begin;
  std::vector<r0h_ctx*> lane_ctx;
  ~r0h_session() {
    pending.clear();  // proofs aborted, buffers and rows handles freed, their bytes taken off the context's count: before the context is let go
    if (ctx) ctx_release(ctx);
  }
};

namespace {
// The DATA group of a segment from its staged rows, committed: phase 1 of every segment and phase 2 of an evicted one -- the same
// launches over the same rows, so the same root.  `global`: the early public inputs, the late ones still zero.  A segment that kept
// its tree top (`pend.top`, `top_levels`) is committed through it: the same witness, no tree built, the root the top's.
const char* commit_rows(const r0h_circuit* c, Pending& pend, r0h_buf* data, const uint32_t* global, uint32_t root[8], Clock::time_point* t_witness, uint32_t top_levels = 0) {
  R0H_TRY(r0h_trace_rows_expand(pend.rows.get(), data));
  R0H_TRY(r0h_logup_multiplicities(pend.lctx, c, pend.po2, data, global));
  *t_witness = Clock::now();
  r0h_proof* proof = nullptr;
  if (pend.top) R0H_TRY(r0h_proof_begin_committed_top(pend.lctx, c, pend.po2, pend.cc, data, global, pend.top.get(), top_levels, nullptr, &proof));
  else R0H_TRY(r0h_proof_begin_committed(pend.lctx, c, pend.po2, pend.cc, data, global, nullptr, &proof));
  pend.proof.reset(proof);
  return r0h_proof_data_root(proof, root);
}

// Phase 1 of a trace-circuit segment: the rows are staged and expanded on the device, the DATA group is committed, the proof waits in
// `pend` -- or, beyond the session's device limit, only the rows do.
const char* commit_segment(r0h_session* ses, RowBuffers& rows, const Produced& seg, DevBuf& data, std::vector<uint32_t>& global, Pending& pend) {
  const r0h_circuit* c = ses->c;
  const Clock::time_point t0 = Clock::now();
  rows.pin(seg.rows.data(), seg.rows.capacity() * sizeof(r0h_preflight_row));
  const r0h_trace_segment ts = {seg.info.index + 1, seg.info.closing, seg.info.pre.pc, 0};
  r0h_trace_rows* staged = nullptr;
  R0H_TRY(r0h_trace_rows_upload(pend.lctx, seg.rows.data(), seg.rows.size(), seg.bounds.data(), seg.bounds.size(), pend.po2, &ts, &staged, global.data()));
  pend.rows.reset(staged);
  Clock::time_point t1;
  R0H_TRY(commit_rows(c, pend, data.get(), global.data(), pend.root, &t1));
  r0h_session::Device& dev = ses->device;
  if (!dev.limit) pend.rows.reset();  // nothing will be committed twice (multiplicities and the root have waited for the stream: the block is idle)
  pend.rows_bytes = r0h_trace_rows_bytes(pend.rows.get());
  const uint64_t evaluations = ((uint64_t)c->group_size[R0H_GROUP_DATA] << pend.po2) * 16;
  bool lean;
  {  // beyond the session's resident limit a segment waits for the challenge without its evaluations
    std::unique_lock<std::mutex> lk(ses->result_mu);
    lean = ses->resident_evaluations + evaluations > ses->resident_limit;
    if (lean) ses->stats.lean_segments++;
    else ses->resident_evaluations += evaluations;
    lk.unlock();
    if (lean) R0H_TRY(r0h_proof_shrink(pend.proof.get(), nullptr));
  }
  {  // beyond its device limit it waits as rows alone, and is neither resident nor lean
    const uint64_t cost = data->bytes + r0h_proof_resident_bytes(pend.proof.get()) + pend.rows_bytes;
    std::unique_lock<std::mutex> lk(ses->result_mu);
    pend.evicted = dev.limit && dev.counted + cost > dev.limit;
    if (pend.evicted) {
      dev.evicted++;
      if (lean) ses->stats.lean_segments--;
      else ses->resident_evaluations -= evaluations;
    } else {
      dev.counted += cost;
      dev.counted_peak = std::max(dev.counted_peak, dev.counted);
    }
    dev.rows_held += pend.rows_bytes;
    dev.rows_peak = std::max(dev.rows_peak, dev.rows_held);
    lk.unlock();
    uint64_t top_bytes = 0;
    if (pend.evicted && dev.tops_levels) {  // the DATA tree's top stays, device to device, before the tree goes; its root is the recorded one
      top_bytes = ((((uint64_t)R0H_INV_RATE << pend.po2) * 2) >> dev.tops_levels) * 32;
      R0H_TRY(pend.top.alloc(pend.lctx, top_bytes));
      R0H_TRY(r0h_proof_data_top(pend.proof.get(), dev.tops_levels, pend.top.get()));
      uint32_t kept_root[8];
      R0H_TRY(r0h_buf_d2h(pend.lctx, pend.top.get(), 32, kept_root, 32));
      R0H_REQUIRE(!memcmp(kept_root, pend.root, 32), "r0h_session_begin: the tree top kept of segment %zu does not carry its recorded root", pend.index);
      lk.lock();
      dev.tops_held += top_bytes;
      dev.tops_peak = std::max(dev.tops_peak, dev.tops_held);
      lk.unlock();
    }
    if (pend.evicted) {
      pend.proof.reset();  // aborted; then its witness goes back to the lane's pool
      data.reset();
    }
    pend.held.set(ses->ctx, pend.evicted ? pend.rows_bytes + top_bytes : cost);
  }
  const Clock::time_point t2 = Clock::now();
  pend.global = global;
  pend.data = std::move(data);
  std::lock_guard<std::mutex> lk(ses->result_mu);
  ses->stats.witgen_ms += 1e3 * seconds(t0, t1);
  ses->stats.prove_ms += 1e3 * seconds(t1, t2);
  ses->pending.push_back(std::move(pend));
  return nullptr;
}

// A segment of any other circuit, proved at once: the synthetic column program with the claim planted.
const char* prove_synthetic_segment(r0h_session* ses, const Produced& seg, DevBuf& data, std::vector<uint32_t>& global, std::vector<uint32_t>& seal, Pending& pend) {
  const r0h_circuit* c = ses->c;
  const Clock::time_point t0 = Clock::now();
  {  // (CODE is regenerated into a scratch block: only DATA is used)
    DevBuf code;
    R0H_TRY(code.alloc(pend.lctx, ((size_t)c->group_size[R0H_GROUP_CODE] << pend.po2) * 4));
    R0H_TRY(r0h_witgen_public(pend.lctx, c, pend.po2, 0x5E55 + seg.index, global.data(), code.get(), data.get()));
  }
  const Clock::time_point t1 = Clock::now();
  size_t words = 0;
  seal.resize((size_t)1 << 20);
  R0H_TRY(r0h_prove_segment_committed(pend.lctx, c, pend.po2, pend.cc, data.get(), global.data(), seal.data(), seal.size(), &words));
  const Clock::time_point t2 = Clock::now();
  pend.seal.assign(seal.begin(), seal.begin() + words);
  pend.done = true;
  std::lock_guard<std::mutex> lk(ses->result_mu);
  ses->stats.witgen_ms += 1e3 * seconds(t0, t1);
  ses->stats.prove_ms += 1e3 * seconds(t1, t2);
  ses->stats.segments++;
  ses->pending.push_back(std::move(pend));
  return nullptr;
}

// One prover lane of phase 1: every segment the feed has for it, as it arrives.
const char* take_segments(r0h_session* ses, Feed& feed, RowBuffers& rows, r0h_ctx* lctx) {
  const r0h_circuit* c = ses->c;
  std::vector<uint32_t> seal, global(c->n_global);
  for (;;) {
    Feed::Segment seg;
    R0H_TRY(feed.next(seg));
    if (!seg) return nullptr;
    const uint64_t rows_needed = ses->trace_mode ? seg->rows.size() + seg->bounds.size() : seg->info.user_cycles + seg->info.paging_cycles;
    DevBuf data;  // (before `pend`: a proof that fails is aborted before its DATA block goes back)
    Pending pend;
    pend.index = seg->index;
    pend.lctx = lctx;
    pend.claim = seg->claim;
    pend.po2 = trace_size(rows_needed);
    if (ses->trace_mode && pend.po2 < R0H_TRACE_MIN_PO2) pend.po2 = R0H_TRACE_MIN_PO2;
    uint8_t cd[32];
    claim_digest(seg->claim, cd);
    std::fill(global.begin(), global.end(), 0u);
    claim_globals(cd, global.data());
    R0H_TRY(data.alloc(lctx, ((size_t)c->group_size[R0H_GROUP_DATA] << pend.po2) * 4));
    R0H_TRY(ctx_code_commit(lctx, c, pend.po2, &pend.cc_held));
    pend.cc = pend.cc_held.get();  // committed once per (circuit, po2) and kept by the circuit's context
    R0H_TRY(ses->trace_mode ? commit_segment(ses, rows, *seg, data, global, pend) : prove_synthetic_segment(ses, *seg, data, global, seal, pend));
  }
}

uint32_t lane_count() {  // two prover lanes by default
  uint32_t n = 2;
  if (const char* v = getenv("R0H_SESSION_LANES")) n = (uint32_t)strtoul(v, nullptr, 10);
  return n < 1 ? 1 : n > 4 ? 4 : n;
}
bool enqueue_begin_default() {  // R0H_SESSION_ENQUEUE_BEGIN=1, unless the session's context says otherwise
  const char* v = getenv("R0H_SESSION_ENQUEUE_BEGIN");
  return v && strtoul(v, nullptr, 10) == 1;
}
uint64_t lane_waits(const r0h_session* s) {
  uint64_t n = 0;
  for (const r0h_ctx* l : s->lane_ctx) n += l->blocking_waits.load();
  return n;
}

// ---- phase 1 from the calling thread (r0h_ctx_set_session_enqueue_begin).  The thread takes every segment from the executor's queue
// and enqueues all of its phase 1 on the next lane's stream: the upload of its rows, the expansion, the multiplicity kernels and the
// begin of its proof with the transcript on the device (r0h_proof_begin_committed_enqueue).  Nothing of that waits.  What the host needs
// of a segment -- its DATA root for the session's records, and the multiplicity kernels' error word -- is gathered device to device
// into one buffer per lane (GATHER_WORDS a segment) and read back once per lane when the executor has finished.  A segment's rows are
// page-locked host memory the executor wants back: they stay with the lane until the event behind their copy has passed, which is
// looked at, without waiting, at every segment (a lane that holds more than two such segments waits for its oldest copy, counted).  A segment beyond the device
// limit needs its root before it gives up its proof: that read-back (r0h_proof_data_root) is the one wait of an eviction; the abort
// behind it finds the stream idle.  A segment beyond the resident limit gives its evaluations back as it is begun (r0h_proof_shrink
// waits, as ever: one wait each, counted).
constexpr uint32_t GATHER_WORDS = 9, GATHER_SLOTS = 64;
const char* begin_enqueued(r0h_session* ses, Feed& feed, RowBuffers& rows) {
  const r0h_circuit* c = ses->c;
  struct Upload { Feed::Segment seg; hipEvent_t done; };
  struct Lane { r0h_ctx* ctx; bool was_finish; DevBuf gather; std::vector<size_t> slots; std::deque<Upload> uploads; };
  std::vector<Lane> lanes;
  for (r0h_ctx* l : ses->lane_ctx) {
    lanes.push_back(Lane{l, l->device_finish, DevBuf(), {}, {}});
    l->device_finish = true;  // for the length of the phase, as phase 2 does
  }
  std::vector<Pending> made;
  r0h_session::Device& dev = ses->device;
  const uint64_t waits0 = lane_waits(ses);
  // the rows whose copies have run go back to the executor, oldest first; a lane keeps the rows of at most `keep` segments whose
  // copies have not (72 MiB each at 2^20 rows): beyond that it waits for the oldest copy, and the wait is counted
  auto release = [&](Lane& l, size_t keep) {
    while (!l.uploads.empty()) {
      Upload& u = l.uploads.front();
      if (!u.done || hipEventQuery(u.done) != hipSuccess) {  // (no event: the segment's enqueue failed before it had one)
        (void)hipGetLastError();
        if (l.uploads.size() <= keep) return;
        l.ctx->blocking_waits++;
        if (u.done) (void)hipEventSynchronize(u.done);
        else (void)hipStreamSynchronize(l.ctx->stream);
      }
      if (u.done) (void)hipEventDestroy(u.done);
      l.uploads.pop_front();
    }
  };
  auto flush = [&](Lane& l) -> const char* {  // the lane's gathered words come home: one read-back
    if (l.slots.empty()) return nullptr;
    std::vector<uint32_t> host(l.slots.size() * GATHER_WORDS);
    R0H_TRY(r0h_buf_d2h(l.ctx, l.gather.get(), 0, host.data(), host.size() * 4));
    for (size_t k = 0; k < l.slots.size(); k++) {
      memcpy(made[l.slots[k]].root, host.data() + k * GATHER_WORDS, 32);
      R0H_TRY(logup_multiplicities_verdict(host[k * GATHER_WORDS + 8]));
    }
    l.slots.clear();
    return nullptr;
  };
  std::vector<uint32_t> global(c->n_global);
  const char* err = [&]() -> const char* {
    for (size_t k = 0;; k++) {
      Feed::Segment taken;
      R0H_TRY(feed.next(taken));
      if (!taken) break;
      Lane& l = lanes[k % lanes.size()];
      r0h_ctx* lctx = l.ctx;
      R0H_TRY_HIP(hipSetDevice(lctx->device));
      for (Lane& other : lanes) release(other, 2);
      // from here on the lane keeps the rows, whatever becomes of the segment: a copy that reads them may be queued when a later step fails
      l.uploads.push_back(Upload{std::move(taken), nullptr});
      const Produced* const seg = l.uploads.back().seg.get();
      DevBuf data;  // (before `pend`: a proof that fails is aborted before its DATA block goes back)
      Pending pend;
      pend.index = seg->index;
      pend.lctx = lctx;
      pend.claim = seg->claim;
      pend.po2 = trace_size(seg->rows.size() + seg->bounds.size());
      if (pend.po2 < R0H_TRACE_MIN_PO2) pend.po2 = R0H_TRACE_MIN_PO2;
      uint8_t cd[32];
      claim_digest(seg->claim, cd);
      std::fill(global.begin(), global.end(), 0u);
      claim_globals(cd, global.data());
      R0H_TRY(data.alloc(lctx, ((size_t)c->group_size[R0H_GROUP_DATA] << pend.po2) * 4));
      R0H_TRY(ctx_code_commit(lctx, c, pend.po2, &pend.cc_held));  // (the first segment of a size on a context commits CODE, and waits for it)
      pend.cc = pend.cc_held.get();
      const Clock::time_point t0 = Clock::now();
      rows.pin(seg->rows.data(), seg->rows.capacity() * sizeof(r0h_preflight_row));
      const r0h_trace_segment ts = {seg->info.index + 1, seg->info.closing, seg->info.pre.pc, 0};
      r0h_trace_rows* staged = nullptr;
      R0H_TRY(trace_rows_upload_enqueue(lctx, seg->rows.data(), seg->rows.size(), seg->bounds.data(), seg->bounds.size(), pend.po2, &ts, &staged, global.data()));
      pend.rows.reset(staged);
      R0H_TRY_HIP(hipEventCreateWithFlags(&l.uploads.back().done, hipEventDisableTiming));
      R0H_TRY_HIP(hipEventRecord(l.uploads.back().done, lctx->stream));
      if (!l.gather) R0H_TRY(l.gather.alloc(lctx, (size_t)GATHER_SLOTS * GATHER_WORDS * 4));
      if (l.slots.size() == GATHER_SLOTS) R0H_TRY(flush(l));
      const size_t at = l.slots.size() * GATHER_WORDS;
      R0H_TRY(r0h_trace_rows_expand(pend.rows.get(), data.get()));
      R0H_TRY(logup_multiplicities_enqueue(lctx, c, pend.po2, data.get(), global.data(), l.gather.get(), at + 8));
      const Clock::time_point t1 = Clock::now();
      r0h_proof* proof = nullptr;
      R0H_TRY(r0h_proof_begin_committed_enqueue(lctx, c, pend.po2, pend.cc, data.get(), global.data(), nullptr, &proof));
      pend.proof.reset(proof);
      R0H_TRY(r0h_proof_data_root_device(proof, l.gather.get(), at));
      if (!dev.limit) pend.rows.reset();  // nothing will be committed twice (the block goes back to the lane's pool in stream order)
      pend.rows_bytes = r0h_trace_rows_bytes(pend.rows.get());
      const uint64_t cost = data->bytes + r0h_proof_resident_bytes(proof) + pend.rows_bytes;
      pend.evicted = dev.limit && dev.counted + cost > dev.limit;
      uint64_t top_bytes = 0;
      if (pend.evicted) {
        dev.evicted++;
        if (dev.tops_levels) {  // the DATA tree's top stays, device to device (merkle_top_copy out of the nodes the root is read from)
          top_bytes = ((((uint64_t)R0H_INV_RATE << pend.po2) * 2) >> dev.tops_levels) * 32;
          R0H_TRY(pend.top.alloc(lctx, top_bytes));
          R0H_TRY(r0h_proof_data_top(proof, dev.tops_levels, pend.top.get()));
          dev.tops_held += top_bytes;
          dev.tops_peak = std::max(dev.tops_peak, dev.tops_held);
        }
        R0H_TRY(r0h_proof_data_root(proof, pend.root));  // the wait of an eviction: everything the segment had on the stream has run
        pend.proof.reset();                               // (aborted without a second wait)
        data.reset();
      } else {
        dev.counted += cost;
        dev.counted_peak = std::max(dev.counted_peak, dev.counted);
        // beyond the session's resident limit a segment waits for the challenge without its evaluations: given back as it is begun, as
        // in the lanes' form (r0h_proof_shrink waits for the lane's stream: one wait a lean segment, counted)
        const uint64_t evaluations = ((uint64_t)c->group_size[R0H_GROUP_DATA] << pend.po2) * 16;
        if (ses->resident_evaluations + evaluations > ses->resident_limit) {
          ses->stats.lean_segments++;
          R0H_TRY(r0h_proof_shrink(proof, nullptr));
        } else {
          ses->resident_evaluations += evaluations;
        }
      }
      dev.rows_held += pend.rows_bytes;
      dev.rows_peak = std::max(dev.rows_peak, dev.rows_held);
      pend.held.set(ses->ctx, pend.evicted ? pend.rows_bytes + top_bytes : cost);
      pend.global = global;
      pend.data = std::move(data);
      ses->stats.witgen_ms += 1e3 * seconds(t0, t1);
      ses->stats.prove_ms += 1e3 * seconds(t1, Clock::now());
      made.push_back(std::move(pend));
      l.slots.push_back(made.size() - 1);
    }
    for (Lane& l : lanes) R0H_TRY(flush(l));
    return nullptr;
  }();
  for (Lane& l : lanes) {
    if (err) (void)ctx_wait(l.ctx);  // what was launched reads the rows: it runs out before they go back
    release(l, 0);  // (behind the lane's read-back every copy has run)
    l.ctx->device_finish = l.was_finish;
  }
  const uint64_t phase1[4] = {0, lane_waits(ses) - waits0, made.size(), dev.evicted};
  memcpy(ses->ctx->session_phase1, phase1, sizeof phase1);
  if (err) return err;  // (`made` goes: proofs aborted, buffers back)
  for (Pending& p : made) ses->pending.push_back(std::move(p));
  return nullptr;
}
bool enqueue_default() {  // R0H_SESSION_ENQUEUE=1: sessions finish from one host thread unless their context says otherwise
  const char* v = getenv("R0H_SESSION_ENQUEUE");
  return v && strtoul(v, nullptr, 10) == 1;
}
}  // namespace

extern "C" {

const char* r0h_last_session_stats(r0h_ctx* ctx, r0h_session_stats* out) {
  R0H_REQUIRE(ctx && out, "r0h_last_session_stats: NULL argument");
  *out = ctx->session;
  return nullptr;
}

const char* r0h_last_session_phase2(r0h_ctx* ctx, uint64_t out[4]) {
  R0H_REQUIRE(ctx && out, "r0h_last_session_phase2: NULL argument");
  memcpy(out, ctx->session_phase2, sizeof ctx->session_phase2);
  return nullptr;
}

const char* r0h_last_session_phase1(r0h_ctx* ctx, uint64_t out[4]) {
  R0H_REQUIRE(ctx && out, "r0h_last_session_phase1: NULL argument");
  memcpy(out, ctx->session_phase1, sizeof ctx->session_phase1);
  return nullptr;
}

const char* r0h_session_free(r0h_session* s) {
  delete s;
  return nullptr;
}

// Phase 1: execute the guest, cut it into segments, and -- for this rank's share of them -- expand the rows on the device and commit
// the DATA group (trace circuit), or prove outright (any other circuit).
const char* r0h_session_begin(r0h_ctx* ctx, const r0h_circuit* c, const uint8_t* elf, size_t elf_len, const uint32_t* input_words, size_t n_input, uint32_t segment_po2,
                              uint64_t max_cycles, uint32_t part, uint32_t parts, r0h_session** session_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && c && elf && session_out && (input_words || !n_input), "r0h_prove_elf: NULL argument");
  R0H_TRY(require_poseidon2(ctx, "r0h_prove_elf / r0h_session_begin"));
  R0H_REQUIRE(parts >= 1 && part < parts, "r0h_prove_elf_part: part %u of %u", part, parts);
  const bool trace_mode = !memcmp(c->info, "R0HIP_TRACE:v5__", 16);
  // (a trace-circuit segment of fewer than 2^16 rows is proved at 2^16: the lookup tables' size)
  R0H_REQUIRE(segment_po2 >= 9 && segment_po2 <= (trace_mode ? R0H_TRACE_MAX_PO2 : R0H_MAX_PO2), "r0h_prove_elf: segment_po2 %u outside [9, %u]", segment_po2,
              (unsigned)(trace_mode ? R0H_TRACE_MAX_PO2 : R0H_MAX_PO2));
  R0H_REQUIRE(c->has_column_program, "r0h_prove_elf: the circuit has no column program (CODE columns, accumulation)");
  R0H_REQUIRE(c->n_global >= 8, "r0h_prove_elf: the circuit exposes %u public inputs, a claim needs 8", c->n_global);
  if (trace_mode)
    R0H_REQUIRE(c->n_global == R0H_TRACE_GLOBALS && c->n_late == R0H_TRACE_LATE_GLOBALS && c->group_size[R0H_GROUP_DATA] == R0H_TRACE_COLUMNS,
                "r0h_prove_elf: this trace circuit is not the one the library was built for");
  else
    R0H_REQUIRE(c->n_late == 0, "r0h_prove_elf: a circuit with late public inputs other than the trace circuit");
  if (!max_cycles) max_cycles = R0H_DEFAULT_SESSION_LIMIT;  // a guest that never halts must not hang the host (risc0: session limit)
  std::unique_ptr<r0h_session> ses(new r0h_session());
  ses->ctx = ctx;
  ctx_retain(ctx);
  ses->c = c;
  ses->trace_mode = trace_mode;
  ses->part = part;
  ses->parts = parts;
  ses->t_begin = Clock::now();
  R0H_REQUIRE(!(trace_mode && ctx->check_session) || parts == 1,
              "r0h_session_begin: r0h_ctx_set_check_session is on and this is part %u of %u: a rank sees its own segments only, the session check covers single-rank sessions", part, parts);
  ses->check_session = trace_mode && ctx->check_session;
  ses->enqueue = trace_mode && (ctx->session_enqueue < 0 ? enqueue_default() : ctx->session_enqueue > 0);
  ses->enqueue_begin = trace_mode && (ctx->session_enqueue_begin < 0 ? enqueue_begin_default() : ctx->session_enqueue_begin > 0);
  R0H_REQUIRE(!ses->enqueue_begin || parts == 1,
              "r0h_session_begin: r0h_ctx_set_session_enqueue_begin is on and this is part %u of %u: a sharded session runs its first phase on lane threads (turn the switch off)", part, parts);
  if (ses->enqueue_begin) ses->enqueue = true;  // phase 2 from the calling thread as well
  if (trace_mode && ((ctx->image_circuit && part == 0) || ses->check_session)) ses->elf.assign(elf, elf + elf_len);
  ses->device.limit = trace_mode ? ctx->session_device_limit : 0;
  ses->device.tops_levels = ses->device.limit ? ctx->session_tree_tops : 0;  // (only an evicted segment keeps a top)
  ses->resident_limit = ctx->session_resident_limit;
  if (!ses->resident_limit) {
    size_t free_b = 0, total_b = 0;
    R0H_TRY_HIP(hipSetDevice(ctx->device));
    R0H_TRY_HIP(hipMemGetInfo(&free_b, &total_b));
    ses->resident_limit = total_b / 8;  // 36 GB of 288: 17 segments of 2^20 rows; the camt53 stand-in's 12 stay whole, the reference's 37 do not
  }
  r0h_vm_limits lim;
  memset(&lim, 0, sizeof lim);
  lim.segment_po2 = segment_po2;
  lim.max_cycles = max_cycles;
  lim.keep_trace = lim.boundary_rows = trace_mode ? 1 : 0;

  // ---- the executor runs ahead on its own thread (`feed` goes before `rows`: the thread is joined before any row buffer is let go)
  RowBuffers rows(trace_mode ? pool_of(ctx) : nullptr);
  Feed feed(rows, lim, part, parts);
  R0H_TRY(feed.start(elf, elf_len, input_words, n_input));

  // ---- every segment as it arrives.  Two prover lanes by default (R0H_SESSION_LANES = 1..4): lane 0 is the caller's context on the
  // calling thread, the others are helper contexts of the same device (kept with `ctx` between calls) on threads of their own -- while
  // one lane waits for a transcript read-back the other keeps the device busy.  The circuit and the CODE commitments are shared.
  ses->lane_ctx.assign(lane_count(), ctx);
  for (size_t k = 1; k < ses->lane_ctx.size(); k++) R0H_TRY(ctx_helper(ctx, k - 1, &ses->lane_ctx[k]));
  feed.set_lanes(ses->lane_ctx.size());
  if (ses->enqueue_begin) {
    R0H_TRY(begin_enqueued(ses.get(), feed, rows));
  } else {
    const uint64_t waits0 = lane_waits(ses.get());
    R0H_TRY(run_lanes(ses->lane_ctx, [&](r0h_ctx* lctx) { return take_segments(ses.get(), feed, rows, lctx); }, [&] { feed.stop(); }));
    const uint64_t phase1[4] = {ses->lane_ctx.size() - 1, lane_waits(ses.get()) - waits0, ses->pending.size(), ses->device.evicted};
    memcpy(ctx->session_phase1, phase1, sizeof phase1);
  }

  const Feed::Run& run = feed.join();
  R0H_REQUIRE(run.exit_kind != R0H_VM_LIMIT, "r0h_prove_elf: the guest did not halt within %llu cycles (session limit)", (unsigned long long)max_cycles);
  R0H_REQUIRE(run.exit_code == 0, "r0h_prove_elf: the guest exited with code %u", run.exit_code);  // `prove` is an Err for a failed guest
  ses->n_segments = r0h_vm_n_segments(run.vm);
  std::sort(ses->pending.begin(), ses->pending.end(), [](const Pending& a, const Pending& b) { return a.index < b.index; });
  size_t own = 0;
  for (size_t i = part; i < ses->n_segments; i += parts) own++;
  R0H_REQUIRE(ses->pending.size() == own, "r0h_prove_elf: %zu of this rank's %zu segments were committed", ses->pending.size(), own);
  ses->cycles = r0h_vm_cycles(run.vm);
  const uint8_t* journal; size_t journal_len;
  R0H_TRY(r0h_vm_journal(run.vm, &journal, &journal_len));
  ses->journal.assign(journal, journal + journal_len);
  system_state_digest(run.first_pre, ses->image_id);  // the image id the verifier is given: digest of the state the run started from
  ses->stats.cycles = ses->cycles;
  ses->stats.executor_s = run.executor_s;
  *session_out = ses.release();
  return nullptr;
  R0H_GUARD_END
}

size_t r0h_session_n_segments(const r0h_session* s) { return s ? s->n_segments : 0; }

// what this rank's segments contribute to the session challenge: R0H_SESSION_RECORD_WORDS words each (early public inputs, DATA root),
// with their indices; a circuit without a session argument contributes nothing
const char* r0h_session_records(const r0h_session* s, uint32_t* indices_out, uint32_t* records_out, size_t capacity, size_t* n_out) {
  R0H_REQUIRE(s && n_out, "r0h_session_records: NULL argument");
  *n_out = s->trace_mode ? s->pending.size() : 0;
  if (!s->trace_mode) return nullptr;
  R0H_REQUIRE(capacity >= s->pending.size() && indices_out && records_out, "r0h_session_records: room for %zu records wanted", s->pending.size());
  const uint32_t n_early = R0H_TRACE_GLOBALS - R0H_TRACE_LATE_GLOBALS;
  for (size_t k = 0; k < s->pending.size(); k++) {
    indices_out[k] = (uint32_t)s->pending[k].index;
    memcpy(records_out + k * RECORD_WORDS, s->pending[k].global.data(), n_early * 4);
    memcpy(records_out + k * RECORD_WORDS + n_early, s->pending[k].root, 32);
  }
  return nullptr;
}

namespace {
struct SessionBalanceFree { void operator()(r0h_session_balance* sb) const { r0h_session_balance_free(sb); } };
// The session's own share of the session balance: every pending segment's session tuples into `sb` (a device handle; `source` is the
// segment's index), in index order -- what check_session below and r0h_session_balance_add_session both add.  *own_proof: a proof on
// the handle's context is still to be finished.
const char* add_pending_segments(r0h_session* s, r0h_session_balance* sb, bool* own_proof) {
  r0h_ctx* ctx = sb->ctx;
  for (Pending& p : s->pending) {  // in index order
    // an evicted segment's witness is expanded again for its addition, into a block that goes back behind it.  The multiplicity
    // columns stay zero there: the addition walks the accumulators with a public total only, and those read no table column
    // (balance.hip builds its tape from accumulators n_chain.. alone; the tables' fractions are links of the chain).
    DevBuf again;
    if (p.evicted) {
      R0H_TRY(again.alloc(p.lctx, ((size_t)s->c->group_size[R0H_GROUP_DATA] << p.po2) * 4));
      R0H_TRY(r0h_trace_rows_expand(p.rows.get(), again.get()));
    }
    if (p.lctx != ctx) R0H_TRY(r0h_sync(p.lctx));
    else *own_proof = *own_proof || !p.done;
    const r0h_buf* code_cols = nullptr;
    R0H_TRY(r0h_code_commit_columns(p.cc, &code_cols));
    R0H_TRY(r0h_session_balance_add(sb, (uint32_t)p.index, s->c, p.po2, code_cols, p.evicted ? again.get() : p.data.get(), p.global.data()));
  }
  return nullptr;
}
// r0h_ctx_set_check_session: between the phases, before the challenge exists -- every segment's session tuples (their DATA witnesses
// are still resident, lean segments included) and the verifier's side from the ELF and the run's journal must cancel class by class.
// A session that does not balance is this call's error, by the name of its lowest class, and its proofs are aborted.
const char* check_session(r0h_session* s) {
  r0h_ctx* ctx = s->ctx;
  profile_phase(ctx, "check_session");
  r0h_session_balance* made = nullptr;
  R0H_TRY(r0h_session_balance_new(ctx, s->c->blob.data(), s->c->blob.size(), &made));
  std::unique_ptr<r0h_session_balance, SessionBalanceFree> sb(made);
  bool own_proof = false;  // a proof of the caller's context is still to be finished: it closes the profile
  R0H_TRY(add_pending_segments(s, sb.get(), &own_proof));
  R0H_TRY(r0h_session_balance_add_verifier_side(sb.get(), s->elf.data(), s->elf.size(), s->journal.data(), s->journal.size()));
  char* text = nullptr;
  R0H_TRY(r0h_session_balance_message(sb.get(), &text));
  if (!own_proof || text) r0h_free_error(profile_close(ctx));
  if (!text) return nullptr;
  for (Pending& p : s->pending) p.proof.reset();  // aborted
  const char* err = make_error("r0h_prove_elf: %s", text);
  r0h_free_error(text);
  return err;
}
// Phase 2 of a segment: the challenge and the segment's own sum under it become its late public inputs, and the proof is finished.
// The DATA block goes back to the pool whether or not the proof succeeds.
const char* finish_segment(r0h_session* s, Pending& p, const uint32_t challenge[16], std::vector<uint32_t>& mix, std::vector<uint32_t>& seal, size_t* words) {
  const r0h_circuit* c = s->c;
  DevBuf data = std::move(p.data);
  memcpy(p.global.data() + R0H_TRACE_GAMMA, challenge, 64);
  const r0h_buf* code_cols = nullptr;
  R0H_TRY(r0h_code_commit_columns(p.cc, &code_cols));
  LogupKept kept;  // the session accumulator's scanned terms: evaluated once, for its total here and for its ACCUM columns below
  R0H_TRY(logup_totals_keep(p.lctx, c, p.po2, code_cols, data.get(), p.global.data(), &kept));
  R0H_TRY(r0h_proof_late(p.proof.get(), p.global.data() + (R0H_TRACE_GLOBALS - R0H_TRACE_LATE_GLOBALS), mix.data()));
  DevBuf accum;
  R0H_TRY(accum.alloc(p.lctx, ((size_t)c->group_size[R0H_GROUP_ACCUM] << p.po2) * 4));
  R0H_TRY(logup_accum_kept(p.lctx, c, p.po2, code_cols, data.get(), p.global.data(), mix.data(), accum.get(), &kept));
  kept.terms.reset();
  return r0h_proof_finish(p.proof.release(), accum.get(), seal.data(), seal.size(), words);  // consumed either way
}
// Phase 2 of an evicted segment, before it is finished: committed again from its rows, on its lane, to the root it was recorded with.
// A replayed commitment continues the profile of the lane's context (the session check's phase is in it) instead of opening one.
const char* replay_segment(r0h_session* s, Pending& p) {
  const Clock::time_point t0 = Clock::now();
  R0H_TRY(p.data.alloc(p.lctx, ((size_t)s->c->group_size[R0H_GROUP_DATA] << p.po2) * 4));
  uint32_t root[8];
  Clock::time_point t1;
  p.lctx->prof.continued = true;
  const char* err = commit_rows(s->c, p, p.data.get(), p.global.data(), root, &t1, s->device.tops_levels);
  p.lctx->prof.continued = false;
  R0H_TRY(err);
  // (from a kept top the root is the top's, held against the recorded one when it was kept: what ties the rows to it is the subtree
  // check of the proof's openings)
  R0H_REQUIRE(!memcmp(root, p.root, 32), "r0h_session_finish: segment %zu committed another root when it was replayed", p.index);
  p.evicted = false;
  p.rows.reset();  // (the commitment has waited for the stream)
  const uint64_t top_bytes = p.top ? p.top->bytes : 0;
  p.top.reset();  // (the proof has its own copy)
  p.held.set(s->ctx, p.data->bytes + r0h_proof_resident_bytes(p.proof.get()));
  std::lock_guard<std::mutex> lk(s->result_mu);
  s->device.replayed++;
  if (top_bytes) s->device.replayed_from_top++;
  s->device.tops_held -= top_bytes;
  s->device.rows_held -= p.rows_bytes;
  s->stats.witgen_ms += 1e3 * seconds(t0, t1);
  s->stats.prove_ms += 1e3 * seconds(t1, Clock::now());
  return nullptr;
}

// Phase 2 of an evicted segment under r0h_ctx_set_session_enqueue_begin: committed again from its rows without a wait.  The root it
// commits and the multiplicity kernels' error word go to `check`, which collect_segment reads back behind the seal and holds against
// the recorded root.
const char* replay_enqueued(r0h_session* s, Pending& p, DevBuf& check) {
  const Clock::time_point t0 = Clock::now();
  R0H_TRY(p.data.alloc(p.lctx, ((size_t)s->c->group_size[R0H_GROUP_DATA] << p.po2) * 4));
  R0H_TRY(check.alloc(p.lctx, GATHER_WORDS * 4));
  p.lctx->prof.continued = true;
  const char* err = [&]() -> const char* {
    R0H_TRY(r0h_trace_rows_expand(p.rows.get(), p.data.get()));
    R0H_TRY(logup_multiplicities_enqueue(p.lctx, s->c, p.po2, p.data.get(), p.global.data(), check.get(), 8));
    r0h_proof* proof = nullptr;
    if (p.top) R0H_TRY(r0h_proof_begin_committed_top_enqueue(p.lctx, s->c, p.po2, p.cc, p.data.get(), p.global.data(), p.top.get(), s->device.tops_levels, nullptr, &proof));
    else R0H_TRY(r0h_proof_begin_committed_enqueue(p.lctx, s->c, p.po2, p.cc, p.data.get(), p.global.data(), nullptr, &proof));
    p.proof.reset(proof);
    return r0h_proof_data_root_device(proof, check.get(), 0);
  }();
  p.lctx->prof.continued = false;
  R0H_TRY(err);
  p.evicted = false;
  p.rows.reset();  // (back to the lane's pool in stream order, behind the expansion)
  const uint64_t top_bytes = p.top ? p.top->bytes : 0;
  p.top.reset();   // (the proof has its own copy)
  p.held.set(s->ctx, p.data->bytes + r0h_proof_resident_bytes(p.proof.get()));
  std::lock_guard<std::mutex> lk(s->result_mu);
  s->device.replayed++;
  if (top_bytes) s->device.replayed_from_top++;
  s->device.tops_held -= top_bytes;
  s->device.rows_held -= p.rows_bytes;
  s->stats.prove_ms += 1e3 * seconds(t0, Clock::now());
  return nullptr;
}

// ---- phase 2 from one host thread (r0h_ctx_set_session_enqueue).  Once the challenge exists nothing a segment needs comes from the host:
// its public inputs go up once, the session sum is left in their device copy (logup_totals_keep_device), the device generator absorbs
// the late inputs and draws the mix (r0h_proof_late_device), the accumulation reads both where they are (logup_accum_kept_device) and
// the finish is enqueued.  What the enqueued steps read stays with the segment's InFlight until it is collected.
struct InFlight {
  Pending* p = nullptr;
  DevBuf check;  // of a segment replayed without a wait (replay_enqueued): its root and the multiplicity kernels' error word, read back behind the collect
  DevBuf data, globals, mix, accum;
  Clock::time_point t0;
};
const char* enqueue_segment(r0h_session* s, Pending& p, const uint32_t challenge[16], InFlight& fl) {
  const r0h_circuit* c = s->c;
  r0h_ctx* lctx = p.lctx;
  const uint32_t n_early = R0H_TRACE_GLOBALS - R0H_TRACE_LATE_GLOBALS;
  fl.p = &p;
  fl.t0 = Clock::now();
  fl.data = std::move(p.data);
  memcpy(p.global.data() + R0H_TRACE_GAMMA, challenge, 64);
  const r0h_buf* code_cols = nullptr;
  R0H_TRY(r0h_code_commit_columns(p.cc, &code_cols));
  R0H_TRY(fl.globals.alloc(lctx, (size_t)c->n_global * 4));
  R0H_TRY(stage_h2d(lctx, fl.globals->ptr, p.global.data(), (size_t)c->n_global * 4));
  LogupKept kept;
  R0H_TRY(logup_totals_keep_device(lctx, c, p.po2, code_cols, fl.data.get(), fl.globals.get(), &kept));
  R0H_TRY(fl.mix.alloc(lctx, (size_t)(c->n_mix ? c->n_mix : 1) * 4));
  const r0h_buf late = buf_view(fl.globals.get(), (size_t)n_early * 4, (size_t)R0H_TRACE_LATE_GLOBALS * 4);
  R0H_TRY(r0h_proof_late_device(p.proof.get(), &late, fl.mix.get()));
  R0H_TRY(fl.accum.alloc(lctx, ((size_t)c->group_size[R0H_GROUP_ACCUM] << p.po2) * 4));
  R0H_TRY(logup_accum_kept_device(lctx, c, p.po2, code_cols, fl.data.get(), fl.globals.get(), fl.mix.get(), fl.accum.get(), &kept));
  kept.terms.reset();  // (back to the lane's pool behind the launches that read it)
  const char* err = r0h_proof_finish_enqueue(p.proof.get(), fl.accum.get());
  if (err) (void)p.proof.release();  // consumed by the failed enqueue
  return err;
}
// the read-back of an enqueued segment, its seal and the session's accounting; the buffers go back to the lane's pool behind the proof
const char* collect_segment(r0h_session* s, InFlight& fl, std::vector<uint32_t>& seal) {
  Pending& p = *fl.p;
  size_t words = 0;
  const char* err = r0h_proof_finish_collect(p.proof.release(), seal.data(), seal.size(), &words);  // consumed either way: the stream has drained
  if (!err && fl.check) {  // a segment replayed without a wait: what it committed is looked at now
    uint32_t got[GATHER_WORDS];
    err = r0h_buf_d2h(p.lctx, fl.check.get(), 0, got, sizeof got);
    if (!err) err = logup_multiplicities_verdict(got[8]);
    if (!err && memcmp(got, p.root, 32)) err = make_error("r0h_session_finish: segment %zu committed another root when it was replayed", p.index);
  }
  fl = InFlight();
  if (p.rows) {
    p.rows.reset();
    std::lock_guard<std::mutex> lk(s->result_mu);
    s->device.rows_held -= p.rows_bytes;
  }
  p.held.set(nullptr, 0);
  R0H_TRY(err);
  std::lock_guard<std::mutex> lk(s->result_mu);
  p.seal.assign(seal.begin(), seal.begin() + words);
  p.done = true;
  return nullptr;
}
uint64_t lane_ring_waits(const r0h_session* s) {
  uint64_t n = 0;
  for (const r0h_ctx* l : s->lane_ctx) n += l->ring_waits.load();
  return n;
}
// The calling thread drives every lane's stream.  Phase 1 dealt the segments to the lanes as they came, so every lane context has a
// queue of its own (in index order), and the thread goes round the lanes that still have one: on each it collects the segment that lane
// has in flight -- the oldest enqueue of all, since every other lane was served after it -- and enqueues the lane's next.  A lane context
// has at most one segment in flight (the ACCUM group and the finish temporaries of one segment per lane, what the blocking form holds
// too; and a lane's 8 MiB pinned staging ring is never asked for more than one segment's tables between two collects), and while one
// lane is being collected the others' streams have their segment to run.  After the first round -- every lane that holds a segment has
// had its first enqueue -- the image proof is made; when no lane has anything left to enqueue, what is still in flight is collected,
// oldest first.  An error ends the rounds: what is in flight is collected, then every other proof is aborted.
const char* finish_enqueued(r0h_session* s, const uint32_t challenge[16], std::vector<uint32_t>& image_seal, uint64_t* other_waits, uint64_t* off_lane_waits) {
  struct Lane { r0h_ctx* ctx; std::deque<Pending*> todo; InFlight flying; };
  std::vector<Lane> lanes;  // in the order of their first segment
  for (Pending& p : s->pending) {
    if (p.done) continue;
    auto it = std::find_if(lanes.begin(), lanes.end(), [&](const Lane& l) { return l.ctx == p.lctx; });
    if (it == lanes.end()) { lanes.push_back(Lane{p.lctx, {}, InFlight()}); it = lanes.end() - 1; }
    it->todo.push_back(&p);
  }
  std::vector<uint32_t> seal((size_t)1 << 20);
  std::deque<Lane*> order;  // lanes with a segment in flight, oldest first
  const char* first = nullptr;
  auto note = [&](const char* err) {  // the first error is the session's; later ones are dropped
    if (!err) return;
    if (first) r0h_free_error(err);
    else first = err;
  };
  auto collect = [&](Lane& l) {
    const Clock::time_point t0 = l.flying.t0;
    if (l.flying.check) *other_waits += 1;  // a replayed segment's root comes home behind its seal
    const char* err = collect_segment(s, l.flying, seal);
    order.erase(std::find(order.begin(), order.end(), &l));
    if (!err) {
      std::lock_guard<std::mutex> lk(s->result_mu);
      s->stats.prove_ms += 1e3 * seconds(t0, Clock::now());  // enqueue to collected
      s->stats.segments++;
    }
    note(err);
  };
  // the blocking r0h_prove_image on the session's own context, whose stream and per-phase profile must be its alone meanwhile (a context
  // reports one proof at a time): what flies there is collected first; the other lanes' segments run beside it
  auto prove_image = [&]() {
    for (Lane& l : lanes)
      if (l.ctx == s->ctx && l.flying.p) collect(l);
    if (first) return;
    const uint64_t w0 = lane_waits(s);
    size_t words = 0;
    const char* err = r0h_prove_image(s->ctx, s->ctx->image_circuit, s->elf.data(), s->elf.size(), challenge, seal.data(), seal.size(), &words);
    *other_waits += lane_waits(s) - w0;
    if (!err) image_seal.assign(seal.begin(), seal.begin() + words);
    note(err);
  };
  bool image_due = !s->elf.empty() && s->ctx->image_circuit;
  // r0h_ctx_set_session_enqueue_begin: the image proof is enqueued now that the challenge exists, on a helper context of its own -- a
  // context reports one proof at a time, and every lane's context has segments to report -- and collected behind the last segment
  r0h_image_proof* image_flying = nullptr;
  r0h_ctx* image_ctx = nullptr;
  bool image_ctx_finish = false;
  uint64_t image_waits0 = 0;
  if (image_due && s->enqueue_begin) {
    image_due = false;
    const char* err = ctx_helper(s->ctx, s->lane_ctx.size() - 1, &image_ctx);
    if (!err) {
      image_ctx_finish = image_ctx->device_finish;
      image_ctx->device_finish = true;
      image_waits0 = image_ctx->blocking_waits.load();
      err = r0h_prove_image_enqueue(image_ctx, s->ctx->image_circuit, s->elf.data(), s->elf.size(), challenge, &image_flying);
    }
    note(err);
  }
  for (bool any = true; any && !first;) {
    any = false;
    for (Lane& l : lanes) {
      if (first) break;
      if (l.todo.empty()) continue;
      any = true;
      if (l.flying.p) collect(l);
      if (first) break;
      Pending& p = *l.todo.front();
      l.todo.pop_front();
      if (p.evicted && s->enqueue_begin) {  // enqueued: its root is compared behind its collect (one read-back there)
        note(replay_enqueued(s, p, l.flying.check));
        if (first) { p.proof.reset(); l.flying = InFlight(); break; }
      } else if (p.evicted) {  // blocking, as in the lanes' form: its root comes to the host to be compared
        const uint64_t w0 = lane_waits(s);
        note(replay_segment(s, p));
        *other_waits += lane_waits(s) - w0;
        if (first) break;
      }
      const char* err = enqueue_segment(s, p, challenge, l.flying);
      if (err) {  // the proof is aborted first (it waits for what the enqueue had launched), then its buffers go
        p.proof.reset();
        l.flying = InFlight();
        note(err);
        break;
      }
      order.push_back(&l);
    }
    if (image_due && !first) {
      image_due = false;
      prove_image();
    }
  }
  while (!order.empty()) collect(*order.front());  // after an error too: what is in flight is collected, its seal kept or its error dropped
  if (image_flying) {
    size_t words = 0;
    const char* err = first ? r0h_prove_image_abort(image_flying) : r0h_prove_image_collect(image_flying, seal.data(), seal.size(), &words);
    if (!err && !first) image_seal.assign(seal.begin(), seal.begin() + words);
    note(err);
  }
  if (image_ctx) {
    *off_lane_waits = image_ctx->blocking_waits.load() - image_waits0;  // (no lane's context: counted beside the lanes')
    *other_waits += *off_lane_waits;
    image_ctx->device_finish = image_ctx_finish;
  }
  if (first)
    for (Pending& p : s->pending) {  // the others' proofs are aborted, and what they held goes with them
      if (p.done) continue;
      p.proof.reset();
      p.data.reset();
      std::lock_guard<std::mutex> lk(s->result_mu);
      if (p.rows) s->device.rows_held -= p.rows_bytes;
      if (p.top) s->device.tops_held -= p.top->bytes;
      p.rows.reset();
      p.top.reset();
      p.held.set(nullptr, 0);
    }
  return first;
}
}  // namespace

// Phase 2: with the records of ALL segments of the session (in index order) the challenge is fixed; every proof of this rank receives
// it and its own sum under it as late public inputs and is finished.  The receipt holds this rank's segments.
const char* r0h_session_finish(r0h_session* s, const uint32_t* all_records, size_t n_records, r0h_receipt** receipt_out, uint8_t image_id_out[32], uint64_t* cycles_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(s && receipt_out, "r0h_session_finish: NULL argument");
  std::vector<uint32_t> image_seal;
  if (s->trace_mode) {
    R0H_REQUIRE(all_records && n_records == s->n_segments, "r0h_session_finish: the session has %zu segments, %zu records were given", s->n_segments, n_records);
    const uint32_t n_early = R0H_TRACE_GLOBALS - R0H_TRACE_LATE_GLOBALS;
    for (const Pending& p : s->pending)
      R0H_REQUIRE(!memcmp(all_records + p.index * RECORD_WORDS, p.global.data(), n_early * 4) && !memcmp(all_records + p.index * RECORD_WORDS + n_early, p.root, 32),
                  "r0h_session_finish: record %zu is not the one this rank committed", p.index);
    if (s->check_session) R0H_TRY(check_session(s));
    uint32_t challenge[16];
    session_challenge(all_records, n_records, challenge);
    const uint64_t waits0 = lane_waits(s), ring0 = lane_ring_waits(s);
    uint64_t other_waits = 0;
    if (s->enqueue) {
      // the lanes' contexts finish on the device generator for the length of the phase, whatever their switch says
      std::vector<bool> was;
      for (r0h_ctx* l : s->lane_ctx) { was.push_back(l->device_finish); l->device_finish = true; }
      uint64_t off_lane_waits = 0;
      const char* err = finish_enqueued(s, challenge, image_seal, &other_waits, &off_lane_waits);
      for (size_t k = 0; k < s->lane_ctx.size(); k++) s->lane_ctx[k]->device_finish = was[k];
      const uint64_t phase2[4] = {1, lane_waits(s) - waits0 + off_lane_waits, lane_ring_waits(s) - ring0, other_waits};  // (with the waits of the image proof's helper context)
      memcpy(s->ctx->session_phase2, phase2, sizeof phase2);
      R0H_TRY(err);
    }
    std::atomic<bool> failed(false);  // a lane's error: the others leave before their next segment
    auto lane = [&](r0h_ctx* lctx) -> const char* {
      std::vector<uint32_t> seal((size_t)1 << 20), mix(s->c->n_mix);
      size_t words = 0;
      if (lctx == s->ctx && !s->elf.empty() && s->ctx->image_circuit) {
        // the image's side of the balance, proved (`receipt.verify(image_id)` then needs no ELF): first thing on the first lane, beside
        // the other lanes' segments -- all it waits for is the challenge
        R0H_TRY(r0h_prove_image(s->ctx, s->ctx->image_circuit, s->elf.data(), s->elf.size(), challenge, seal.data(), seal.size(), &words));
        image_seal.assign(seal.begin(), seal.begin() + words);
      }
      for (Pending& p : s->pending) {
        if (p.lctx != lctx || p.done) continue;
        if (failed) return nullptr;
        if (p.evicted) R0H_TRY(replay_segment(s, p));  // one at a time: finished before the lane's next one is committed again
        const Clock::time_point t0 = Clock::now();
        R0H_TRY(finish_segment(s, p, challenge, mix, seal, &words));
        if (p.rows) {  // a segment that stayed committed: its rows were not needed
          p.rows.reset();
          std::lock_guard<std::mutex> lk(s->result_mu);
          s->device.rows_held -= p.rows_bytes;
        }
        p.held.set(nullptr, 0);  // (witness and proof went with finish_segment)
        std::lock_guard<std::mutex> lk(s->result_mu);
        p.seal.assign(seal.begin(), seal.begin() + words);
        p.done = true;
        s->stats.prove_ms += 1e3 * seconds(t0, Clock::now());
        s->stats.segments++;
      }
      return nullptr;
    };
    if (!s->enqueue) {
      R0H_TRY(run_lanes(s->lane_ctx, lane, [&] { failed = true; }));
      const uint64_t phase2[4] = {s->lane_ctx.size(), lane_waits(s) - waits0, lane_ring_waits(s) - ring0, 0};
      memcpy(s->ctx->session_phase2, phase2, sizeof phase2);
    }
  }
  r0h_receipt* rc = nullptr;
  R0H_TRY(r0h_receipt_new(R0H_RECEIPT_COMPOSITE, nullptr, 0, &rc));
  std::unique_ptr<r0h_receipt, const char* (*)(r0h_receipt*)> rc_guard(rc, r0h_receipt_free);
  for (Pending& p : s->pending) {
    R0H_REQUIRE(p.done, "r0h_prove_elf: segment %zu was never proved", p.index);
    R0H_TRY(r0h_receipt_add_segment_claim(rc, p.seal.data(), p.seal.size(), (uint32_t)p.index, &p.claim, nullptr));
  }
  rc->journal = s->journal;
  rc->image_seal = image_seal;
  if (image_id_out) memcpy(image_id_out, s->image_id, 32);
  if (cycles_out) *cycles_out = s->cycles;
  s->stats.wall_s = seconds(s->t_begin, Clock::now());
  s->ctx->session = s->stats;
  const uint64_t device[4] = {s->device.evicted, s->device.replayed, s->device.counted_peak, s->device.rows_peak};
  memcpy(s->ctx->session_device, device, sizeof device);
  const uint64_t tops[3] = {s->device.replayed_from_top, s->device.tops_peak, s->device.tops_levels};
  memcpy(s->ctx->session_tops, tops, sizeof tops);
  *receipt_out = rc_guard.release();
  return nullptr;
  R0H_GUARD_END
}

// A rank's share of the gathered session balance (include/r0hip.h): the pending segments' additions and nothing else.
const char* r0h_session_balance_add_session(r0h_session_balance* sb, r0h_session* s) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(sb && s, "r0h_session_balance_add_session: NULL argument");
  R0H_REQUIRE(s->trace_mode, "r0h_session_balance_add_session: the session's circuit is not the trace circuit: its segments are proved at once and share no sum");
  R0H_REQUIRE(sb->ctx, "r0h_session_balance_add_session: this handle was made without a context: a session's witnesses are on the device");
  for (const Pending& p : s->pending)
    R0H_REQUIRE(!p.done && (p.evicted ? (bool)p.rows : (bool)p.data), "r0h_session_balance_add_session: segment %zu is finished: a session is added between r0h_session_begin and r0h_session_finish", p.index);
  bool own_proof = false;
  return add_pending_segments(s, sb, &own_proof);
  R0H_GUARD_END
}

const char* r0h_session_journal(const r0h_session* s, const uint8_t** bytes, size_t* n) {
  R0H_REQUIRE(s && bytes && n, "r0h_session_journal: NULL argument");
  *bytes = s->journal.data();
  *n = s->journal.size();
  return nullptr;
}

// both phases on one rank: the records this rank contributes are all there are
static const char* prove_session(r0h_ctx* ctx, const r0h_circuit* c, const uint8_t* elf, size_t elf_len, const uint32_t* input_words, size_t n_input, uint32_t segment_po2,
                                 uint64_t max_cycles, uint32_t part, uint32_t parts, r0h_receipt** receipt_out, uint8_t image_id_out[32], uint64_t* cycles_out) {
  r0h_session* s = nullptr;
  R0H_TRY(r0h_session_begin(ctx, c, elf, elf_len, input_words, n_input, segment_po2, max_cycles, part, parts, &s));
  std::unique_ptr<r0h_session> guard(s);
  std::vector<uint32_t> indices(s->pending.size() + 1), records((s->pending.size() + 1) * RECORD_WORDS);
  size_t n = 0;
  R0H_TRY(r0h_session_records(s, indices.data(), records.data(), s->pending.size(), &n));
  return r0h_session_finish(s, records.data(), n, receipt_out, image_id_out, cycles_out);
}

const char* r0h_prove_elf(r0h_ctx* ctx, const r0h_circuit* c, const uint8_t* elf, size_t elf_len, const uint32_t* input_words, size_t n_input, uint32_t segment_po2,
                          uint64_t max_cycles, r0h_receipt** receipt_out, uint8_t image_id_out[32], uint64_t* cycles_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(receipt_out, "r0h_prove_elf: NULL argument");
  return prove_session(ctx, c, elf, elf_len, input_words, n_input, segment_po2, max_cycles, 0, 1, receipt_out, image_id_out, cycles_out);
  R0H_GUARD_END
}

// One rank's share of a session whose circuit has no session-wide argument (the synthetic circuits: segments are independent);
// with the trace circuit the ranks exchange their records between the phases: r0h_session_begin / _records / _finish.
const char* r0h_prove_elf_part(r0h_ctx* ctx, const r0h_circuit* c, const uint8_t* elf, size_t elf_len, const uint32_t* input_words, size_t n_input, uint32_t segment_po2,
                               uint64_t max_cycles, uint32_t part, uint32_t parts, r0h_receipt** receipt_out, uint8_t image_id_out[32], uint64_t* cycles_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(receipt_out && c, "r0h_prove_elf_part: NULL argument");
  R0H_REQUIRE(parts == 1 || c->n_late == 0, "r0h_prove_elf_part: the segments of a trace-circuit session share one challenge: ranks use r0h_session_begin / r0h_session_records / r0h_session_finish");
  return prove_session(ctx, c, elf, elf_len, input_words, n_input, segment_po2, max_cycles, part, parts, receipt_out, image_id_out, cycles_out);
  R0H_GUARD_END
}

}  // extern "C"
