// lift + join behind the C ABI (risc0-zkvm 3.0.5 `ProverServer::{lift, join}` over
// risc0-circuit-recursion 4.0.4, Cargo.lock:3050-3085): `lift` turns a segment receipt into a recursion-circuit proof, `join` folds
// two of them into one whose claim is the composition of theirs -- {pre: a.pre, post: b.post, exit_code: b.exit_code,
// input: a.input, output: b.output}, refused unless a ends in SystemSplit exactly where b starts -- and the folds form the binary tree
// whose levels are the one inter-GPU exchange of the whole path (hyperfridge-r0_amd/recursion.py moves the nodes; nothing else).
//
// What a node's proof is, stated plainly: one STARK over the recursion circuit of this repository (circuits/recursion.r0c) made with the
// same kernels as a segment proof, whose 16 public inputs are (a) the 8 words naming the node's composed ReceiptClaim
// (r0h_claim_globals) and (b) the Poseidon2 digest of what it consumed (the segment seal, or the two child seals' digests).  (b) is
// computed INSIDE the proof: the circuit's sponge component (tools/sponge_component.py, blob section SPONGE) hashes the consumed words,
// held in witness cells, one Poseidon2 round per row, and ties the result to those public inputs -- a node whose witness holds other
// words than its digest names has no satisfying trace.  That is the first in-circuit step and the only one: the children's SEALS are
// still verified BESIDE the proof -- host threads run the verifier while the device proves -- because risc0's recursion circuit (whose
// programs are downloaded at build time upstream) cannot be reproduced here; a root node is a checkable tree of seals with a composed
// claim, not a succinct receipt.  r0h_node_verify checks one node's seal, control root and naming words.
//
// What none of lift / join / node_verify checks is the SESSION argument of trace-circuit seals (numbers, closing rules, the common
// challenge, the balance of the sums with the image and the journal: csrc/claim.cpp session_verdict).  A node therefore carries its
// leaves' session parts (R0H_NODE_SESSION_WORDS each, taken by lift from the seal it verified, concatenated by join) beside its claim,
// and r0h_root_verify_session_elf / _image (claim.cpp) hold a root to them.  r0h_compress is the whole tree in one call: a queue of
// lifts and joins taken by up to four prover lanes of the device, refusing a receipt that fails the image-free session checks first.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "circuit.hpp"
#include "receipt_types.hpp"

using namespace r0h;

struct r0h_recursor {
  r0h_ctx* ctx = nullptr;
  r0h_circuit* circuit = nullptr;          // the recursion-shaped circuit, loaded on ctx
  r0h_code_commit* code = nullptr;         // its CODE group at `po2`, committed once
  uint32_t po2 = 0;
  uint32_t root[8] = {0};                  // control root of the recursion circuit at po2
  std::vector<uint32_t> recursion_blob, segment_blob;
  std::vector<uint32_t> segment_roots;     // n records of 9 words [po2, root[8]]: control roots of the segment circuit
  bool verify_on_device = false;           // r0h_recursor_set_verify_on_device: consumed seals are verified as a batch on the lane's context
};

namespace {
bool same_state(const r0h_system_state& a, const r0h_system_state& b) {
  uint8_t da[32], db[32];
  system_state_digest(a, da);
  system_state_digest(b, db);
  return !memcmp(da, db, 32);
}

void naming_words(const r0h_receipt_claim& claim, uint32_t out[8]) {
  uint8_t cd[32];
  claim_digest(claim, cd);
  claim_globals(cd, out);
}

// one recursion-circuit proof with the given 16 public inputs, on `ctx` -- the recursor's context or a helper lane of it (r0h_compress:
// the lanes share the loaded circuit and its CODE commitment) -- while `checks` run on host threads.  `states`: what the sponge chain
// over the consumed words starts every permutation from (p2_sponge_chain_host); the rows are expanded on the device (sponge.hip)
const char* prove_node(r0h_recursor* rc, r0h_ctx* ctx, const uint32_t publics[16], const std::vector<uint32_t>& states, std::vector<uint32_t>& seal) {
  const size_t n = (size_t)1 << rc->po2;
  DevBuf data, code;  // (freed in the reverse order: CODE first)
  R0H_TRY(code.alloc(ctx, (size_t)rc->circuit->group_size[R0H_GROUP_CODE] * n * 4));
  R0H_TRY(data.alloc(ctx, (size_t)rc->circuit->group_size[R0H_GROUP_DATA] * n * 4));
  // the rest of the witness is the circuit's synthetic column program: any deterministic seed
  const uint64_t seed = (uint64_t)publics[0] | (uint64_t)publics[8] << 32;
  R0H_TRY(r0h_witgen_public(ctx, rc->circuit, rc->po2, seed, publics, code.get(), data.get()));
  // the sponge rows over what this node consumes: the digest the circuit computes from them is publics[8..16)
  R0H_TRY(sponge_plant_states(ctx, rc->circuit, rc->po2, states.data(), states.size() / P2_CELLS, data.get()));
  seal.resize((size_t)1 << 19);
  size_t words = 0;
  R0H_TRY(r0h_prove_segment_committed(ctx, rc->circuit, rc->po2, rc->code, data.get(), publics, seal.data(), seal.size(), &words));
  seal.resize(words);
  return nullptr;
}

struct Check {  // a seal this step consumes, verified on a host thread while the device proves
  const uint32_t* blob; size_t blob_words; const uint32_t* seal; size_t seal_words; const uint32_t* root; const char* what;
  int verdict = -1;
  const char* err = nullptr;
  uint32_t data_root[8] = {0};  // of the seal's DATA commitment, as its transcript recomputes it
  void run() { err = r0h_verify_seal_roots(blob, blob_words, seal, seal_words, root, &verdict, nullptr, data_root); }
};

// the checks as one batch of the collecting verifier on `ctx`: the openings of all of them hashed by one launch, every comparison and
// verdict the host's (verify.cpp verify_seals_batch).  Blocks; leaves in every check what run() leaves.
const char* run_checks_on(r0h_ctx* ctx, std::vector<Check>& checks) {
  std::vector<SealCheck> batch;
  for (const Check& c : checks) batch.push_back(SealCheck{c.blob, c.blob_words, c.seal, c.seal_words, c.root});
  R0H_TRY(verify_seals_batch(ctx, HASH_POSEIDON2, batch.data(), batch.size()));
  for (size_t i = 0; i < checks.size(); i++) {
    checks[i].err = batch[i].err;
    checks[i].verdict = batch[i].verdict;
    memcpy(checks[i].data_root, batch[i].data_root, 32);
  }
  return nullptr;
}

const char* prove_checked(r0h_recursor* rc, r0h_ctx* ctx, std::vector<Check>& checks, const uint32_t publics[16], const std::vector<uint32_t>& states,
                          std::vector<uint32_t>& seal) {
  std::vector<std::thread> threads;
  // on the device: the batch goes first, so that its one short launch does not wait behind the node's proof on the lane's stream
  if (rc->verify_on_device) R0H_TRY(run_checks_on(ctx, checks));
  else for (Check& c : checks) threads.emplace_back([&c] { c.run(); });
  const char* err = prove_node(rc, ctx, publics, states, seal);
  for (std::thread& t : threads) t.join();
  for (Check& c : checks) {
    if (c.err && !err) err = c.err;
    else if (c.err) r0h_free_error(c.err);
  }
  if (err) return err;
  for (Check& c : checks) R0H_REQUIRE(c.verdict == R0H_VERIFY_OK, "%s: the seal to be consumed does not verify: %s", c.what, r0h_verify_reason(c.verdict));
  return nullptr;
}

// the control root a segment seal of 2^po2 rows is verified against: nullptr when the recursor was given none at all
const char* segment_root(const r0h_recursor* rc, const char* caller, uint32_t po2, const uint32_t** root_out) {
  *root_out = nullptr;
  for (size_t k = 0; k < rc->segment_roots.size() / 9; k++)
    if (rc->segment_roots[9 * k] == po2) *root_out = rc->segment_roots.data() + 9 * k + 1;
  R0H_REQUIRE(*root_out || rc->segment_roots.empty(), "%s: no control root known for a segment of 2^%u rows", caller, po2);
  return nullptr;
}

// r0h_lift on `ctx`.  `verified_data_root`: the seal has been verified bound to its control root already and this is the root of its
// DATA commitment (r0h_compress verifies a receipt's seals before it proves anything); nullptr: verified beside the proof
const char* lift_on(r0h_recursor* rc, r0h_ctx* ctx, const uint32_t* seal, size_t seal_words, const r0h_receipt_claim* claim, const uint32_t* verified_data_root,
                    r0h_node** out) {
  r0h_circuit seg;
  R0H_TRY(parse_blob(&seg, rc->segment_blob.data(), rc->segment_blob.size()));
  R0H_REQUIRE(seal_words > (size_t)seg.n_global && seal[seg.n_global] < P, "r0h_lift: the segment seal is truncated");
  // `SegmentReceipt::verify_integrity`: the seal names the claim it is lifted for ...
  uint32_t publics[16];
  naming_words(*claim, publics);
  R0H_REQUIRE(!memcmp(publics, seal, 32), "r0h_lift: the segment seal's public inputs do not name this claim");
  // a trace-circuit seal also says where its run starts and stops and how it ends: the claim it is lifted under must say the same
  // (r0h_receipt_verify refuses a receipt otherwise; a root built from lifted nodes must not carry a claim that check would refuse)
  const bool trace = is_trace_circuit(seg);
  if (trace) R0H_REQUIRE(trace_seal_carries_claim(seal, *claim), "r0h_lift: the segment seal's first / last pc, way of ending or exit code are not this claim's");
  // ... and verifies against the control root of its trace size, when the recursor was given one (else against the circuit alone)
  const uint32_t* root = nullptr;
  R0H_TRY(segment_root(rc, "r0h_lift", dec(seal[seg.n_global]), &root));
  // one pass of the sponge chain over the seal: the digest among the public inputs, and what the planted rows start from
  for (size_t i = 0; i < seal_words; i++) R0H_REQUIRE(seal[i] < P, "r0h_seal_digest: word %zu is not a canonical field element", i);
  std::vector<uint32_t> states;
  p2_sponge_chain_host(p2_default(), seal, seal_words, publics + 8, &states);
  std::vector<Check> checks(verified_data_root ? 0 : 1);
  if (!verified_data_root) checks[0] = Check{rc->segment_blob.data(), rc->segment_blob.size(), seal, seal_words, root, "lift"};
  std::unique_ptr<r0h_node> node(new r0h_node());
  node->claim = *claim;
  R0H_TRY(prove_checked(rc, ctx, checks, publics, states, node->seal));
  if (trace) {  // the leaf's session part, from the seal that was just verified
    node->session.resize(R0H_NODE_SESSION_WORDS);
    session_part_of(seal, verified_data_root ? verified_data_root : checks[0].data_root, node->session.data());
  }
  *out = node.release();
  return nullptr;
}

const char* join_on(r0h_recursor* rc, r0h_ctx* ctx, const r0h_node* a, const r0h_node* b, r0h_node** out) {
  // risc0 `ReceiptClaim::join`: a must stop in a system split exactly where b starts.  One more case here: b is a node of closing rows
  // only (the trace circuit's session may end in segments without cycles: pre == post, SystemSplit, no output) -- it follows whatever
  // a ends in, the run's last segment included, and the composed claim ends the way a does
  static const uint8_t no_output[32] = {0};
  const bool b_idle = same_state(b->claim.pre, b->claim.post) && b->claim.exit_system == 2 && b->claim.exit_user == 0 && !memcmp(b->claim.output_digest, no_output, 32);
  R0H_REQUIRE(b_idle || (a->claim.exit_system == 2 && a->claim.exit_user == 0), "r0h_join: the left node does not end in SystemSplit: nothing can follow it");
  R0H_REQUIRE(same_state(a->claim.post, b->claim.pre), "r0h_join: the left node's post-state is not the right node's pre-state: these two do not follow one another");
  uint32_t names[16];
  for (int side = 0; side < 2; side++) {  // each child's seal names the claim it is carried with
    const r0h_node* nd = side ? b : a;
    R0H_REQUIRE(nd->seal.size() > 17, "r0h_join: a child seal is truncated");
    naming_words(nd->claim, names);
    R0H_REQUIRE(!memcmp(names, nd->seal.data(), 32), "r0h_join: the %s node's seal does not name the claim it is carried with", side ? "right" : "left");
  }
  std::unique_ptr<r0h_node> node(new r0h_node());
  node->claim = a->claim;             // pre, input from the left ...
  node->claim.post = b->claim.post;   // ... post, exit code, output from the right (a node of closing rows only leaves the left's)
  if (!(b_idle && a->claim.exit_system != 2)) {
    node->claim.exit_system = b->claim.exit_system;
    node->claim.exit_user = b->claim.exit_user;
    memcpy(node->claim.output_digest, b->claim.output_digest, 32);
  }
  // the leaves' session parts, left then right; a tree with a leaf that has none has none
  if (!a->session.empty() && !b->session.empty()) {
    node->session = a->session;
    node->session.insert(node->session.end(), b->session.begin(), b->session.end());
  }
  uint32_t publics[16], children[16];
  naming_words(node->claim, publics);
  R0H_TRY(r0h_seal_digest(a->seal.data(), a->seal.size(), children));
  R0H_TRY(r0h_seal_digest(b->seal.data(), b->seal.size(), children + 8));
  std::vector<uint32_t> states;  // the consumed words are the two digests: one permutation, its digest and its rows from one pass
  p2_sponge_chain_host(p2_default(), children, 16, publics + 8, &states);
  std::vector<Check> checks(2);
  checks[0] = Check{rc->recursion_blob.data(), rc->recursion_blob.size(), a->seal.data(), a->seal.size(), rc->root, "join (left)"};
  checks[1] = Check{rc->recursion_blob.data(), rc->recursion_blob.size(), b->seal.data(), b->seal.size(), rc->root, "join (right)"};
  R0H_TRY(prove_checked(rc, ctx, checks, publics, states, node->seal));
  *out = node.release();
  return nullptr;
}

// ---- r0h_compress: the whole tree as a queue of work.  A lift is ready at once, a join when both its children are done; the lanes
// take what is ready.  The shape is the level-by-level fold of neighbours with an odd last node carried up.
struct TreeTask {
  int left = -1, right = -1;  // tasks whose nodes a join consumes; a lift has none and names its segment instead
  size_t segment = 0;
  int parent = -1, waiting = 0;
  std::unique_ptr<r0h_node> node;
};
struct TreeQueue {
  std::mutex mu;
  std::condition_variable cv;
  std::deque<int> ready;
  size_t left_to_do = 0;
  bool stop = false;
};
}  // namespace

extern "C" {

const char* r0h_recursor_new(r0h_ctx* ctx, const uint32_t* recursion_blob, size_t recursion_words, const char* code_object_path, uint32_t po2,
                             const uint32_t* segment_blob, size_t segment_words, const uint32_t* segment_control_roots, size_t n_roots, r0h_recursor** out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && recursion_blob && segment_blob && out && (segment_control_roots || !n_roots), "r0h_recursor_new: NULL argument");
  R0H_REQUIRE(po2 >= 9 && po2 <= R0H_MAX_PO2, "r0h_recursor_new: po2 %u outside [9, %u]", po2, R0H_MAX_PO2);
  R0H_TRY(require_poseidon2(ctx, "r0h_recursor_new"));
  std::unique_ptr<r0h_recursor, const char* (*)(r0h_recursor*)> rc(new r0h_recursor(), r0h_recursor_free);
  rc->ctx = ctx; rc->po2 = po2;
  ctx_retain(ctx);
  rc->recursion_blob.assign(recursion_blob, recursion_blob + recursion_words);
  rc->segment_blob.assign(segment_blob, segment_blob + segment_words);
  rc->segment_roots.assign(segment_control_roots, segment_control_roots + 9 * n_roots);
  {
    r0h_circuit seg;  // the leaves' circuit is only ever handed to the verifier: parse it once to refuse a malformed blob early
    R0H_TRY(parse_blob(&seg, segment_blob, segment_words));
    R0H_REQUIRE(seg.n_global >= 8, "r0h_recursor_new: the segment circuit exposes %u public inputs, a claim needs 8", seg.n_global);
  }
  R0H_TRY(r0h_circuit_load(ctx, recursion_blob, recursion_words, code_object_path, &rc->circuit));
  R0H_REQUIRE(rc->circuit->n_global == 16 && rc->circuit->has_column_program, "r0h_recursor_new: a recursion circuit exposes 16 public inputs (claim words, digest of what it consumed) and carries a column program; this one has %u",
              rc->circuit->n_global);
  R0H_REQUIRE(rc->circuit->has_sponge && rc->circuit->sponge_global == 8, "r0h_recursor_new: a recursion circuit computes the digest of what a node consumed in-circuit (blob section SPONGE, public inputs 8..15); this one does not");
  R0H_TRY(code_commit_of(ctx, rc->circuit, po2, &rc->code));
  R0H_TRY(r0h_code_commit_root(rc->code, rc->root));
  *out = rc.release();
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_recursor_free(r0h_recursor* rc) {
  if (!rc) return nullptr;
  if (rc->code) r0h_code_commit_free(rc->code);
  if (rc->circuit) r0h_circuit_free(rc->circuit);
  r0h_ctx* ctx = rc->ctx;
  delete rc;
  if (ctx) ctx_release(ctx);
  return nullptr;
}

const char* r0h_recursor_set_verify_on_device(r0h_recursor* rc, int on) {
  R0H_REQUIRE(rc, "r0h_recursor_set_verify_on_device: NULL argument");
  rc->verify_on_device = on != 0;
  return nullptr;
}

const char* r0h_recursor_control_root(const r0h_recursor* rc, uint32_t root_out[8]) {
  R0H_REQUIRE(rc && root_out, "r0h_recursor_control_root: NULL argument");
  memcpy(root_out, rc->root, 32);
  return nullptr;
}

const char* r0h_lift(r0h_recursor* rc, const uint32_t* seal, size_t seal_words, const r0h_receipt_claim* claim, r0h_node** out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(rc && seal && claim && out, "r0h_lift: NULL argument");
  R0H_TRY(require_poseidon2(rc->ctx, "r0h_lift"));
  return lift_on(rc, rc->ctx, seal, seal_words, claim, nullptr, out);
  R0H_GUARD_END
}

const char* r0h_join(r0h_recursor* rc, const r0h_node* a, const r0h_node* b, r0h_node** out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(rc && a && b && out, "r0h_join: NULL argument");
  R0H_TRY(require_poseidon2(rc->ctx, "r0h_join"));
  return join_on(rc, rc->ctx, a, b, out);
  R0H_GUARD_END
}

// risc0 `prover.compress(opts, &receipt)`: every segment lifted, the nodes joined into one root, on `lanes` prover lanes (1..4; 0: 2).
// Lane 0 is the recursor's context on the calling thread, the others are helper contexts of the same device on threads of their own
// (ctx_helper / run_lanes, as sessions use them); all share the loaded recursion circuit and its CODE commitment.  A node's seal depends
// only on its public inputs and what it consumed, so the root is the one the sequential fold of r0h_lift / r0h_join gives, word for
// word, whatever the lanes' order.  A trace-circuit receipt's seals are verified first, all of them, and the receipt is held to the
// ELF-free session checks (numbers, closing rules, the common challenge) before any proof is made; the balance needs the image and
// stays r0h_root_verify_session_*'s.  The first failure stops the queue; every lane has been joined when the error is returned.
const char* r0h_compress(r0h_recursor* rc, const r0h_receipt* receipt, uint32_t lanes, r0h_node** out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(rc && receipt && out, "r0h_compress: NULL argument");
  R0H_REQUIRE(lanes <= 4, "r0h_compress: %u lanes: 1 to 4 (0 selects 2)", lanes);
  if (!lanes) lanes = 2;
  R0H_TRY(require_poseidon2(rc->ctx, "r0h_compress"));
  R0H_REQUIRE(receipt->kind == R0H_RECEIPT_COMPOSITE && !receipt->segments.empty(), "r0h_compress: not a composite receipt: there are no segment seals to lift");
  const size_t n = receipt->segments.size();
  for (size_t i = 0; i < n; i++) {
    const r0h_receipt::Segment& g = receipt->segments[i];
    R0H_REQUIRE(g.has_claim, "r0h_compress: segment %zu carries no claim", i);
    R0H_REQUIRE(g.hashfn == "poseidon2", "r0h_compress: segment %zu names the hash function %s: nodes are Poseidon2 only", i, g.hashfn.c_str());
  }
  r0h_circuit seg;
  R0H_TRY(parse_blob(&seg, rc->segment_blob.data(), rc->segment_blob.size()));
  // a trace-circuit receipt: every seal verified bound to its control root (what r0h_lift would do beside its proof, done here on
  // up to three host threads per lane instead), which gives the DATA roots the session's challenge is derived from
  std::vector<uint32_t> data_roots;
  if (is_trace_circuit(seg)) {
    data_roots.resize(8 * n);
    std::vector<Check> checks(n);
    for (size_t i = 0; i < n; i++) {
      const std::vector<uint32_t>& sl = receipt->segments[i].seal;
      R0H_REQUIRE(sl.size() > (size_t)seg.n_global && sl[seg.n_global] < P, "r0h_lift: the segment seal is truncated");
      const uint32_t* root = nullptr;
      R0H_TRY(segment_root(rc, "r0h_lift", dec(sl[seg.n_global]), &root));
      checks[i] = Check{rc->segment_blob.data(), rc->segment_blob.size(), sl.data(), sl.size(), root, "lift"};
    }
    std::atomic<size_t> next(0);
    std::vector<std::thread> threads;
    if (rc->verify_on_device) R0H_TRY(run_checks_on(rc->ctx, checks));  // all leaves in one batch
    else for (size_t t = 0; t < std::min<size_t>(n, 3 * (size_t)lanes); t++)
      threads.emplace_back([&] { for (size_t i = next++; i < n; i = next++) checks[i].run(); });
    for (std::thread& t : threads) t.join();
    const char* err = nullptr;
    for (Check& c : checks) {
      if (c.err && !err) err = c.err;
      else if (c.err) r0h_free_error(c.err);
    }
    if (err) return err;
    std::vector<SessionLeaf> leaves(n);
    for (size_t i = 0; i < n; i++) {
      R0H_REQUIRE(checks[i].verdict == R0H_VERIFY_OK, "lift: the seal to be consumed does not verify: %s (segment %zu)", r0h_verify_reason(checks[i].verdict), i);
      memcpy(&data_roots[8 * i], checks[i].data_root, 32);
      const uint32_t* sl = receipt->segments[i].seal.data();
      leaves[i] = SessionLeaf{sl, &data_roots[8 * i], sl + R0H_TRACE_GAMMA, sl + R0H_TRACE_SUM};
    }
    size_t term = n - 1, leaf = 0;
    for (size_t i = 0; i < n; i++)
      if (receipt->segments[i].claim.exit_system <= 1) { term = i; break; }
    const int v = session_verdict(leaves, term, nullptr, &leaf);
    R0H_REQUIRE(v == R0H_RECEIPT_V_OK, "r0h_compress: segment %zu: %s", leaf, r0h_receipt_verify_reason(v));
  }
  // the tree: tasks [0, n) lift, the joins follow level by level
  std::vector<TreeTask> tasks(n);
  std::vector<int> level(n);
  for (size_t i = 0; i < n; i++) { tasks[i].segment = i; level[i] = (int)i; }
  while (level.size() > 1) {
    std::vector<int> up;
    for (size_t i = 0; i + 1 < level.size(); i += 2) {
      TreeTask t;
      t.left = level[i]; t.right = level[i + 1]; t.waiting = 2;
      tasks[t.left].parent = tasks[t.right].parent = (int)tasks.size();
      up.push_back((int)tasks.size());
      tasks.push_back(std::move(t));
    }
    if (level.size() & 1) up.push_back(level.back());
    level.swap(up);
  }
  TreeQueue q;
  q.left_to_do = tasks.size();
  for (size_t i = 0; i < n; i++) q.ready.push_back((int)i);
  std::vector<r0h_ctx*> lane_ctx(std::min<size_t>(lanes, tasks.size()), rc->ctx);
  for (size_t k = 1; k < lane_ctx.size(); k++) R0H_TRY(ctx_helper(rc->ctx, k - 1, &lane_ctx[k]));
  auto lane = [&](r0h_ctx* lctx) -> const char* {
    for (;;) {
      int id;
      {
        std::unique_lock<std::mutex> lk(q.mu);
        q.cv.wait(lk, [&] { return q.stop || !q.left_to_do || !q.ready.empty(); });
        if (q.stop || !q.left_to_do) return nullptr;
        id = q.ready.front();
        q.ready.pop_front();
      }
      TreeTask& t = tasks[id];
      r0h_node* made = nullptr;
      if (t.left < 0) {
        const r0h_receipt::Segment& g = receipt->segments[t.segment];
        R0H_TRY(lift_on(rc, lctx, g.seal.data(), g.seal.size(), &g.claim, data_roots.empty() ? nullptr : &data_roots[8 * t.segment], &made));
      } else {
        R0H_TRY(join_on(rc, lctx, tasks[t.left].node.get(), tasks[t.right].node.get(), &made));
      }
      std::lock_guard<std::mutex> lk(q.mu);
      t.node.reset(made);
      q.left_to_do--;
      if (t.parent >= 0 && --tasks[t.parent].waiting == 0) q.ready.push_back(t.parent);
      q.cv.notify_all();
    }
  };
  R0H_TRY(run_lanes(lane_ctx, lane, [&] { std::lock_guard<std::mutex> lk(q.mu); q.stop = true; q.cv.notify_all(); }));
  *out = tasks[level[0]].node.release();
  return nullptr;
  R0H_GUARD_END
}

// a node as it arrives from another rank: the seal and the claim it is carried with (checked when it is joined or verified)
const char* r0h_node_new(const uint32_t* seal, size_t seal_words, const r0h_receipt_claim* claim, r0h_node** out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(seal && claim && out, "r0h_node_new: NULL argument");
  std::unique_ptr<r0h_node> node(new r0h_node());
  node->seal.assign(seal, seal + seal_words);
  node->claim = *claim;
  *out = node.release();
  return nullptr;
  R0H_GUARD_END
}
// ... and with its leaves' session parts, as r0h_node_session gave them where it was made (n_leaves x R0H_NODE_SESSION_WORDS words).
// They travel beside the node as the claim does: r0h_root_verify_session_* reads them, nothing here checks them against the seal.
const char* r0h_node_new_with_session(const uint32_t* seal, size_t seal_words, const r0h_receipt_claim* claim, const uint32_t* session, size_t n_leaves, r0h_node** out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(seal && claim && out && (session || !n_leaves), "r0h_node_new_with_session: NULL argument");
  std::unique_ptr<r0h_node> node(new r0h_node());
  node->seal.assign(seal, seal + seal_words);
  node->claim = *claim;
  node->session.assign(session, session + n_leaves * R0H_NODE_SESSION_WORDS);
  *out = node.release();
  return nullptr;
  R0H_GUARD_END
}
const char* r0h_node_session(const r0h_node* node, const uint32_t** words, size_t* n_leaves) {
  R0H_REQUIRE(node && words && n_leaves, "r0h_node_session: NULL argument");
  *words = node->session.data();
  *n_leaves = node->session.size() / R0H_NODE_SESSION_WORDS;
  return nullptr;
}
const char* r0h_node_free(r0h_node* node) {
  delete node;
  return nullptr;
}
const char* r0h_node_seal(const r0h_node* node, const uint32_t** seal, size_t* seal_words) {
  R0H_REQUIRE(node && seal && seal_words, "r0h_node_seal: NULL argument");
  *seal = node->seal.data();
  *seal_words = node->seal.size();
  return nullptr;
}
const char* r0h_node_claim(const r0h_node* node, r0h_receipt_claim* claim_out) {
  R0H_REQUIRE(node && claim_out, "r0h_node_claim: NULL argument");
  *claim_out = node->claim;
  return nullptr;
}
// One node on its own: its seal verifies against the recursion circuit bound to `control_root` (NULL: unbound), and its first eight
// public inputs name the claim it is carried with.  *ok_out = 1 / 0; pure host code.  (What it consumed is vouched for by whoever
// made it: see the header of this file.)
const char* r0h_node_verify(const uint32_t* recursion_blob, size_t blob_words, const uint32_t* control_root, const r0h_node* node, int* ok_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(recursion_blob && node && ok_out, "r0h_node_verify: NULL argument");
  *ok_out = 0;
  int verdict = -1;
  R0H_TRY(r0h_verify_seal_bound(recursion_blob, blob_words, nullptr, nullptr, node->seal.data(), node->seal.size(), control_root, &verdict, nullptr, nullptr));
  if (verdict != R0H_VERIFY_OK || node->seal.size() < 16) return nullptr;
  uint32_t names[8];
  naming_words(node->claim, names);
  *ok_out = !memcmp(names, node->seal.data(), 32);
  return nullptr;
  R0H_GUARD_END
}

}  // extern "C"
