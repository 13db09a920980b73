// The segment-proof sequencer: owns the Fiat-Shamir transcript on the host and drives the device operations.
// Replaces risc0-circuit-rv32im 4.0.4 prove/hal/mod.rs (`SegmentProver::prove`: seed transcript, commit CODE and DATA,
// draw the accumulation mix, accumulate, finalize) and risc0-zkp 3.0.4 prove/{prover.rs, poly_group.rs, merkle.rs,
// fri.rs, write_iop.rs} + core/hash/{poseidon2,sha}/rng.rs behind the suite interface of hash_suite.cpp -- SURVEY.md 3.4 steps 3-13, 8(a) a8, a15-a17.
// This is what host/src/main.rs:423 (`prover.prove(env, HYPERFRIDGE_ELF)`) spends its time in, once per segment.
//
// One function per protocol step (proof_begin: steps 1-2; proof_steps: commit_accum, commit_check, evaluate_at_z, deep, fri_commit,
// queries), one owner per buffer, and one question every step asks: where does the transcript live?  It starts on the host (WriteIop)
// and may be handed over to the device generator (iop.hip; tail_open) at one of four places: before step 7
// (r0h_ctx_set_device_transcript), before step 3 (r0h_ctx_set_device_finish), before the late public inputs (r0h_proof_late_device)
// or before the DATA commitment (r0h_proof_begin_committed_enqueue: the first half of a proof waits for nothing either).
// After the hand-over `r0h_proof::iop` is set and the tail block exists, where the steps behind it leave their seal words for one
// read-back (tail_collect); before it neither does.  draw_ext, commit_tree and commit_words are the transcript in either place, so a
// step branches only where the two forms are different computations.  With the hand-over before step 3 nothing waits for the stream,
// and proof_finish splits into an enqueue and a collect that waits once.
//
// Device-resident throughout: witness, coefficients, evaluations, Merkle nodes, combos.  What crosses to the host per
// segment: Merkle tops + roots (<= 2 KB each), ~500 tap evaluations, the FRI final polynomial (4 KB) and the 50
// query openings (gathered on the device into one packed buffer per tree).  Upstream pulls the combos back to the
// host for the DEEP division; here the division is a device scan (r0h_poly_divide).
#include <memory>

#include "seal_layout.hpp"

namespace r0h {

// ------------------------------------------------------------------ transcript
// The generator and the slice hash are the context's hash suite (internal.hpp HashSuite: Poseidon2 or SHA-256); the order of
// commits, writes and draws below is the same under both.
struct WriteIop {
  std::vector<uint32_t> proof;
  std::unique_ptr<HashSuite> suite;
  std::unique_ptr<SuiteRng> rng_;
  SuiteRng& rng;
  WriteIop(int hashfn, const P2Consts* k) : suite(make_suite(hashfn, k)), rng_(suite->rng()), rng(*rng_) {}
  void write(const uint32_t* w, size_t n) { proof.insert(proof.end(), w, w + n); }
  void commit(const uint32_t digest[8]) { rng.mix(digest); }
  void commit_elems(const uint32_t* w, size_t n) {  // the suite's hash_elem_slice over words the seal carries (or a tag), then commit
    uint32_t d[8];
    suite->hash_elems(w, n, d);
    commit(d);
  }
};

// ------------------------------------------------------------------ Merkle
// The full form holds all 2 * rows nodes.  The top form (top_levels != 0: r0h_proof_begin_committed_top) holds digests
// [0, 2 * rows >> top_levels) only, and its openings hash the bottom top_levels levels again from the matrix (merkle_top.hip).
struct Tree {
  MerkleShape mp;
  DevBuf nodes;
  uint32_t top_levels = 0;
  const r0h_buf* matrix = nullptr;
  Tree(size_t rows, size_t cols) : mp(rows, cols) {}
};
// Nodes [1, 2 * top_size) of a built tree on the host, fetched in one blocking copy: the seal takes the top layer, the transcript the root
struct TreeTop {
  std::vector<uint32_t> nodes;  // node i at words [8i, 8i + 8)
  const uint32_t* root() const { return nodes.data() + 8; }
  void into(WriteIop& io) const {
    io.write(nodes.data() + nodes.size() / 2, nodes.size() / 2);
    io.commit(root());
  }
};

static const char* tree_build(r0h_ctx* ctx, Tree& t, const r0h_buf* matrix) {
  t.matrix = matrix;
  R0H_TRY(t.nodes.alloc(ctx, t.mp.rows * 2 * 32));
  return r0h_merkle_build(ctx, t.nodes.get(), matrix, (uint32_t)t.mp.rows, (uint32_t)t.mp.cols);
}
static const char* tree_top(r0h_ctx* ctx, const Tree& t, TreeTop& top) {
  top.nodes.assign(2 * t.mp.top_size * 8, 0u);
  return r0h_buf_d2h(ctx, t.nodes.get(), 32, top.nodes.data() + 8, (2 * t.mp.top_size - 1) * 32);
}
// The rows d_idx[0 .. n_q) opened into `out`, packed (device pointers): opened_words() words.  A tree in its top form reports in the
// last two of them whether every queried subtree hashed to the top's node (merkle_open_top_verdict reads them on the host).
static size_t opened_words(const Tree& t, uint32_t n_q) { return (size_t)n_q * t.mp.opening_words() + (t.top_levels ? 2 : 0); }
static const char* open_tree(r0h_ctx* ctx, const Tree& t, const uint32_t* d_idx, uint32_t n_q, uint32_t* out) {
  if (t.top_levels)
    return merkle_open_top(ctx, out, u32(t.matrix), u32(t.nodes.get()), t.top_levels, d_idx, n_q, (uint32_t)t.mp.rows, (uint32_t)t.mp.cols,
                           out + (size_t)n_q * t.mp.opening_words());
  return merkle_open(ctx, out, u32(t.matrix), u32(t.nodes.get()), d_idx, n_q, (uint32_t)t.mp.rows, (uint32_t)t.mp.cols);
}

// ------------------------------------------------------------------ poly groups
struct Group {
  DevBuf coeffs;     // bit-reversed, zk-shifted coefficients
  DevBuf evaluated;  // [count][4N]
  uint32_t count = 0;
  Tree tree;
  Group(uint32_t cnt, size_t domain) : count(cnt), tree(domain, cnt) {}
  size_t bytes() const {  // what it holds on the device
    size_t total = 0;
    for (const r0h_buf* b : {coeffs.get(), evaluated.get(), tree.nodes.get()}) total += b ? b->bytes : 0;
    return total;
  }
};
static const char* group_evaluate(r0h_ctx* ctx, Group& g, uint32_t po2) {
  R0H_TRY(g.evaluated.alloc(ctx, ((size_t)g.count << (po2 + 2)) * 4));
  g.tree.matrix = g.evaluated.get();
  return r0h_batch_expand_into_evaluate_ntt(ctx, g.evaluated.get(), g.coeffs.get(), g.count, po2, 2);
}
// A group up to its tree: witness columns -> bit-reversed, zk-shifted coefficients -> evaluations on 4N -> tree.  The tree stands in
// device memory; its top layer and root go to the seal and the transcript by commit_tree (below), or to a CODE commitment by tree_top.
// CHECK comes with its coefficients made by its own interpolation (witness == nullptr).
// With `kept_top` (levels != 0) no tree is built: the group's tree takes its top form from a copy of those digests.
static const char* group_build(r0h_ctx* ctx, Group& g, const r0h_buf* witness, uint32_t po2, const r0h_buf* kept_top = nullptr, uint32_t levels = 0) {
  if (witness) {
    const size_t bytes = ((size_t)g.count << po2) * 4;
    R0H_REQUIRE(bytes <= witness->bytes, "prove_segment: witness buffer holds fewer than %u columns of 2^%u", g.count, po2);
    R0H_TRY(g.coeffs.alloc(ctx, bytes));
    // out-of-place iNTT straight from the witness (no staging copy), zk shift fused into its last pass
    R0H_TRY(interpolate_ntt(ctx, g.coeffs.get(), witness, g.count, po2, true));
  }
  R0H_TRY(group_evaluate(ctx, g, po2));
  // upstream flips the coefficients to natural order here; the sequencer keeps them bit-reversed instead (evaluate-at-z
  // uses permuted power tables, the FRI mix is order-agnostic) and flips only the handful of mixed combos
  if (levels) {
    R0H_TRY(g.tree.nodes.alloc(ctx, ((g.tree.mp.rows * 2) >> levels) * 32));
    R0H_TRY(merkle_top_copy(ctx, kept_top, (uint32_t)g.tree.mp.rows, levels, g.tree.nodes.get(), "r0h_proof_begin_committed_top"));
    g.tree.top_levels = levels;
  } else {
    R0H_TRY(tree_build(ctx, g.tree, g.evaluated.get()));
  }
  return nullptr;
}

// Lagrange interpolation of a handful of extension points (host; a register has at most a few taps)
static void poly_interpolate(Fp4* out, const Fp4* xs, const Fp4* ys, uint32_t n) {
  std::vector<Fp4> acc(n, fp4_zero()), basis(n + 1);
  for (uint32_t i = 0; i < n; i++) {
    uint32_t deg = 0;
    basis[0] = fp4_one();
    Fp4 denom = fp4_one();
    for (uint32_t j = 0; j < n; j++) {
      if (j == i) continue;
      basis[deg + 1] = fp4_zero();
      for (uint32_t k = deg + 1; k-- > 0;) {
        basis[k + 1] = basis[k + 1] + basis[k];
        basis[k] = fp4_zero() - basis[k] * xs[j];
      }
      deg++;
      denom = denom * (xs[i] - xs[j]);
    }
    Fp4 s = ys[i] * fp4_inv(denom);
    for (uint32_t k = 0; k < n; k++) acc[k] = acc[k] + basis[k] * s;
  }
  for (uint32_t k = 0; k < n; k++) out[k] = acc[k];
}

// combos[row 0..size) of one combo -= cur * coeff_u (tiny host-driven fix-up of the first few coefficients)
__global__ void sub_head_kernel(uint32_t* __restrict__ combos, const uint32_t* __restrict__ fix /* (word index, value) pairs */, uint32_t n) {
  uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) combos[fix[2 * k]] = sub(combos[fix[2 * k]], fix[2 * k + 1]);
}

// ---- the small kernels of steps 5 and 6 under r0h_ctx_set_device_finish: what the host computes from z and the DEEP mix when it has
// them, computed where the device's transcript left them.  All latency-bound, a lane per item; extension words are read and written
// word by word, so no table needs more than word alignment.
__device__ __forceinline__ Fp4 ldw4(const uint32_t* p) { return Fp4{{p[0], p[1], p[2], p[3]}}; }
__device__ __forceinline__ void stw4(uint32_t* p, const Fp4& v) { p[0] = v.e[0]; p[1] = v.e[1]; p[2] = v.e[2]; p[3] = v.e[3]; }

// the point table: pts[i] = z * wpow[i] for the circuit's i-th distinct back (wpow[i] = omega^-back, host-known), pts[n_backs] = z^4
__global__ __launch_bounds__(64) void deep_points_kernel(uint32_t* __restrict__ pts, const uint32_t* __restrict__ z, const uint32_t* __restrict__ wpow, uint32_t n_backs) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  const Fp4 zz = ldw4(z);
  if (i < n_backs) stw4(pts + 4 * (size_t)i, scale(zz, wpow[i]));
  else if (i == n_backs) stw4(pts + 4 * (size_t)i, fp4_pow(zz, 4));
}

// poly_interpolate on the device, a register per lane: regs[3r ..) = (first tap, taps, first work slot).  Register r's taps t have
// x = pts[tap_pt[t]] and y = eval_u[t]; its interpolant goes to coeff_u[first tap ..).  M(x) = prod (x - x_j) is built once in the
// register's taps + 1 work slots; per tap i the quotient M / (x - x_i) comes from synthetic division, twice: once for its value at x_i
// (the Lagrange denominator), once to add it, scaled, into the interpolant.  Quadratic in the taps, and right for any count of them.
// The lanes behind the registers copy CHECK's sixteen openings.
__global__ __launch_bounds__(64) void interpolate_regs_kernel(uint32_t* __restrict__ coeff_u, const uint32_t* __restrict__ eval_u, const uint32_t* __restrict__ pts,
                                                               const uint32_t* __restrict__ tap_pt, const uint32_t* __restrict__ regs, uint32_t n_regs, uint32_t n_taps,
                                                               uint32_t* __restrict__ work) {
  const uint32_t r = blockIdx.x * 64 + threadIdx.x;
  if (r >= n_regs) {
    const uint32_t i = r - n_regs;
    if (i < R0H_CHECK_SIZE) stw4(coeff_u + 4 * (size_t)(n_taps + i), ldw4(eval_u + 4 * (size_t)(n_taps + i)));
    return;
  }
  const uint32_t first = regs[3 * r], n = regs[3 * r + 1];
  uint32_t* M = work + 4 * (size_t)regs[3 * r + 2];
  uint32_t* out = coeff_u + 4 * (size_t)first;
  auto x = [&](uint32_t j) { return ldw4(pts + 4 * (size_t)tap_pt[first + j]); };
  stw4(M, fp4_one());
  for (uint32_t j = 0; j < n; j++) {  // M <- M * (x - x_j); j is M's degree going in
    const Fp4 xj = x(j);
    stw4(M + 4 * (j + 1), fp4_zero());
    for (uint32_t k = j + 1; k-- > 0;) {
      const Fp4 m = ldw4(M + 4 * k);
      stw4(M + 4 * (k + 1), ldw4(M + 4 * (k + 1)) + m);
      stw4(M + 4 * k, fp4_zero() - m * xj);
    }
  }
  for (uint32_t k = 0; k < n; k++) stw4(out + 4 * k, fp4_zero());
  for (uint32_t i = 0; i < n; i++) {
    const Fp4 xi = x(i);
    // q = M / (x - x_i): q[n-1] = M[n], q[k-1] = M[k] + x_i q[k]; its value at x_i by Horner's rule over the same descent
    Fp4 q = ldw4(M + 4 * n), d = q;
    for (uint32_t k = n - 1; k >= 1; k--) {
      q = ldw4(M + 4 * k) + xi * q;
      d = d * xi + q;
    }
    const Fp4 s = ldw4(eval_u + 4 * (size_t)(first + i)) * fp4_inv(d);
    q = ldw4(M + 4 * n);
    stw4(out + 4 * (n - 1), ldw4(out + 4 * (n - 1)) + q * s);
    for (uint32_t k = n - 1; k >= 1; k--) {
      q = ldw4(M + 4 * k) + xi * q;
      stw4(out + 4 * (k - 1), ldw4(out + 4 * (k - 1)) + q * s);
    }
  }
}

// the values of sub_head_kernel's fix list: entry e covers the pairs [4e, 4e + 4) (an extension coefficient of a combo's head) and is
// the sum over its terms t in [begin[e], begin[e + 1]) of pw[terms[2t]] * coeff_u[terms[2t + 1]], pw the powers of the DEEP mix
__global__ __launch_bounds__(64) void deep_head_kernel(uint32_t* __restrict__ fix, const uint32_t* __restrict__ pw, const uint32_t* __restrict__ coeff_u,
                                                        const uint32_t* __restrict__ begin, const uint32_t* __restrict__ terms, uint32_t n_entries) {
  const uint32_t e = blockIdx.x * 64 + threadIdx.x;
  if (e >= n_entries) return;
  Fp4 h = fp4_zero();
  for (uint32_t t = begin[e]; t < begin[e + 1]; t++) h = h + ldw4(pw + 4 * (size_t)terms[2 * t]) * ldw4(coeff_u + 4 * (size_t)terms[2 * t + 1]);
#pragma unroll
  for (int q = 0; q < 4; q++) fix[2 * (4 * (size_t)e + q) + 1] = h.e[q];
}

struct Round { Tree tree; DevBuf evaluated; };  // a committed FRI round

// The steps behind the hand-over of the transcript to the device: where their seal words stand in the proof's tail block, in words.
// Steps 7 and 8 always (r0h_ctx_set_device_transcript); the head with steps 3-6 in front of them.  The block is read back once, at
// the end of step 8.
struct IopFree { void operator()(r0h_iop* iop) const { r0h_iop_free(iop); } };
struct TailLayout {
  // the head, under r0h_ctx_set_device_finish only: what steps 3-6 add to the seal, and the verdict of the DEEP divisions
  bool head = false;
  size_t accum_top = 0, check_top = 0;  // the two groups' top layers, 8 * top_size words each
  size_t coeff_u = 0;                   // 4 * n_u words: per register its interpolant, then CHECK's sixteen openings
  size_t report = 0;                    // one word: 0, or 1 + the first DEEP division whose remainder is not zero
  // under r0h_proof_late_device as well: the late public inputs (seal words: tail_collect patches them into the opening block) and one
  // word, 0 or 1 + the first of them that is not canonical; `mix` (below) is the accumulation mix, the device's own
  bool late = false;
  size_t late_report = 0, late_words = 0;
  // under r0h_proof_begin_committed[_top]_enqueue as well (the hand-over before the DATA commitment): in front of the head the DATA
  // group's top layer, 8 * top_size words (seal words), and its root, eight words (what r0h_proof_data_root gives once they are home)
  bool begin = false;
  size_t data_top = 0, data_root = 0;
  std::vector<size_t> round_top;  // per FRI round: its tree's top layer, 8 * top_size words
  size_t final_coeffs = 0;        // 4 * final_degree words
  size_t idx = 0;                 // the query rows [n_trees][R0H_QUERIES]
  std::vector<size_t> opened;     // per tree: R0H_QUERIES packed openings, and behind a top-form tree's the two report words of merkle_open_top
  size_t seal_words = 0;          // everything above: what the read-back brings home
  size_t fold_mix = 0;            // per FRI round the four words of its fold mix (the device's own: never read back)
  size_t poly_mix = 0, z = 0, deep_mix = 0;  // with the head: the challenges of steps 4-6, four words each (the device's own as well)
  size_t mix = 0;                            // with `late`: the circuit's n_mix words
  size_t words = 0;
};

}  // namespace r0h

// The committed CODE group of a program at one trace size: bit-reversed zk-shifted coefficients, evaluations on the 4N coset, Merkle
// nodes, and the host copies of what a commit sends to the transcript (top layer, root).  CODE depends on (circuit, po2) only --
// risc0 keeps one control root per po2 for exactly that reason -- so a prover commits it once and every segment of that size
// reads it: three device buffers that no kernel of a proof writes.  Complete (stream-synchronised) when code_commit returns,
// hence readable from any context of the same device.
struct r0h_code_commit {
  r0h_ctx* ctx = nullptr;  // a kept commitment (r0h_code_commit_new) holds a reference on it
  uint32_t po2 = 0;
  int hashfn = 0;  // the suite the tree was hashed under (the context's when it was made): a proof under another suite refuses it
  r0h::Group g;
  // the CODE columns themselves (a log-derivative accumulation reads its tables from them): the caller's buffer, borrowed, in a proof's
  // own commitment; `kept_columns`, a copy, in a kept one
  const r0h_buf* witness = nullptr;
  r0h::DevBuf kept_columns;
  r0h::TreeTop top;
  r0h_code_commit(uint32_t count, uint32_t p) : po2(p), g(count, (size_t)4 << p) {}
};

// A proof in flight between r0h_proof_begin (CODE and DATA committed, accumulation mix drawn) and r0h_proof_finish.
// Mirrors risc0-zkp's `Prover` object between `commit_group(DATA)` and `finalize`.
struct r0h_proof {
  r0h_ctx* ctx;
  const r0h_circuit* circ;
  uint32_t po2;
  r0h::WriteIop io;
  r0h_code_commit own_code;           // the columns forms: this proof's own commitment (pooled, made by proof_begin); empty otherwise
  const r0h_code_commit* const code;  // where every step reads CODE: the caller's commitment, or own_code
  r0h::Group g_accum, g_data, g_check;
  std::vector<uint32_t> mix, global;
  size_t seal_globals_at = 0;   // where the seal's opening block of public inputs starts
  mutable uint32_t data_root[8] = {0};  // the DATA group's Merkle root (what a session's common challenge is derived from)
  bool mix_drawn = false;
  const r0h_buf *check_code = nullptr, *check_data = nullptr;  // r0h_ctx_set_check_witness: the witness columns proof_finish checks (the caller's buffers)
  // what a step of proof_finish leaves for the steps after it
  // the point table of steps 5 and 6: z * omega^-back for every distinct back of the circuit's taps, then z^4, where CHECK is opened.
  // On the host (`points_host`) or, after the hand-over, on the device (`points`: behind the points the host-known omega^-back)
  uint32_t n_points = 0;
  uint32_t point_of_back[64] = {0};
  std::vector<r0h::Fp4> points_host;
  r0h::DevBuf points;
  std::vector<r0h::Fp4> coeff_u;       // (host) per register the interpolant through its openings, then CHECK's sixteen openings
  std::vector<uint32_t> divide_combo;  // the combo of every DEEP division in job order (whom the tail's report word names)
  r0h::DevBuf fri_coeffs;              // the FRI input; inside step 7 what the rounds so far have folded it to
  std::vector<r0h::Round> rounds;
  // The hand-over: once the host generator has gone to the device, `iop` is that generator and `tail` the block the steps behind it
  // write their seal words into (laid out by `tail_at`); before it, neither exists.  Every step asks `iop` where the transcript lives.
  std::unique_ptr<r0h_iop, r0h::IopFree> iop;
  r0h::DevBuf tail;
  r0h::TailLayout tail_at;
  bool enqueued = false;  // the steps have been enqueued (r0h_proof_finish_enqueue) and wait for r0h_proof_finish_collect
  // r0h_proof_late_device: the late public inputs were absorbed and the mix drawn by the device generator (they stand in the tail; the
  // host's `mix` and the late part of `global` are zeros until the collect).  A circuit without late inputs has drawn its mix on the
  // host at proof_begin: `pre_mix_state` is the generator as it was before, which the device form starts from to draw the same words.
  bool late_device = false;
  std::vector<uint32_t> pre_mix_state;
  // r0h_proof_begin_committed[_top]_enqueue: DATA was committed on the device generator, so `data_root` is on the host only once it
  // has been read back (r0h_proof_data_root: eight words, a wait; or the collect)
  mutable bool data_root_home = true;
  // ... and a proof whose root was read back that way may be aborted right behind it (a session's eviction in phase 1): r0h_proof_abort
  // then asks the stream whether anything is still queued on it, and waits only if so
  mutable bool root_read_back = false;
  // r0h_prove_segment_committed_enqueue: what the enqueued steps read until r0h_prove_segment_collect -- the ACCUM witness, and for a
  // log-derivative accumulation the public inputs as device words
  r0h::DevBuf own_accum, own_globals;
  r0h_proof(r0h_ctx* c, const r0h_circuit* ci, uint32_t p, const r0h_buf* code_columns, const r0h_code_commit* cc)
      : ctx(c), circ(ci), po2(p), io(c->hashfn, &c->p2_host), own_code(ci->group_size[R0H_GROUP_CODE], p), code(cc ? cc : &own_code),
        g_accum(ci->group_size[R0H_GROUP_ACCUM], (size_t)4 << p), g_data(ci->group_size[R0H_GROUP_DATA], (size_t)4 << p),
        g_check(R0H_CHECK_SIZE, (size_t)4 << p) {
    own_code.witness = code_columns;
  }
  const r0h::Group& group(int g) const {  // in the order of the seal's openings: R0H_GROUP_ACCUM, _CODE, _DATA, then CHECK
    const r0h::Group* all[4] = {&g_accum, &code->g, &g_data, &g_check};
    return *all[g];
  }
};

namespace r0h {

// the CODE columns committed into `cc` on `ctx`: the proof-owned commitment of the columns forms, r0h_code_commit_new, r0h_code_root
static const char* code_commit(r0h_ctx* ctx, r0h_code_commit& cc, const r0h_buf* columns) {
  cc.ctx = ctx;
  cc.hashfn = ctx->hashfn;
  cc.witness = columns;
  R0H_TRY(group_build(ctx, cc.g, columns, cc.po2));
  return tree_top(ctx, cc.g.tree, cc.top);  // (a blocking read-back: the stream has drained when this returns)
}

// ------------------------------------------------------------------ the transcript, wherever it lives
// A proof's steps talk to the transcript through the three helpers below.  Each asks `st.iop`: null, and the generator is the host's
// (`st.io.rng`), seal words are read back and appended to `st.io.proof` -- a wait each; set, and the generator is the device's, seal
// words go device to device into their place in the tail block (a word offset, from `st.tail_at`), and nothing waits.
static const char* copy_words(r0h_ctx* ctx, r0h_buf* dst, size_t dst_word, const r0h_buf* src, size_t src_word, size_t n) {
  R0H_TRY_HIP(hipMemcpyAsync(u32(dst) + dst_word, u32(src) + src_word, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
  return nullptr;
}
// A challenge: in `host`, or in the four device words at `dev` (the tail's, which the next kernels read)
struct Challenge {
  Fp4 host;
  const uint32_t* dev = nullptr;
};
static const char* draw_ext(r0h_proof& st, size_t tail_slot, Challenge& out) {
  if (!st.iop) {
    out.host = st.io.rng.ext();
    return nullptr;
  }
  R0H_TRY(r0h_iop_draw_ext(st.iop.get(), st.tail.get(), tail_slot, 1));
  out.dev = u32(st.tail.get()) + tail_slot;
  return nullptr;
}
// A built tree committed: its top layer -- nodes [top_size, 2 * top_size) -- into the seal, its root -- node 1 -- into the transcript
static const char* commit_tree(r0h_proof& st, const Tree& t, size_t tail_slot) {
  if (!st.iop) {
    TreeTop top;
    R0H_TRY(tree_top(st.ctx, t, top));
    top.into(st.io);
    return nullptr;
  }
  const size_t top_words = 8 * t.mp.top_size;
  R0H_TRY(copy_words(st.ctx, st.tail.get(), tail_slot, t.nodes.get(), top_words, top_words));
  return r0h_iop_commit(st.iop.get(), t.nodes.get(), 8);
}
// `n` seal words that lie in device memory, at word `src_word` of `src`, written to the seal and committed as elements.  Words a
// kernel has put into their tail slot itself need no copy (src == the tail).
static const char* commit_words(r0h_proof& st, const r0h_buf* src, size_t src_word, size_t n, size_t tail_slot) {
  if (!st.iop) {
    std::vector<uint32_t> w(n);
    R0H_TRY(r0h_buf_d2h(st.ctx, src, src_word * 4, w.data(), n * 4));
    st.io.write(w.data(), n);
    st.io.commit_elems(w.data(), n);
    return nullptr;
  }
  if (src != st.tail.get()) R0H_TRY(copy_words(st.ctx, st.tail.get(), tail_slot, src, src_word, n));
  return r0h_iop_commit_elems(st.iop.get(), st.tail.get(), tail_slot, n);
}

static const char* proof_late(r0h_proof& st, const uint32_t* late);
static const char* tail_open(r0h_proof& st, bool head, bool late = false, bool begin = false);
static const char* late_enqueue(r0h_proof& st, const r0h_buf* late, const uint32_t* late_host, r0h_buf* mix_out);
// steps 1 and 2: the transcript opens, CODE and DATA are committed (DATA through its kept tree top where one is given).  With `enqueue`
// the generator goes to the device once CODE's top layer -- host words -- is in: DATA is committed there, the mix of a circuit without
// late inputs is drawn there (into `mix_dev` too, if given), and nothing waits for the stream.
static const char* proof_begin(r0h_proof& st, const r0h_buf* data, const uint32_t* global, const r0h_buf* data_top = nullptr, uint32_t top_levels = 0, bool enqueue = false,
                               r0h_buf* mix_dev = nullptr) {
  r0h_ctx* ctx = st.ctx;
  const r0h_circuit* circ = st.circ;
  const uint32_t po2 = st.po2;
  WriteIop& io = st.io;
  const r0h_code_commit& code = *st.code;
  if (!ctx->prof.continued) ctx->prof.names.clear();
  st.global.assign(global, global + circ->n_global);
  if (ctx->check_witness) {
    st.check_code = code.witness;
    st.check_data = data;
    R0H_REQUIRE(st.check_code, "prove_segment: checking the witness needs the CODE columns, and this CODE commitment keeps none");
  }
  if (ctx->check_balance && circ->logup.n_chain) {  // r0h_ctx_set_check_balance: before anything of this segment is committed
    R0H_REQUIRE(code.witness, "prove_segment: checking the witness needs the CODE columns, and this CODE commitment keeps none");
    profile_phase(ctx, "check_balance");
    R0H_TRY(require_balance("prove_segment", ctx, circ, po2, code.witness, data, global));
  }

  profile_phase(ctx, "transcript_seed");
  {
    // the seal opens with every public input and po2; the transcript takes the early ones here and the late ones (inputs that depend
    // on commitments made outside this proof, R0H_SEC_LATE) after the DATA group is committed
    for (uint32_t i = 0; i < circ->n_global - circ->n_late; i++) R0H_REQUIRE(global[i] < P, "prove_segment: global word not canonical");
    transcript_open(io, *circ, global, po2);
    st.seal_globals_at = io.proof.size();
    io.write(global, circ->n_global);
    const uint32_t po2_word = enc(po2);
    io.write(&po2_word, 1);
  }

  profile_phase(ctx, "commit_code");
  if (&code == &st.own_code) R0H_TRY(code_commit(ctx, st.own_code, code.witness));  // the columns forms commit here; a caller's commitment was made ahead of time
  const uint32_t code_count = circ->group_size[R0H_GROUP_CODE];
  R0H_REQUIRE(code.po2 == po2 && code.g.count == code_count, "prove_segment: the CODE commitment is for %u columns of 2^%u rows, this proof needs %u of 2^%u",
              code.g.count, code.po2, code_count, po2);
  R0H_REQUIRE(code.hashfn == ctx->hashfn, "prove_segment: the CODE commitment was made under the %s hash suite, this context is on %s",
              hashfn_name(code.hashfn), hashfn_name(ctx->hashfn));
  R0H_REQUIRE(code.ctx->device == ctx->device, "prove_segment: the CODE commitment lives on device %d, this context on device %d", code.ctx->device, ctx->device);
  code.top.into(io);  // the same words whoever committed
  profile_phase(ctx, "commit_data");
  R0H_TRY(group_build(ctx, st.g_data, data, po2, data_top, top_levels));
  if (enqueue) {  // the hand-over before the DATA commitment: top layer and root go device to device, the root into the generator
    R0H_TRY(tail_open(st, true, true, true));
    R0H_TRY(commit_tree(st, st.g_data.tree, st.tail_at.data_top));
    R0H_TRY(copy_words(ctx, st.tail.get(), st.tail_at.data_root, st.g_data.tree.nodes.get(), 8, 8));
    st.data_root_home = false;
    return circ->n_late ? nullptr : late_enqueue(st, nullptr, nullptr, mix_dev);
  }
  R0H_TRY(commit_tree(st, st.g_data.tree, 0));  // (on the host: the hand-over comes later, if at all)
  R0H_TRY(r0h_buf_d2h(ctx, st.g_data.tree.nodes.get(), 32, st.data_root, 32));
  if (!circ->n_late) {
    st.pre_mix_state.resize(SUITE_RNG_MAX_WORDS);
    st.pre_mix_state.resize(io.rng.state(st.pre_mix_state.data()));
    return proof_late(st, nullptr);
  }
  return nullptr;
}

// the late public inputs enter the transcript (and the seal's opening block), then the accumulation mix is drawn
static const char* proof_late(r0h_proof& st, const uint32_t* late) {
  const uint32_t n_late = st.circ->n_late, n_early = st.circ->n_global - n_late;
  R0H_REQUIRE(!st.mix_drawn, "r0h_proof_late: the accumulation mix has been drawn already");
  R0H_REQUIRE(!st.iop, "r0h_proof_late: the proof's transcript went to the device before its DATA commitment (r0h_proof_begin_committed_enqueue): r0h_proof_late_device takes the late inputs");
  if (n_late) {
    R0H_REQUIRE(late, "r0h_proof_late: NULL argument");
    for (uint32_t i = 0; i < n_late; i++) R0H_REQUIRE(late[i] < P, "r0h_proof_late: word %u not canonical", i);
    memcpy(st.global.data() + n_early, late, (size_t)n_late * 4);
    memcpy(st.io.proof.data() + st.seal_globals_at + n_early, late, (size_t)n_late * 4);
    st.io.commit_elems(late, n_late);
  }
  st.mix.resize(st.circ->n_mix);
  for (uint32_t i = 0; i < st.circ->n_mix; i++) st.mix[i] = st.io.rng.elem();
  st.mix_drawn = true;
  profile_phase(st.ctx, "accum");
  return nullptr;
}

// ------------------------------------------------------------------ the hand-over
// The tail block laid out and taken from the pool, and the host generator handed over to the device (its state goes up in stream
// order).  With `head` the block starts with what steps 3-6 add to the seal; every part of it keeps its offset modulo 8 words.
static const char* tail_open(r0h_proof& st, bool head, bool late, bool begin) {
  r0h_ctx* ctx = st.ctx;
  const FriSchedule fri((size_t)1 << st.po2);
  TailLayout& at = st.tail_at;
  at = TailLayout();
  {
    size_t w = 0;
    if (head) {
      at.head = true;
      if (begin) {
        at.begin = true;
        at.data_top = w;
        w += 8 * st.g_data.tree.mp.top_size;
        at.data_root = w;
        w += 8;
      }
      at.accum_top = w;
      w += 8 * st.g_accum.tree.mp.top_size;
      at.check_top = w;
      w += 8 * st.g_check.tree.mp.top_size;
      at.coeff_u = w;
      w += 4 * (st.circ->taps.size() + R0H_CHECK_SIZE);
      at.report = w;
      at.late_report = w + 1;
      w = (w + (late ? 2 : 1) + 7) & ~(size_t)7;
      if (late) {
        at.late = true;
        at.late_words = w;
        w = (w + st.circ->n_late + 7) & ~(size_t)7;
      }
    }
    for (const FriRound& fr : fri.rounds) { at.round_top.push_back(w); w += 8 * MerkleShape(fr.rows, R0H_FRI_FOLD * 4).top_size; }
    at.final_coeffs = w;
    w += 4 * fri.final_degree;
    at.idx = w;
    w += (4 + fri.rounds.size()) * R0H_QUERIES;
    for (size_t t = 0; t < 4 + fri.rounds.size(); t++) {
      const MerkleShape mp = t < 4 ? st.group((int)t).tree.mp : MerkleShape(fri.rounds[t - 4].rows, R0H_FRI_FOLD * 4);
      at.opened.push_back(w);
      w += (size_t)R0H_QUERIES * mp.opening_words() + (t < 4 && st.group((int)t).tree.top_levels ? 2 : 0);
    }
    at.seal_words = w;
    at.fold_mix = w;
    w += 4 * fri.rounds.size();
    if (head) {
      w = (w + 3) & ~(size_t)3;
      at.poly_mix = w;
      at.z = w + 4;
      at.deep_mix = w + 8;
      w += 12;
      if (late) { at.mix = w; w += st.circ->n_mix; }
    }
    at.words = w;
  }
  R0H_TRY(st.tail.alloc(ctx, at.words * 4));
  r0h_iop* iop = nullptr;
  if (late && !begin && !st.circ->n_late) R0H_TRY(iop_make_words(ctx, st.pre_mix_state.data(), st.pre_mix_state.size(), &iop));  // (the host has drawn the mix: from before it did)
  else R0H_TRY(iop_make(ctx, st.io.rng, &iop));
  st.iop.reset(iop);
  return nullptr;
}

// ---- the late public inputs on the device transcript (r0h_proof_late_device).  The generator goes up before them: they are absorbed
// from device words and the accumulation mix is drawn into device words, so the host is out of the loop from the DATA commitment on.
// 0, or 1 + the first word that is not canonical (a handful of words: one lane)
__global__ __launch_bounds__(64) void late_check_kernel(uint32_t* __restrict__ report, const uint32_t* __restrict__ late, uint32_t n_late) {
  if (blockIdx.x || threadIdx.x) return;
  uint32_t bad = 0;
  for (uint32_t k = n_late; k-- > 0;)
    if (late[k] >= P) bad = k + 1;
  *report = bad;
}
static const char* proof_late_device(r0h_proof& st, const r0h_buf* late, r0h_buf* mix_out) {
  r0h_ctx* ctx = st.ctx;
  const uint32_t n_late = st.circ->n_late, n_mix = st.circ->n_mix;
  R0H_REQUIRE(!st.late_device && !(st.mix_drawn && n_late), "r0h_proof_late_device: the accumulation mix has been drawn already");
  R0H_REQUIRE(st.io.suite->fn() == ctx->hashfn, "r0h_proof_late_device: the proof was begun under the %s hash suite, its context is now on %s", hashfn_name(st.io.suite->fn()),
              hashfn_name(ctx->hashfn));
  R0H_REQUIRE(ctx->device_finish, "r0h_proof_late_device: the proof's context has r0h_ctx_set_device_finish off: the steps behind the late inputs would ask the host generator");
  R0H_REQUIRE(n_late ? late && late->bytes == (size_t)n_late * 4 : !late || !late->bytes, "r0h_proof_late_device: the late buffer holds %zu words, the circuit has %u late public inputs",
              late ? late->bytes / 4 : (size_t)0, n_late);
  R0H_REQUIRE(!mix_out || mix_out->bytes >= (size_t)n_mix * 4, "r0h_proof_late_device: mix_out holds %zu words, the circuit draws %u", mix_out ? mix_out->bytes / 4 : (size_t)0, n_mix);
  // A proof begun by r0h_proof_begin_committed_enqueue has handed its generator over already: the late inputs follow DATA's root there.
  if (st.iop) return late_enqueue(st, late, nullptr, mix_out);
  // a step that fails after the hand-over takes it back: the tail and the device generator go (to the pool, behind what was launched),
  // so the proof is as it was and r0h_proof_late, or this call again, finds it so
  const char* err = tail_open(st, true, true);
  if (!err) err = late_enqueue(st, late, nullptr, mix_out);
  if (err) {
    st.iop.reset();
    st.tail.reset();
    st.tail_at = TailLayout();
  }
  return err;
}
// The late inputs -- device words at `late`, or host words at `late_host` -- into the tail, their canonicity into its report word, the
// inputs into the device generator, and the mix drawn into the tail (and `mix_out`).  The generator has been handed over.
static const char* late_enqueue(r0h_proof& st, const r0h_buf* late, const uint32_t* late_host, r0h_buf* mix_out) {
  r0h_ctx* ctx = st.ctx;
  const uint32_t n_late = st.circ->n_late, n_mix = st.circ->n_mix;
  const TailLayout& at = st.tail_at;
  uint32_t* tail = u32(st.tail.get());
  if (n_late && late) R0H_TRY(copy_words(ctx, st.tail.get(), at.late_words, late, 0, n_late));
  else if (n_late) R0H_TRY(stage_h2d(ctx, tail + at.late_words, late_host, (size_t)n_late * 4));
  hipLaunchKernelGGL(late_check_kernel, dim3(1), dim3(64), 0, ctx->stream, tail + at.late_report, tail + at.late_words, n_late);
  R0H_TRY(launch_ok("late_check_kernel"));
  if (n_late) R0H_TRY(r0h_iop_commit_elems(st.iop.get(), st.tail.get(), at.late_words, n_late));
  R0H_TRY(iop_draw_words(st.iop.get(), st.tail.get(), at.mix, n_mix));
  if (mix_out && n_mix) R0H_TRY(copy_words(ctx, mix_out, 0, st.tail.get(), at.mix, n_mix));
  st.mix.assign(n_mix, 0u);  // (canonical stand-ins: the kernels read the tail's words)
  st.late_device = true;
  if (!st.mix_drawn) profile_phase(ctx, "accum");
  st.mix_drawn = true;
  return nullptr;
}

// step 3: commit ACCUM -- behind the DATA evaluations made again where r0h_proof_shrink gave them back, and the witness check where it is on
static const char* commit_accum(r0h_proof& st, const r0h_buf* accum) {
  r0h_ctx* ctx = st.ctx;
  if (!st.g_data.evaluated) {  // the same expanding NTT over the kept coefficients
    profile_phase(ctx, "evaluate_data_again");
    R0H_TRY(group_evaluate(ctx, st.g_data, st.po2));
  }
  if (st.check_data) {  // reads its table back: the one wait of an enqueue
    profile_phase(ctx, "check_witness");
    if (st.late_device) {  // the checker takes host words: the late inputs and the mix come home for it (two more read-backs)
      const uint32_t n_late = st.circ->n_late;
      if (n_late) R0H_TRY(r0h_buf_d2h(ctx, st.tail.get(), st.tail_at.late_words * 4, st.global.data() + (st.circ->n_global - n_late), (size_t)n_late * 4));
      if (st.circ->n_mix) R0H_TRY(r0h_buf_d2h(ctx, st.tail.get(), st.tail_at.mix * 4, st.mix.data(), (size_t)st.circ->n_mix * 4));
      for (uint32_t i = 0; i < n_late; i++) R0H_REQUIRE(st.global[st.circ->n_global - n_late + i] < P, "r0h_proof_finish: late public input %u is not canonical", i);
    }
    R0H_TRY(require_witness("prove_segment", ctx, st.circ, st.po2, accum, st.check_code, st.check_data, st.global.data(), st.mix.data()));
  }
  profile_phase(ctx, "commit_accum");
  R0H_TRY(group_build(ctx, st.g_accum, accum, st.po2));
  return commit_tree(st, st.g_accum.tree, st.tail_at.accum_top);
}

// step 4: the constraint check on the 4N coset, and CHECK committed
static const char* commit_check(r0h_proof& st) {
  r0h_ctx* ctx = st.ctx;
  Group& g_check = st.g_check;
  profile_phase(ctx, "eval_check");
  Challenge poly_mix;
  R0H_TRY(draw_ext(st, st.tail_at.poly_mix, poly_mix));
  R0H_TRY(g_check.coeffs.alloc(ctx, ((size_t)R0H_INV_RATE << st.po2) * 16));
  const r0h_buf *accum = st.g_accum.evaluated.get(), *code = st.code->g.evaluated.get(), *data = st.g_data.evaluated.get();
  if (poly_mix.dev) {  // (r0h_proof_late_device: the late public inputs and the mix are the tail's words as well)
    const uint32_t* tail = u32(st.tail.get());
    R0H_TRY(eval_check_dev(ctx, st.circ, st.po2, accum, code, data, st.global.data(), st.mix.data(), poly_mix.dev, g_check.coeffs.get(),
                           st.late_device ? tail + st.tail_at.late_words : nullptr, st.late_device ? tail + st.tail_at.mix : nullptr));
  } else {
    R0H_TRY(r0h_eval_check(ctx, st.circ, st.po2, accum, code, data, st.global.data(), st.mix.data(), poly_mix.host.e, g_check.coeffs.get()));
  }
  profile_phase(ctx, "commit_check");
  R0H_TRY(r0h_batch_interpolate_ntt(ctx, g_check.coeffs.get(), 4, st.po2 + 2));  // 4 polys of 4N == 16 polys of N (bit-reversed)
  R0H_TRY(group_build(ctx, g_check, nullptr, st.po2));
  return commit_tree(st, g_check.tree, st.tail_at.check_top);
}

// Steps 5 and 6 always run in the same form: the transcript is handed over before step 3, before step 7 or not at all, never between
// them.  So step 6 finds the point table, and coeff_u, where step 5 left them -- on the host, or on the device and in the tail.
//
// deep_points_kernel over plain tables (the sequencer's, and r0h_deep_points_buf's): n_backs + 1 points to d_pts from z at d_z
static const char* deep_points_table(r0h_ctx* ctx, uint32_t* d_pts, const uint32_t* d_z, uint32_t* d_wpow, const uint32_t* wpow, uint32_t n_backs) {
  R0H_TRY(stage_h2d(ctx, d_wpow, wpow, (size_t)n_backs * 4));  // the kernel's: omega^-back, host-known, n_backs words
  KScope ks(ctx, "deep_points_kernel", 16.0 * (n_backs + 1));
  hipLaunchKernelGGL(deep_points_kernel, dim3((n_backs + 1 + 63) / 64), dim3(64), 0, ctx->stream, d_pts, d_z, d_wpow, n_backs);
  return launch_ok("deep_points_kernel");
}
// the point table: a point per distinct back of the circuit's taps (the blob format admits backs below 64), then z^4
static const char* deep_points(r0h_proof& st, const Challenge& z) {
  r0h_ctx* ctx = st.ctx;
  const uint32_t back_one = rou_rev(st.po2);  // omega^-1: a tap `back` rows behind is opened at z * back_one^back
  bool has_back[64] = {false};
  for (const Tap& t : st.circ->taps) has_back[t.back] = true;
  std::vector<uint32_t> wpow;
  for (uint32_t b = 0; b < 64; b++)
    if (has_back[b]) { st.point_of_back[b] = (uint32_t)wpow.size(); wpow.push_back(fpow(back_one, b)); }
  const uint32_t n_backs = (uint32_t)wpow.size();
  st.n_points = n_backs + 1;
  if (!z.dev) {
    st.points_host.resize(st.n_points);
    for (uint32_t i = 0; i < n_backs; i++) st.points_host[i] = scale(z.host, wpow[i]);
    st.points_host[n_backs] = fp4_pow(z.host, 4);
    return nullptr;
  }
  R0H_TRY(st.points.alloc(ctx, (size_t)(4 * st.n_points + n_backs) * 4));
  uint32_t* pts = u32(st.points.get());
  return deep_points_table(ctx, pts, z.dev, pts + 4 * st.n_points, wpow.data(), n_backs);
}
// step 5's middle on the host: the evaluations read back, every register's interpolant through its openings by poly_interpolate
static const char* interpolate_host(r0h_proof& st, const r0h_buf* d_eval, const std::vector<Fp4>& xs) {
  const uint32_t n_u = (uint32_t)xs.size(), n_taps = n_u - R0H_CHECK_SIZE;
  std::vector<Fp4> eval_u(n_u);
  R0H_TRY(r0h_buf_d2h(st.ctx, d_eval, 0, eval_u.data(), (size_t)n_u * 16));
  st.coeff_u.resize(n_u);
  for (const Reg& reg : st.circ->regs) poly_interpolate(&st.coeff_u[reg.first_tap], &xs[reg.first_tap], &eval_u[reg.first_tap], reg.size);
  for (uint32_t i = 0; i < R0H_CHECK_SIZE; i++) st.coeff_u[n_taps + i] = eval_u[n_taps + i];
  return nullptr;
}
// and on the device: interpolate_regs_kernel writes coeff_u (n_taps + R0H_CHECK_SIZE elements) from the evaluations d_eval.  Tap t is opened
// at point tap_pt[t] of the table d_points; register r is the taps [regs[2r], +regs[2r + 1]), one to 64 of them, no two registers sharing a tap.
static const char* interpolate_regs(r0h_ctx* ctx, uint32_t* d_coeff_u, const uint32_t* d_eval, const uint32_t* d_points, const uint32_t* tap_pt, const uint32_t* regs,
                                    uint32_t n_regs, uint32_t n_taps) {
  // the registers' table: [point of every tap][per register: first tap, taps, first work slot], then the work slots (taps + 1 a register)
  std::vector<uint32_t> table(tap_pt, tap_pt + n_taps);
  uint32_t work_slots = 0;
  for (uint32_t r = 0; r < n_regs; r++) {
    table.insert(table.end(), {regs[2 * r], regs[2 * r + 1], work_slots});
    work_slots += regs[2 * r + 1] + 1;
  }
  DevBuf d_regs;
  R0H_TRY(d_regs.alloc(ctx, (table.size() + 4 * (size_t)work_slots) * 4));
  R0H_TRY(stage_h2d(ctx, d_regs->ptr, table.data(), table.size() * 4));
  KScope ks(ctx, "interpolate_regs_kernel", 32.0 * (n_taps + R0H_CHECK_SIZE));
  const uint32_t* d_table = u32(d_regs.get());
  hipLaunchKernelGGL(interpolate_regs_kernel, dim3((n_regs + R0H_CHECK_SIZE + 63) / 64), dim3(64), 0, ctx->stream, d_coeff_u, d_eval, d_points, d_table, d_table + n_taps, n_regs,
                     n_taps, u32(d_regs.get()) + table.size());
  return launch_ok("interpolate_regs_kernel");
}
static const char* interpolate_device(r0h_proof& st, const r0h_buf* d_eval, const std::vector<uint32_t>& pt) {
  const uint32_t n_taps = (uint32_t)pt.size() - R0H_CHECK_SIZE;
  std::vector<uint32_t> regs;
  for (const Reg& reg : st.circ->regs) regs.insert(regs.end(), {reg.first_tap, reg.size});
  return interpolate_regs(st.ctx, u32(st.tail.get()) + st.tail_at.coeff_u, u32(d_eval), u32(st.points.get()), pt.data(), regs.data(), (uint32_t)st.circ->regs.size(), n_taps);
}

// step 5: every tap opened at z * omega^-back and CHECK at z^4; coeff_u into the seal and the transcript
static const char* evaluate_at_z(r0h_proof& st) {
  r0h_ctx* ctx = st.ctx;
  const r0h_circuit* circ = st.circ;
  profile_phase(ctx, "evaluate_at_z");
  // (a register's taps are a run of the blob's: never none.  Step 6 keeps a combo's head in 64 slots.)
  for (const Reg& reg : circ->regs) R0H_REQUIRE(reg.size >= 1 && reg.size <= 64, "prove_segment: register with more than 64 taps");
  Challenge z;
  R0H_TRY(draw_ext(st, st.tail_at.z, z));
  R0H_TRY(deep_points(st, z));
  const uint32_t n_taps = (uint32_t)circ->taps.size(), n_u = n_taps + R0H_CHECK_SIZE;  // CHECK's columns stand behind the taps, as a fourth group
  std::vector<uint32_t> which(n_u), pt(n_u);  // request k: column which[k] of its group at point pt[k] of the table
  for (uint32_t t = 0; t < n_taps; t++) { which[t] = circ->taps[t].offset; pt[t] = st.point_of_back[circ->taps[t].back]; }
  for (uint32_t i = 0; i < R0H_CHECK_SIZE; i++) { which[n_taps + i] = i; pt[n_taps + i] = st.n_points - 1; }
  std::vector<Fp4> xs;  // on the host a request carries its point
  if (!z.dev)
    for (uint32_t p : pt) xs.push_back(st.points_host[p]);
  DevBuf d_eval;
  R0H_TRY(d_eval.alloc(ctx, (size_t)n_u * 16));
  for (int g = 0; g < 4; g++) {
    const uint32_t b = circ->group_tap_begin[g], e = g < 3 ? circ->group_tap_begin[g + 1] : n_u;
    if (e == b) continue;
    r0h_buf view = buf_view(d_eval.get(), (size_t)b * 16, (size_t)(e - b) * 16);
    if (z.dev) R0H_TRY(evaluate_any_points(ctx, st.group(g).coeffs.get(), st.po2, which.data() + b, pt.data() + b, e - b, u32(st.points.get()), st.n_points, &view, true));
    else R0H_TRY(evaluate_any(ctx, st.group(g).coeffs.get(), st.po2, which.data() + b, (const uint32_t*)(xs.data() + b), e - b, &view, true));
  }
  if (z.dev) {
    R0H_TRY(interpolate_device(st, d_eval.get(), pt));
    return commit_words(st, st.tail.get(), st.tail_at.coeff_u, 4 * (size_t)n_u, st.tail_at.coeff_u);
  }
  R0H_TRY(interpolate_host(st, d_eval.get(), xs));
  st.io.write((const uint32_t*)st.coeff_u.data(), 4 * (size_t)n_u);
  st.io.commit_elems((const uint32_t*)st.coeff_u.data(), 4 * (size_t)n_u);
  return nullptr;
}

// step 6, second part: subtract the interpolants from the mixed combos -- only the first few coefficients of each combo change
// The fix list is (word index, value) pairs, four to an entry; entry e is coefficient i of combo k's head, in the order of (k, i).  The
// indices are the host's in both forms; the two routines below fill in the values and leave the list at the start of `d_fix`.
// On the host: the heads summed from coeff_u and the running powers of the mix (a power per register, then one per CHECK column)
// Both take the registers as (combo, first tap, taps) triples and coeff_u as n_taps + R0H_CHECK_SIZE elements, CHECK's openings last.
static const char* head_values_host(r0h_ctx* ctx, const uint32_t* regs, uint32_t n_regs, uint32_t n_taps, const Fp4* coeff_u, const Fp4& mixv,
                                    const std::vector<uint32_t>& head_len, std::vector<uint32_t>& fix, DevBuf& d_fix) {
  const uint32_t n_combos = (uint32_t)head_len.size() - 1;
  std::vector<Fp4> head((size_t)(n_combos + 1) * 64, fp4_zero());
  Fp4 cur = fp4_one();
  for (uint32_t r = 0; r < n_regs; r++) {
    const uint32_t combo = regs[3 * r], first_tap = regs[3 * r + 1], size = regs[3 * r + 2];
    for (uint32_t i = 0; i < size; i++) {
      Fp4& h = head[(size_t)combo * 64 + i];
      h = h + cur * coeff_u[first_tap + i];
    }
    cur = cur * mixv;
  }
  for (uint32_t i = 0; i < R0H_CHECK_SIZE; i++) {
    head[(size_t)n_combos * 64] = head[(size_t)n_combos * 64] + cur * coeff_u[n_taps + i];
    cur = cur * mixv;
  }
  size_t e = 0;
  for (uint32_t k = 0; k <= n_combos; k++)
    for (uint32_t i = 0; i < head_len[k]; i++, e++)
      for (uint32_t q = 0; q < 4; q++) fix[2 * (4 * e + q) + 1] = head[(size_t)k * 64 + i].e[q];
  R0H_TRY(d_fix.alloc(ctx, fix.size() * 4));
  return stage_h2d(ctx, d_fix->ptr, fix.data(), fix.size() * 4);
}
// On the device: per entry the terms of its sum, (power of the mix, word of coeff_u) in the same running order; deep_head_kernel adds them up
static const char* head_values_device(r0h_ctx* ctx, const uint32_t* regs, uint32_t n_regs, uint32_t n_taps, const uint32_t* d_coeff_u, const uint32_t* d_mix,
                                      const std::vector<uint32_t>& head_len, const std::vector<uint32_t>& fix, DevBuf& d_fix) {
  const uint32_t n_combos = (uint32_t)head_len.size() - 1;
  std::vector<uint32_t> begin(1, 0u), terms;
  for (uint32_t k = 0; k <= n_combos; k++)
    for (uint32_t i = 0; i < head_len[k]; i++) {
      if (k < n_combos) {
        for (uint32_t r = 0; r < n_regs; r++)
          if (regs[3 * r] == k && regs[3 * r + 2] > i) terms.insert(terms.end(), {r, regs[3 * r + 1] + i});
      } else {
        for (uint32_t j = 0; j < R0H_CHECK_SIZE; j++) terms.insert(terms.end(), {n_regs + j, n_taps + j});
      }
      begin.push_back((uint32_t)(terms.size() / 2));
    }
  const uint32_t n_entries = (uint32_t)begin.size() - 1, n_pw = n_regs + R0H_CHECK_SIZE;
  std::vector<uint32_t> table(fix);  // [fix pairs][begin][terms], then the powers of the mix
  table.insert(table.end(), begin.begin(), begin.end());
  table.insert(table.end(), terms.begin(), terms.end());
  R0H_TRY(d_fix.alloc(ctx, (table.size() + 4 * (size_t)n_pw) * 4));
  R0H_TRY(stage_h2d(ctx, d_fix->ptr, table.data(), table.size() * 4));
  uint32_t *d_table = u32(d_fix.get()), *d_pw = d_table + table.size();
  R0H_TRY(ext_powers(ctx, d_pw, d_mix, nullptr, n_pw));
  KScope ks(ctx, "deep_head_kernel", 32.0 * (double)(terms.size() / 2));
  hipLaunchKernelGGL(deep_head_kernel, dim3((n_entries + 63) / 64), dim3(64), 0, ctx->stream, d_table, d_pw, d_coeff_u, d_table + fix.size(),
                     d_table + fix.size() + begin.size(), n_entries);
  return launch_ok("deep_head_kernel");
}
// `combos`: n_combos + 1 polynomials of 2^po2 extension coefficients, the last one CHECK's.  The device form (d_mix) reads coeff_u from
// d_coeff_u, the host form from coeff_u_host.
static const char* subtract_heads(r0h_ctx* ctx, r0h_buf* combos, uint32_t po2, uint32_t n_combos, const uint32_t* regs, uint32_t n_regs, uint32_t n_taps, const Fp4* coeff_u_host,
                                  const uint32_t* d_coeff_u, const Fp4* mix_host, const uint32_t* d_mix) {
  std::vector<uint32_t> head_len(n_combos + 1, 0);  // (at most 64: evaluate_at_z has looked)
  for (uint32_t r = 0; r < n_regs; r++)
    if (regs[3 * r + 2] > head_len[regs[3 * r]]) head_len[regs[3 * r]] = regs[3 * r + 2];
  head_len[n_combos] = 1;
  R0H_REQUIRE(((size_t)(n_combos + 1) << po2) * 4 < ((size_t)1 << 32), "prove_segment: combos buffer exceeds 32-bit word indexing");
  std::vector<uint32_t> fix;
  for (uint32_t k = 0; k <= n_combos; k++)
    for (uint32_t i = 0; i < head_len[k]; i++)
      for (uint32_t q = 0; q < 4; q++) {
        fix.push_back((uint32_t)((((size_t)k << po2) + i) * 4 + q));
        fix.push_back(0u);  // its value
      }
  DevBuf d_fix;  // back to the pool once the kernel that reads it is enqueued
  if (d_mix) R0H_TRY(head_values_device(ctx, regs, n_regs, n_taps, d_coeff_u, d_mix, head_len, fix, d_fix));
  else R0H_TRY(head_values_host(ctx, regs, n_regs, n_taps, coeff_u_host, *mix_host, head_len, fix, d_fix));
  const uint32_t nf = (uint32_t)(fix.size() / 2);
  hipLaunchKernelGGL(sub_head_kernel, dim3((nf + 255) / 256), dim3(256), 0, ctx->stream, u32(combos), u32(d_fix.get()), nf);
  return launch_ok("sub_head_kernel");
}
static const char* subtract_interpolants(r0h_proof& st, r0h_buf* combos, const Challenge& mix, uint32_t n_combos) {
  std::vector<uint32_t> regs;
  for (const Reg& reg : st.circ->regs) regs.insert(regs.end(), {reg.combo, reg.first_tap, reg.size});
  return subtract_heads(st.ctx, combos, st.po2, n_combos, regs.data(), (uint32_t)st.circ->regs.size(), (uint32_t)st.circ->taps.size(), st.coeff_u.data(),
                        mix.dev ? u32(st.tail.get()) + st.tail_at.coeff_u : nullptr, &mix.host, mix.dev);
}

// step 6, third part: every (combo, point) division of the DEEP step as one batch: a launch set per "k-th point of every combo", one
// read-back of all remainders (upstream divides on the host; round 1 here ran one scan and one host sync per division)
// A job is (combo, point of the table): a combo by every back of its registers, the last combo -- CHECK's -- by z^4.  On the host the
// remainders come back and are looked at here; on the device the tail's report word names the first that is not zero (tail_collect).
static const char* deep_divide(r0h_proof& st, r0h_buf* combos, uint32_t n_combos) {
  const r0h_circuit* circ = st.circ;
  std::vector<uint32_t>& job_poly = st.divide_combo;
  std::vector<uint32_t> job_pt;
  job_poly.clear();
  for (uint32_t k = 0; k < n_combos; k++)
    for (uint32_t b = circ->combo_begin[k]; b < circ->combo_begin[k + 1]; b++) {
      job_poly.push_back(k);
      job_pt.push_back(st.point_of_back[circ->combo_backs[b]]);
    }
  job_poly.push_back(n_combos);
  job_pt.push_back(st.n_points - 1);
  const uint32_t n = 1u << st.po2, n_jobs = (uint32_t)job_poly.size();
  if (st.iop) return poly_divide_batch_points(st.ctx, combos, n, job_poly.data(), job_pt.data(), n_jobs, u32(st.points.get()), st.n_points, u32(st.tail.get()) + st.tail_at.report);
  std::vector<uint32_t> points, rem(4 * (size_t)n_jobs);
  for (uint32_t p : job_pt) points.insert(points.end(), st.points_host[p].e, st.points_host[p].e + 4);
  R0H_TRY(poly_divide_batch(st.ctx, combos, n, job_poly.data(), points.data(), n_jobs, rem.data()));
  for (uint32_t j = 0; j < n_jobs; j++)
    R0H_REQUIRE(!(rem[4 * j] | rem[4 * j + 1] | rem[4 * j + 2] | rem[4 * j + 3]),
                "prove_segment: DEEP quotient of combo %u has a non-zero remainder (witness violates the taps?)", job_poly[j]);
  return nullptr;
}

// step 6: the columns of the four groups mixed into the combos, the interpolants subtracted, the divisions, the sum: the FRI input
static const char* deep(r0h_proof& st) {
  r0h_ctx* ctx = st.ctx;
  const r0h_circuit* circ = st.circ;
  const uint32_t po2 = st.po2, n = 1u << po2;
  profile_phase(ctx, "mix_combos");
  Challenge mix;
  R0H_TRY(draw_ext(st, st.tail_at.deep_mix, mix));
  const uint32_t n_combos = (uint32_t)circ->combo_begin.size() - 1;
  DevBuf combos;  // back to the pool on return: before the first FRI round
  R0H_TRY(combos.alloc(ctx, (size_t)(n_combos + 1) * n * 16));
  R0H_TRY(r0h_buf_zero(ctx, combos.get()));
  uint32_t first_exp = 0;  // a column is weighed by the mix to its position in the running order over the four groups
  Fp4 cur = fp4_one();     // (host) mix^first_exp
  for (int g = 0; g < 4; g++) {
    const uint32_t gs = st.group(g).count;
    std::vector<uint32_t> combo_of(gs, g < 3 ? 0u : n_combos);  // CHECK's columns all go into the last combo
    for (const Reg& reg : circ->regs)
      if (reg.group == (uint32_t)g) combo_of[reg.offset] = reg.combo;
    if (mix.dev) {
      R0H_TRY(mix_poly_coeffs_dev(ctx, combos.get(), first_exp, mix.dev, st.group(g).coeffs.get(), combo_of.data(), gs, po2));
    } else {
      R0H_TRY(r0h_mix_poly_coeffs(ctx, combos.get(), cur.e, mix.host.e, st.group(g).coeffs.get(), combo_of.data(), gs, po2));
      cur = cur * fp4_pow(mix.host, gs);
    }
    first_exp += gs;
  }
  R0H_TRY(bit_reverse_ext(ctx, combos.get(), n_combos + 1, po2));  // combos were mixed in bit-reversed order: natural from here on
  R0H_TRY(subtract_interpolants(st, combos.get(), mix, n_combos));
  profile_phase(ctx, "deep_divide");
  R0H_TRY(deep_divide(st, combos.get(), n_combos));
  R0H_TRY(st.fri_coeffs.alloc(ctx, (size_t)n * 16));
  R0H_TRY(r0h_eltwise_sum_extelem(ctx, st.fri_coeffs.get(), combos.get(), n_combos + 1, n));
  return r0h_batch_bit_reverse(ctx, st.fri_coeffs.get(), 4, po2);
}

// step 7: per round evaluate, commit, draw the fold mix, fold by 16; what is left goes into the seal as it is
static const char* fri_commit(r0h_proof& st) {
  r0h_ctx* ctx = st.ctx;
  const TailLayout& at = st.tail_at;
  profile_phase(ctx, "fri_commit");
  const FriSchedule fri((size_t)1 << st.po2);
  for (size_t r = 0; r < fri.rounds.size(); r++) {
    const FriRound& fr = fri.rounds[r];
    Round rd{Tree(fr.rows, R0H_FRI_FOLD * 4), DevBuf()};
    R0H_TRY(rd.evaluated.alloc(ctx, fr.domain * 16));
    R0H_TRY(r0h_batch_expand_into_evaluate_ntt(ctx, rd.evaluated.get(), st.fri_coeffs.get(), 4, log2u(fr.degree), 2));
    R0H_TRY(tree_build(ctx, rd.tree, rd.evaluated.get()));
    R0H_TRY(commit_tree(st, rd.tree, st.iop ? at.round_top[r] : 0));
    Challenge fold_mix;
    R0H_TRY(draw_ext(st, at.fold_mix + 4 * r, fold_mix));
    DevBuf folded;
    R0H_TRY(folded.alloc(ctx, fr.degree / R0H_FRI_FOLD * 16));
    const uint32_t n_folded = (uint32_t)(fr.degree / R0H_FRI_FOLD);
    if (fold_mix.dev) R0H_TRY(r0h_fri_fold_buf(ctx, folded.get(), st.fri_coeffs.get(), st.tail.get(), at.fold_mix + 4 * r, n_folded));
    else R0H_TRY(r0h_fri_fold(ctx, folded.get(), st.fri_coeffs.get(), fold_mix.host.e, n_folded));
    st.fri_coeffs = std::move(folded);  // the coefficients it was folded from go back to the pool
    st.rounds.push_back(std::move(rd));
  }
  R0H_TRY(r0h_batch_bit_reverse(ctx, st.fri_coeffs.get(), 4, log2u(fri.final_degree)));
  R0H_TRY(commit_words(st, st.fri_coeffs.get(), 0, 4 * fri.final_degree, at.final_coeffs));
  st.fri_coeffs.reset();
  return nullptr;
}

static std::vector<const Tree*> proof_trees(const r0h_proof& st) {  // in the order of the seal's openings
  std::vector<const Tree*> trees;
  for (int g = 0; g < 4; g++) trees.push_back(&st.group(g).tree);
  for (const Round& rd : st.rounds) trees.push_back(&rd.tree);
  return trees;
}

// step 8: the query positions depend only on the transcript state, not on the openings: draw all of them, then open each tree for
// all queries in one kernel.  On the device both go into the tail, and the top-form trees' verdicts wait for tail_collect; on the host
// the rows are drawn here and every tree's openings come back in a copy of their own.
static const char* queries(r0h_proof& st) {
  r0h_ctx* ctx = st.ctx;
  profile_phase(ctx, "queries");
  const size_t domain = (size_t)R0H_INV_RATE << st.po2;
  const std::vector<const Tree*> trees = proof_trees(st);
  const uint32_t nq = R0H_QUERIES, n_trees = (uint32_t)trees.size();
  if (st.iop) {
    const TailLayout& at = st.tail_at;
    uint32_t* tail = u32(st.tail.get());
    std::vector<uint32_t> rows;
    for (const Tree* t : trees) rows.push_back((uint32_t)t->mp.rows);
    R0H_TRY(r0h_iop_draw_queries(st.iop.get(), (uint32_t)domain, rows.data(), n_trees, nq, st.tail.get(), at.idx));
    for (uint32_t t = 0; t < n_trees; t++) R0H_TRY(open_tree(ctx, *trees[t], tail + at.idx + (size_t)t * nq, nq, tail + at.opened[t]));
    return nullptr;
  }
  std::vector<uint32_t> idx((size_t)n_trees * nq);
  for (uint32_t q = 0; q < nq; q++) {
    size_t pos = st.io.rng.bits(log2u(domain)) % domain;
    for (uint32_t t = 0; t < n_trees; t++) {
      if (t >= 4) pos = pos % trees[t]->mp.rows;
      idx[(size_t)t * nq + q] = (uint32_t)pos;
    }
  }
  DevBuf d_idx;
  R0H_TRY(d_idx.alloc(ctx, idx.size() * 4));
  R0H_TRY(stage_h2d(ctx, d_idx->ptr, idx.data(), idx.size() * 4));
  std::vector<std::vector<uint32_t>> opened(n_trees);
  for (uint32_t t = 0; t < n_trees; t++) {
    DevBuf packed;  // back to the pool behind the read-back
    opened[t].resize(opened_words(*trees[t], nq));
    R0H_TRY(packed.alloc(ctx, opened[t].size() * 4));
    R0H_TRY(open_tree(ctx, *trees[t], u32(d_idx.get()) + (size_t)t * nq, nq, u32(packed.get())));
    R0H_TRY(r0h_buf_d2h(ctx, packed.get(), 0, opened[t].data(), opened[t].size() * 4));
    if (trees[t]->top_levels) R0H_TRY(merkle_open_top_verdict("r0h_proof_finish", opened[t].data() + opened[t].size() - 2, idx.data() + (size_t)t * nq));
  }
  for (uint32_t q = 0; q < nq; q++)
    for (uint32_t t = 0; t < n_trees; t++) {
      const size_t w = trees[t]->mp.opening_words();
      st.io.write(opened[t].data() + (size_t)q * w, w);
    }
  return nullptr;
}

// The tail block read back -- the one wait of the steps that ran on the device transcript -- then the verdicts the host draws from
// it, and its parts appended to the seal in the order the host steps write them
static const char* tail_collect(r0h_proof& st) {
  r0h_ctx* ctx = st.ctx;
  const TailLayout& at = st.tail_at;
  const std::vector<const Tree*> trees = proof_trees(st);
  const uint32_t nq = R0H_QUERIES, n_trees = (uint32_t)trees.size();
  std::vector<uint32_t> host(at.seal_words);
  R0H_TRY(r0h_buf_d2h(ctx, st.tail.get(), 0, host.data(), host.size() * 4));
  st.iop.reset();
  st.tail.reset();
  WriteIop& io = st.io;
  if (at.late) {  // before any other verdict: words that are no field elements make every later one meaningless
    const uint32_t n_late = st.circ->n_late, n_early = st.circ->n_global - n_late, bad = host[at.late_report];
    R0H_REQUIRE(bad <= n_late, "r0h_proof_finish_collect: the late report word %u names none of the %u late public inputs", bad, n_late);
    R0H_REQUIRE(!bad, "r0h_proof_finish_collect: late public input %u is not canonical", bad ? bad - 1 : 0);
    if (n_late) {
      memcpy(st.global.data() + n_early, host.data() + at.late_words, (size_t)n_late * 4);
      memcpy(io.proof.data() + st.seal_globals_at + n_early, host.data() + at.late_words, (size_t)n_late * 4);
    }
  }
  if (at.head) {
    const uint32_t report = host[at.report];
    R0H_REQUIRE(report <= st.divide_combo.size(), "prove_segment: the DEEP report word %u names none of the %zu divisions", report, st.divide_combo.size());
    R0H_REQUIRE(!report, "prove_segment: DEEP quotient of combo %u has a non-zero remainder (witness violates the taps?)", st.divide_combo[report ? report - 1 : 0]);
    if (at.begin) {  // DATA's top layer follows CODE's in the seal, as the host form writes it at the begin
      io.write(host.data() + at.data_top, at.data_root - at.data_top);
      memcpy(st.data_root, host.data() + at.data_root, 32);
      st.data_root_home = true;
    }
    io.write(host.data() + at.accum_top, at.check_top - at.accum_top);
    io.write(host.data() + at.check_top, at.coeff_u - at.check_top);
    io.write(host.data() + at.coeff_u, at.report - at.coeff_u);
  }
  for (uint32_t t = 0; t < n_trees; t++)
    if (trees[t]->top_levels)
      R0H_TRY(merkle_open_top_verdict("r0h_proof_finish", host.data() + at.opened[t] + (size_t)nq * trees[t]->mp.opening_words(), host.data() + at.idx + (size_t)t * nq));
  for (size_t r = 0; r < st.rounds.size(); r++) io.write(host.data() + at.round_top[r], 8 * st.rounds[r].tree.mp.top_size);
  io.write(host.data() + at.final_coeffs, at.idx - at.final_coeffs);
  for (uint32_t q = 0; q < nq; q++)
    for (uint32_t t = 0; t < n_trees; t++) {
      const size_t w = trees[t]->mp.opening_words();
      io.write(host.data() + at.opened[t] + (size_t)q * w, w);
    }
  return nullptr;
}

static const char* require_finishable(const r0h_proof& st, const char* caller) {
  R0H_REQUIRE(st.mix_drawn, "%s: this circuit has late public inputs: r0h_proof_late comes first", caller);
  R0H_REQUIRE(st.io.suite->fn() == st.ctx->hashfn, "%s: the proof was begun under the %s hash suite, its context is now on %s", caller, hashfn_name(st.io.suite->fn()),
              hashfn_name(st.ctx->hashfn));
  return nullptr;
}
// Steps 3-8 of DESIGN.md 2, each under its own phase marks, and between them the hand-over of the transcript where the context asks
// for one: before step 3 with the tail's head (r0h_ctx_set_device_finish; whatever it says goes, since what is handed over stays so),
// before step 7 with the tail alone (r0h_ctx_set_device_transcript), earlier still by r0h_proof_late_device, or never.  Behind the
// hand-over nothing waits for the stream (but the witness checker, where it is on) and the host generator is not touched again.
static const char* proof_steps(r0h_proof& st, const r0h_buf* accum) {
  const r0h_ctx* ctx = st.ctx;
  R0H_REQUIRE(ctx->device_finish || !st.late_device,
              "r0h_proof_finish: the late public inputs went to the device generator (r0h_proof_late_device) and r0h_ctx_set_device_finish is off now");
  if (ctx->device_finish && !st.iop) R0H_TRY(tail_open(st, true));
  R0H_TRY(commit_accum(st, accum));
  R0H_TRY(commit_check(st));
  R0H_TRY(evaluate_at_z(st));
  R0H_TRY(deep(st));
  if (ctx->device_transcript && !st.iop) R0H_TRY(tail_open(st, false));
  R0H_TRY(fri_commit(st));
  R0H_TRY(queries(st));
  return nullptr;
}
// r0h_ctx_set_device_finish: the steps enqueued on the proof's stream, the end of the last phase marked behind them ...
static const char* proof_finish_enqueue(r0h_proof& st, const r0h_buf* accum) {
  R0H_TRY(require_finishable(st, "r0h_proof_finish"));
  R0H_REQUIRE(!st.enqueued, "r0h_proof_finish_enqueue: the proof has been enqueued already");
  R0H_TRY(proof_steps(st, accum));
  profile_end(st.ctx);
  st.enqueued = true;
  return nullptr;
}
// ... then the read-back (one wait), the host's verdicts, the seal, and the profile closes (a second wait, of a stream that has drained)
static const char* proof_finish_collect(r0h_proof& st, std::vector<uint32_t>& seal) {
  R0H_REQUIRE(st.enqueued, "r0h_proof_finish_collect: the proof has not been enqueued (r0h_proof_finish_enqueue comes first)");
  st.enqueued = false;  // the stream has drained once the read-back returns, whatever it brings
  R0H_TRY(tail_collect(st));
  R0H_TRY(profile_collect(st.ctx));
  seal.swap(st.io.proof);
  return nullptr;
}

// The seal is the transcript's written words.  Under r0h_ctx_set_device_finish the two halves above, one after the other (the last
// phase ends before the read-back); otherwise the same steps, the tail brought home if there is one, and the profile closed.
static const char* proof_finish(r0h_proof& st, const r0h_buf* accum, std::vector<uint32_t>& seal) {
  R0H_TRY(require_finishable(st, "r0h_proof_finish"));
  if (st.ctx->device_finish) {
    R0H_TRY(proof_finish_enqueue(st, accum));
    return proof_finish_collect(st, seal);
  }
  R0H_TRY(proof_steps(st, accum));
  if (st.iop) R0H_TRY(tail_collect(st));
  R0H_TRY(profile_close(st.ctx));
  seal.swap(st.io.proof);
  return nullptr;
}

// the entry points' common checks and their way out
static const char* require_po2(const char* caller, uint32_t po2) {
  R0H_REQUIRE(po2 >= 9 && po2 <= R0H_MAX_PO2, "%s: po2 %u outside [9, %u]", caller, po2, R0H_MAX_PO2);
  return nullptr;
}
static const char* seal_copy_out(const char* caller, const std::vector<uint32_t>& seal, uint32_t* seal_out, size_t seal_cap, size_t* seal_words_out) {
  *seal_words_out = seal.size();
  R0H_REQUIRE(seal.size() <= seal_cap || !seal_out, "%s: seal needs %zu words, capacity is %zu", caller, seal.size(), seal_cap);
  if (seal_out) memcpy(seal_out, seal.data(), seal.size() * 4);
  return nullptr;
}

}  // namespace r0h

using namespace r0h;

extern "C" {

// r0h_prove_segment == r0h_code_commit_new + r0h_prove_segment_committed: `code` columns (the proof commits them itself) or `cc`
static const char* prove_segment_impl(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_code_commit* cc,
                                      const r0h_buf* data, const uint32_t* global, uint32_t* seal_out, size_t seal_cap, size_t* seal_words_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && c && (code || cc) && data && seal_words_out, "r0h_prove_segment: NULL argument");
  R0H_REQUIRE(global || r0h_circuit_n_global(c) == 0, "r0h_prove_segment: global is NULL");
  R0H_TRY(require_po2("r0h_prove_segment", po2));
  R0H_REQUIRE(c->has_column_program, "r0h_prove_segment: the circuit has no accumulation program; drive the per-op entry points with your own accum step");
  R0H_TRY_HIP(hipSetDevice(ctx->device));
  std::vector<uint32_t> seal;
  {
    r0h_proof st(ctx, c, po2, code, cc);
    R0H_TRY(proof_begin(st, data, global));
    if (c->n_late) R0H_TRY(proof_late(st, global + (c->n_global - c->n_late)));
    DevBuf accum;
    R0H_TRY(accum.alloc(ctx, ((size_t)c->group_size[R0H_GROUP_ACCUM] << po2) * 4));
    R0H_TRY(r0h_accum_public(ctx, c, po2, st.code->witness, data, st.global.data(), st.mix.data(), accum.get()));
    R0H_TRY(proof_finish(st, accum.get(), seal));
  }
  return seal_copy_out("r0h_prove_segment", seal, seal_out, seal_cap, seal_words_out);
  R0H_GUARD_END
}

static const char* proof_begin_impl(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_code_commit* cc,
                                    const r0h_buf* data, const uint32_t* global, uint32_t* mix_out, r0h_proof** out, const r0h_buf* data_top = nullptr,
                                    uint32_t top_levels = 0) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && c && (code || cc) && data && out, "r0h_proof_begin: NULL argument");
  R0H_REQUIRE((global || r0h_circuit_n_global(c) == 0) && (mix_out || r0h_circuit_n_mix(c) == 0 || c->n_late), "r0h_proof_begin: NULL globals / mix_out");
  R0H_TRY(require_po2("r0h_proof_begin", po2));
  R0H_TRY_HIP(hipSetDevice(ctx->device));
  std::unique_ptr<r0h_proof> st(new r0h_proof(ctx, c, po2, code, cc));
  R0H_TRY(proof_begin(*st, data, global, data_top, top_levels));
  if (c->n_mix && st->mix_drawn && mix_out) memcpy(mix_out, st->mix.data(), (size_t)c->n_mix * 4);
  *out = st.release();
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_prove_segment(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data,
                              const uint32_t* global, uint32_t* seal_out, size_t seal_cap, size_t* seal_words_out) {
  R0H_REQUIRE(code, "r0h_prove_segment: NULL argument");
  return prove_segment_impl(ctx, c, po2, code, nullptr, data, global, seal_out, seal_cap, seal_words_out);
}
const char* r0h_prove_segment_committed(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_code_commit* code, const r0h_buf* data,
                                        const uint32_t* global, uint32_t* seal_out, size_t seal_cap, size_t* seal_words_out) {
  R0H_REQUIRE(code, "r0h_prove_segment_committed: NULL argument");
  return prove_segment_impl(ctx, c, po2, nullptr, code, data, global, seal_out, seal_cap, seal_words_out);
}

const char* r0h_proof_begin(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data,
                            const uint32_t* global, uint32_t* mix_out, r0h_proof** out) {
  R0H_REQUIRE(code, "r0h_proof_begin: NULL argument");
  return proof_begin_impl(ctx, c, po2, code, nullptr, data, global, mix_out, out);
}
const char* r0h_proof_begin_committed(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_code_commit* code, const r0h_buf* data,
                                      const uint32_t* global, uint32_t* mix_out, r0h_proof** out) {
  R0H_REQUIRE(code, "r0h_proof_begin_committed: NULL argument");
  return proof_begin_impl(ctx, c, po2, nullptr, code, data, global, mix_out, out);
}

// The DATA commitment carried as its tree top: taken from a proof in flight, and a proof begun from it without hashing (merkle_top.hip)
const char* r0h_proof_data_top(const r0h_proof* proof, uint32_t levels, r0h_buf* top_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(proof && top_out, "r0h_proof_data_top: NULL argument");
  const Tree& t = proof->g_data.tree;
  R0H_REQUIRE(!t.top_levels || t.top_levels <= levels, "r0h_proof_data_top: this proof keeps its DATA tree to %u levels above the leaves, a top at %u levels needs more", t.top_levels,
              levels);
  return merkle_top_copy(proof->ctx, t.nodes.get(), (uint32_t)t.mp.rows, levels, top_out, "r0h_proof_data_top");
  R0H_GUARD_END
}
const char* r0h_proof_begin_committed_top(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_code_commit* code, const r0h_buf* data,
                                          const uint32_t* global, const r0h_buf* top, uint32_t levels, uint32_t* mix_out, r0h_proof** out) {
  R0H_REQUIRE(code && top, "r0h_proof_begin_committed_top: NULL argument");
  R0H_REQUIRE(levels >= 1 && levels <= R0H_MERKLE_TOP_MAX_LEVELS, "r0h_proof_begin_committed_top: levels %u outside [1, %u]", levels,
              (unsigned)R0H_MERKLE_TOP_MAX_LEVELS);  // (and at most the tree's path digests: merkle_top_copy, by name)
  return proof_begin_impl(ctx, c, po2, nullptr, code, data, global, mix_out, out, top, levels);
}

// ---- a proof's first half enqueued (include/r0hip.h): the hand-over before the DATA commitment.  What is refused is refused before
// anything is launched; an error behind that consumes the proof, once what was launched has run (it reads the caller's buffers).
static const char* require_begin_enqueue(const char* caller, r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_code_commit* code, const r0h_buf* data,
                                         const uint32_t* global, const void* out) {
  R0H_REQUIRE(ctx && c && data && out, "%s: NULL argument", caller);
  R0H_REQUIRE(code, "%s: no CODE commitment: the columns forms commit CODE with a read-back that waits; commit it once with r0h_code_commit_new", caller);
  R0H_REQUIRE(global || r0h_circuit_n_global(c) == 0, "%s: global is NULL", caller);
  R0H_REQUIRE(ctx->device_finish, "%s: the context has r0h_ctx_set_device_finish off: the steps behind the DATA commitment would ask the host generator", caller);
  return require_po2(caller, po2);
}
static const char* proof_begin_enqueue_impl(const char* caller, r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_code_commit* code, const r0h_buf* data,
                                            const uint32_t* global, r0h_buf* mix_out, r0h_proof** out, const r0h_buf* top, uint32_t levels) {
  R0H_GUARD_BEGIN
  R0H_TRY(require_begin_enqueue(caller, ctx, c, po2, code, data, global, out));
  R0H_REQUIRE(!mix_out || mix_out->bytes >= (size_t)c->n_mix * 4, "%s: mix_out holds %zu words, the circuit draws %u", caller, mix_out ? mix_out->bytes / 4 : (size_t)0, c->n_mix);
  R0H_TRY_HIP(hipSetDevice(ctx->device));
  std::unique_ptr<r0h_proof> st(new r0h_proof(ctx, c, po2, nullptr, code));
  const char* err = proof_begin(*st, data, global, top, levels, true, mix_out);
  if (err) {
    (void)ctx_wait(ctx);
    return err;
  }
  *out = st.release();
  return nullptr;
  R0H_GUARD_END
}
const char* r0h_proof_begin_committed_enqueue(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_code_commit* code, const r0h_buf* data, const uint32_t* global,
                                              r0h_buf* mix_out, r0h_proof** out) {
  return proof_begin_enqueue_impl("r0h_proof_begin_committed_enqueue", ctx, c, po2, code, data, global, mix_out, out, nullptr, 0);
}
const char* r0h_proof_begin_committed_top_enqueue(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_code_commit* code, const r0h_buf* data, const uint32_t* global,
                                                  const r0h_buf* top, uint32_t levels, r0h_buf* mix_out, r0h_proof** out) {
  R0H_REQUIRE(top, "r0h_proof_begin_committed_top_enqueue: NULL argument");
  R0H_REQUIRE(levels >= 1 && levels <= R0H_MERKLE_TOP_MAX_LEVELS, "r0h_proof_begin_committed_top_enqueue: levels %u outside [1, %u]", levels, (unsigned)R0H_MERKLE_TOP_MAX_LEVELS);
  return proof_begin_enqueue_impl("r0h_proof_begin_committed_top_enqueue", ctx, c, po2, code, data, global, mix_out, out, top, levels);
}
// begin-enqueue + the late inputs (host words: they go up through the pinned ring) + the accumulation from the tail's mix words +
// r0h_proof_finish_enqueue.  The proof keeps the ACCUM witness (and a log-derivative circuit's public inputs on the device) until the collect.
const char* r0h_prove_segment_committed_enqueue(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_code_commit* code, const r0h_buf* data, const uint32_t* global,
                                                r0h_proof** out) {
  R0H_GUARD_BEGIN
  const char* const caller = "r0h_prove_segment_committed_enqueue";
  R0H_TRY(require_begin_enqueue(caller, ctx, c, po2, code, data, global, out));
  R0H_REQUIRE(c->has_column_program, "%s: the circuit has no accumulation program; drive the per-op entry points with your own accum step", caller);
  const uint32_t n_early = c->n_global - c->n_late;
  for (uint32_t i = 0; i < c->n_late; i++) R0H_REQUIRE(global[n_early + i] < P, "%s: late public input %u is not canonical", caller, i);
  R0H_TRY_HIP(hipSetDevice(ctx->device));
  std::unique_ptr<r0h_proof> st(new r0h_proof(ctx, c, po2, nullptr, code));
  const char* err = [&]() -> const char* {
    R0H_TRY(proof_begin(*st, data, global, nullptr, 0, true));
    if (c->n_late) R0H_TRY(late_enqueue(*st, nullptr, global + n_early, nullptr));
    R0H_TRY(st->own_accum.alloc(ctx, ((size_t)c->group_size[R0H_GROUP_ACCUM] << po2) * 4));
    if (c->logup.accs.empty()) {
      R0H_TRY(r0h_accum_mixbuf(ctx, c, po2, code->witness, data, st->tail.get(), st->tail_at.mix, st->own_accum.get()));
    } else {
      R0H_TRY(st->own_globals.alloc(ctx, (size_t)c->n_global * 4));
      R0H_TRY(stage_h2d(ctx, st->own_globals->ptr, global, (size_t)c->n_global * 4));
      const r0h_buf mix = buf_view(st->tail.get(), st->tail_at.mix * 4, (size_t)c->n_mix * 4);
      R0H_TRY(r0h_accum_public_device(ctx, c, po2, code->witness, data, st->own_globals.get(), &mix, st->own_accum.get()));
    }
    return proof_finish_enqueue(*st, st->own_accum.get());
  }();
  if (err) {
    (void)ctx_wait(ctx);
    return err;
  }
  *out = st.release();
  return nullptr;
  R0H_GUARD_END
}
const char* r0h_prove_segment_collect(r0h_proof* proof, uint32_t* seal_out, size_t seal_cap, size_t* seal_words_out) {
  return r0h_proof_finish_collect(proof, seal_out, seal_cap, seal_words_out);
}
// the DATA root where it stands on the device (node 1 of the group's tree): eight words to `out`, device to device, no wait
const char* r0h_proof_data_root_device(const r0h_proof* proof, r0h_buf* out, size_t word_offset) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(proof && out, "r0h_proof_data_root_device: NULL argument");
  R0H_TRY(require_words_in("r0h_proof_data_root_device", "root", out, word_offset, 8));
  R0H_TRY_HIP(hipSetDevice(proof->ctx->device));
  return copy_words(proof->ctx, out, word_offset, proof->g_data.tree.nodes.get(), 8, 8);
  R0H_GUARD_END
}

// Commit the CODE group once (the sequencer's commit_code: code_commit above) and keep it, with a copy of the columns.
const char* r0h_code_commit_new(r0h_ctx* ctx, const r0h_buf* code, uint32_t count, uint32_t po2, r0h_code_commit** out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && code && out, "r0h_code_commit_new: NULL argument");
  R0H_REQUIRE(count >= 1, "r0h_code_commit_new: the CODE group has no columns");
  R0H_TRY(require_po2("r0h_code_commit_new", po2));
  R0H_TRY_HIP(hipSetDevice(ctx->device));
  std::unique_ptr<r0h_code_commit, const char* (*)(r0h_code_commit*)> cc(new r0h_code_commit(count, po2), r0h_code_commit_free);
  cc->ctx = ctx;
  ctx_retain(ctx);
  R0H_TRY(code_commit(ctx, *cc, code));
  const size_t bytes = ((size_t)count << po2) * 4;
  r0h_buf* copy = nullptr;
  R0H_TRY(r0h_buf_alloc(ctx, bytes, &copy));
  cc->kept_columns.reset(copy);
  cc->witness = copy;
  R0H_TRY_HIP(hipMemcpyAsync(copy->ptr, code->ptr, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  R0H_TRY_HIP(ctx_wait(ctx));
  // Everything has succeeded: the group's three buffers leave the pool's ownership.  They are long-lived and read from other
  // contexts' streams, so on release they go back to the device (hipFree waits for every stream), not into this context's
  // stream-ordered pool
  for (r0h_buf* b : {cc->g.coeffs.get(), cc->g.evaluated.get(), cc->g.tree.nodes.get()}) { b->pooled = false; b->owned = true; }
  *out = cc.release();
  return nullptr;
  R0H_GUARD_END
}
const char* r0h_code_commit_free(r0h_code_commit* cc) {
  if (!cc) return nullptr;
  // a proof on another context may still be reading these buffers on its own stream: the caller frees a commitment only after
  // the proofs that use it have returned (r0h_prove_segment_committed / r0h_proof_finish block until the seal is out)
  r0h_ctx* ctx = cc->ctx;
  delete cc;  // its buffers go with it
  if (ctx) ctx_release(ctx);
  return nullptr;
}
const char* r0h_code_commit_columns(const r0h_code_commit* cc, const r0h_buf** columns_out) {
  R0H_REQUIRE(cc && columns_out && cc->witness, "r0h_code_commit_columns: NULL argument");
  *columns_out = cc->witness;
  return nullptr;
}
const char* r0h_code_commit_root(const r0h_code_commit* cc, uint32_t root_out[8]) {
  R0H_REQUIRE(cc && root_out, "r0h_code_commit_root: NULL argument");
  memcpy(root_out, cc->top.root(), 32);
  return nullptr;
}

const char* r0h_proof_finish(r0h_proof* proof, const r0h_buf* accum, uint32_t* seal_out, size_t seal_cap, size_t* seal_words_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(proof && accum && seal_words_out, "r0h_proof_finish: NULL argument");
  R0H_TRY_HIP(hipSetDevice(proof->ctx->device));
  std::vector<uint32_t> seal;
  const char* err = proof_finish(*proof, accum, seal);
  r0h_proof_abort(proof);  // consumed either way (an error under r0h_ctx_set_device_finish may leave steps in flight: they run out first)
  return err ? err : seal_copy_out("r0h_proof_finish", seal, seal_out, seal_cap, seal_words_out);
  R0H_GUARD_END
}

const char* r0h_proof_data_root(const r0h_proof* proof, uint32_t root_out[8]) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(proof && root_out, "r0h_proof_data_root: NULL argument");
  if (!proof->data_root_home) {  // begun by r0h_proof_begin_committed[_top]_enqueue: node 1 comes home now, eight words and a wait
    R0H_TRY_HIP(hipSetDevice(proof->ctx->device));
    R0H_TRY(r0h_buf_d2h(proof->ctx, proof->g_data.tree.nodes.get(), 32, proof->data_root, 32));
    proof->data_root_home = true;
    proof->root_read_back = true;
  }
  memcpy(root_out, proof->data_root, 32);
  return nullptr;
  R0H_GUARD_END
}
const char* r0h_proof_late(r0h_proof* proof, const uint32_t* late_globals, uint32_t* mix_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(proof && (mix_out || !proof->circ->n_mix), "r0h_proof_late: NULL argument");
  R0H_REQUIRE(proof->circ->n_late, "r0h_proof_late: this circuit has no late public inputs");
  R0H_TRY_HIP(hipSetDevice(proof->ctx->device));
  R0H_TRY(proof_late(*proof, late_globals));
  if (proof->circ->n_mix) memcpy(mix_out, proof->mix.data(), (size_t)proof->circ->n_mix * 4);
  return nullptr;
  R0H_GUARD_END
}
// r0h_proof_late with the late public inputs and the mix on the device (include/r0hip.h): nothing waits, nothing is read back
const char* r0h_proof_late_device(r0h_proof* proof, const r0h_buf* late, r0h_buf* mix_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(proof, "r0h_proof_late_device: NULL argument");
  R0H_TRY_HIP(hipSetDevice(proof->ctx->device));
  return proof_late_device(*proof, late, mix_out);
  R0H_GUARD_END
}
const char* r0h_proof_globals(const r0h_proof* proof, uint32_t* globals_out) {
  R0H_REQUIRE(proof && globals_out, "r0h_proof_globals: NULL argument");
  memcpy(globals_out, proof->global.data(), proof->global.size() * 4);
  return nullptr;
}

// The two halves of r0h_proof_finish under r0h_ctx_set_device_finish (include/r0hip.h)
const char* r0h_proof_finish_enqueue(r0h_proof* proof, const r0h_buf* accum) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(proof && accum, "r0h_proof_finish_enqueue: NULL argument");
  R0H_REQUIRE(!proof->enqueued, "r0h_proof_finish_enqueue: the proof has been enqueued already");
  const char* err = nullptr;
  if (!proof->ctx->device_finish) err = make_error("r0h_proof_finish_enqueue: the proof's context has r0h_ctx_set_device_finish off: only r0h_proof_finish takes this proof");
  if (!err) {
    R0H_TRY_HIP(hipSetDevice(proof->ctx->device));
    err = proof_finish_enqueue(*proof, accum);
  }
  if (err) r0h_proof_abort(proof);  // consumed, as by r0h_proof_finish; what was enqueued before the error has run when the buffers go
  return err;
  R0H_GUARD_END
}
const char* r0h_proof_finish_collect(r0h_proof* proof, uint32_t* seal_out, size_t seal_cap, size_t* seal_words_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(proof && seal_words_out, "r0h_proof_finish_collect: NULL argument");
  R0H_REQUIRE(proof->enqueued, "r0h_proof_finish_collect: the proof has not been enqueued (r0h_proof_finish_enqueue comes first)");
  R0H_TRY_HIP(hipSetDevice(proof->ctx->device));
  std::vector<uint32_t> seal;
  const char* err = proof_finish_collect(*proof, seal);
  r0h_proof_abort(proof);  // consumed either way
  return err ? err : seal_copy_out("r0h_proof_finish_collect", seal, seal_out, seal_cap, seal_words_out);
  R0H_GUARD_END
}

const char* r0h_proof_abort(r0h_proof* proof) {
  if (!proof) return nullptr;
  // steps may be in flight on its stream (enqueued and not collected, or an enqueue that ended in an error): they read the caller's
  // buffers, so they have run before anything is released
  if (proof->enqueued || proof->iop) {
    (void)hipSetDevice(proof->ctx->device);
    // (the stream's own answer: nothing an earlier call enqueued for this proof, or for another on its context, is missed)
    const bool idle = proof->root_read_back && hipStreamQuery(proof->ctx->stream) == hipSuccess;
    if (!idle) {
      (void)hipGetLastError();
      (void)ctx_wait(proof->ctx);
    }
  }
  delete proof;
  return nullptr;
}
// Give back the DATA group's evaluations on the 4N coset (4/5 of what a proof holds between its phases): the commitment -- the Merkle
// nodes -- and the coefficients stay, r0h_proof_finish evaluates again (the same words: one expanding NTT).
const char* r0h_proof_shrink(r0h_proof* proof, size_t* bytes_freed_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(proof, "r0h_proof_shrink: NULL argument");
  size_t freed = 0;
  Group& g_data = proof->g_data;
  if (g_data.evaluated) {
    R0H_TRY_HIP(hipSetDevice(proof->ctx->device));
    R0H_TRY_HIP(ctx_wait(proof->ctx));  // the block goes back to the pool: nothing in flight may still read it
    freed = g_data.evaluated->bytes;
    g_data.evaluated.reset();
    g_data.tree.matrix = nullptr;
  }
  if (bytes_freed_out) *bytes_freed_out = freed;
  return nullptr;
  R0H_GUARD_END
}
// what the proof owns on the device: its groups, CODE only where it committed the columns itself, and what a proof submitted whole
// (r0h_prove_segment_committed_enqueue) keeps until its collect: the ACCUM witness and the device copy of the public inputs
size_t r0h_proof_resident_bytes(const r0h_proof* proof) {
  if (!proof) return 0;
  size_t kept = 0;
  for (const r0h_buf* b : {proof->own_accum.get(), proof->own_globals.get()}) kept += b ? b->bytes : 0;
  return proof->own_code.g.bytes() + proof->g_accum.bytes() + proof->g_data.bytes() + proof->g_check.bytes() + kept;
}

// The control root of a program at one trace size: the Merkle root of its committed CODE group (risc0 keeps one such root per
// po2 -- the control id -- and `verify` compares the seal's CODE commitment with it).  The sequencer's commit_code: code_commit above.
const char* r0h_code_root(r0h_ctx* ctx, const r0h_buf* code, uint32_t count, uint32_t po2, uint32_t root_out[8]) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && code && root_out, "r0h_code_root: NULL argument");
  R0H_REQUIRE(count >= 1, "r0h_code_root: the CODE group has no columns");
  R0H_TRY(require_po2("r0h_code_root", po2));
  R0H_TRY_HIP(hipSetDevice(ctx->device));
  r0h_code_commit cc(count, po2);
  R0H_TRY(code_commit(ctx, cc, code));
  memcpy(root_out, cc.top.root(), 32);
  return nullptr;
  R0H_GUARD_END
}

// ---- the small kernels of steps 5 and 6 on their own (deep_points_table, interpolate_regs, subtract_heads): what the sequencer's inputs
// are by construction -- register sizes, taps inside their tables -- is looked at here, before anything is launched
const char* r0h_deep_points_buf(r0h_ctx* ctx, r0h_buf* points_out, const r0h_buf* z_buf, size_t z_word_offset, const uint32_t* wpow, uint32_t n_backs) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(n_backs >= 1 && n_backs <= 64, "r0h_deep_points_buf: %u backs (1 to 64)", n_backs);
  R0H_REQUIRE(ctx && points_out && z_buf && wpow, "r0h_deep_points_buf: NULL argument");
  for (uint32_t i = 0; i < n_backs; i++) R0H_REQUIRE(wpow[i] < P, "r0h_deep_points_buf: wpow[%u] not canonical", i);
  R0H_TRY(require_words_in("r0h_deep_points_buf", "z", z_buf, z_word_offset, 4));
  R0H_TRY(require_words_in("r0h_deep_points_buf", "point table", points_out, 0, 4 * (size_t)(n_backs + 1)));
  DevBuf d_wpow;  // back to the pool once the kernel that reads it is enqueued
  R0H_TRY(d_wpow.alloc(ctx, (size_t)n_backs * 4));
  return deep_points_table(ctx, u32(points_out), u32(z_buf) + z_word_offset, u32(d_wpow.get()), wpow, n_backs);
  R0H_GUARD_END
}

const char* r0h_poly_interpolate_host(const uint32_t* xs, const uint32_t* ys, uint32_t n, uint32_t* out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(xs && ys && out, "r0h_poly_interpolate_host: NULL argument");
  R0H_REQUIRE(n >= 1 && n <= 64, "r0h_poly_interpolate_host: %u points (1 to 64)", n);
  for (size_t k = 0; k < 4 * (size_t)n; k++) R0H_REQUIRE(xs[k] < P && ys[k] < P, "r0h_poly_interpolate_host: point %zu not canonical", k / 4);
  for (uint32_t i = 0; i < n; i++)
    for (uint32_t j = 0; j < i; j++) R0H_REQUIRE(memcmp(xs + 4 * i, xs + 4 * j, 16) != 0, "r0h_poly_interpolate_host: points %u and %u are equal", j, i);
  poly_interpolate((Fp4*)out, (const Fp4*)xs, (const Fp4*)ys, n);
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_poly_interpolate_regs(r0h_ctx* ctx, r0h_buf* coeff_u_out, const r0h_buf* eval_u, const r0h_buf* points_buf, size_t points_word_offset, uint32_t n_points,
                                      const uint32_t* tap_pt, const uint32_t* regs, uint32_t n_regs, uint32_t n_taps) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && coeff_u_out && eval_u && points_buf && tap_pt && regs, "r0h_poly_interpolate_regs: NULL argument");
  R0H_REQUIRE(n_regs >= 1 && n_regs <= n_taps && n_taps <= (1u << 24), "r0h_poly_interpolate_regs: %u registers over %u taps", n_regs, n_taps);
  std::vector<uint32_t> owner(n_taps, 0u);  // 1 + the register a tap belongs to
  for (uint32_t r = 0; r < n_regs; r++) {
    const uint32_t first = regs[2 * r], size = regs[2 * r + 1];
    R0H_REQUIRE(size >= 1 && size <= 64, "r0h_poly_interpolate_regs: register %u has %u taps (1 to 64)", r, size);
    R0H_REQUIRE(first <= n_taps && size <= n_taps - first, "r0h_poly_interpolate_regs: register %u runs past the %u taps", r, n_taps);
    for (uint32_t t = first; t < first + size; t++) {
      R0H_REQUIRE(!owner[t], "r0h_poly_interpolate_regs: registers %u and %u overlap at tap %u", owner[t] - 1, r, t);
      owner[t] = r + 1;
    }
  }
  for (uint32_t t = 0; t < n_taps; t++) R0H_REQUIRE(tap_pt[t] < n_points, "r0h_poly_interpolate_regs: tap %u names point %u of a table of %u", t, tap_pt[t], n_points);
  R0H_TRY(require_words_in("r0h_poly_interpolate_regs", "point table", points_buf, points_word_offset, 4 * (size_t)n_points));
  R0H_TRY(require_words_in("r0h_poly_interpolate_regs", "evaluations", eval_u, 0, 4 * ((size_t)n_taps + R0H_CHECK_SIZE)));
  R0H_TRY(require_words_in("r0h_poly_interpolate_regs", "interpolants", coeff_u_out, 0, 4 * ((size_t)n_taps + R0H_CHECK_SIZE)));
  return interpolate_regs(ctx, u32(coeff_u_out), u32(eval_u), u32(points_buf) + points_word_offset, tap_pt, regs, n_regs, n_taps);
  R0H_GUARD_END
}

const char* r0h_deep_subtract_heads(r0h_ctx* ctx, r0h_buf* combos, uint32_t po2, uint32_t n_combos, const uint32_t* regs, uint32_t n_regs, uint32_t n_taps,
                                    const uint32_t* coeff_u_host, const r0h_buf* coeff_u_buf, size_t coeff_u_word_offset, const uint32_t* mix_host, const r0h_buf* mix_buf,
                                    size_t mix_word_offset) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && combos && (regs || !n_regs), "r0h_deep_subtract_heads: NULL argument");
  const bool host = coeff_u_host && mix_host && !coeff_u_buf && !mix_buf, dev = !coeff_u_host && !mix_host && coeff_u_buf && mix_buf;
  R0H_REQUIRE(host || dev, "r0h_deep_subtract_heads: coeff_u and the mix are both host words or both device words");
  R0H_REQUIRE(po2 <= MAX_DOMAIN_PO2, "r0h_deep_subtract_heads: po2 %u too large", po2);
  R0H_REQUIRE(n_combos < (1u << 16) && n_taps <= (1u << 24), "r0h_deep_subtract_heads: %u combos over %u taps", n_combos, n_taps);
  R0H_REQUIRE(((size_t)(n_combos + 1) << po2) * 4 < ((size_t)1 << 32), "r0h_deep_subtract_heads: combos buffer exceeds 32-bit word indexing");
  R0H_REQUIRE(((size_t)(n_combos + 1) << po2) * 16 <= combos->bytes, "r0h_deep_subtract_heads: %u combos and CHECK's exceed the combos buffer", n_combos);
  for (uint32_t r = 0; r < n_regs; r++) {
    const uint32_t combo = regs[3 * r], first = regs[3 * r + 1], size = regs[3 * r + 2];
    R0H_REQUIRE(combo < n_combos, "r0h_deep_subtract_heads: register %u names combo %u of %u", r, combo, n_combos);
    R0H_REQUIRE(size >= 1 && size <= 64 && size <= ((uint64_t)1 << po2), "r0h_deep_subtract_heads: register %u has %u taps (1 to 64, and no more than the combo's coefficients)", r, size);
    R0H_REQUIRE(first <= n_taps && size <= n_taps - first, "r0h_deep_subtract_heads: register %u runs past the %u taps", r, n_taps);
  }
  const size_t n_u = (size_t)n_taps + R0H_CHECK_SIZE;
  if (dev) {
    R0H_TRY(require_words_in("r0h_deep_subtract_heads", "interpolants", coeff_u_buf, coeff_u_word_offset, 4 * n_u));
    R0H_TRY(require_words_in("r0h_deep_subtract_heads", "mix", mix_buf, mix_word_offset, 4));
    return subtract_heads(ctx, combos, po2, n_combos, regs, n_regs, n_taps, nullptr, u32(coeff_u_buf) + coeff_u_word_offset, nullptr, u32(mix_buf) + mix_word_offset);
  }
  for (size_t k = 0; k < 4 * n_u; k++) R0H_REQUIRE(coeff_u_host[k] < P, "r0h_deep_subtract_heads: coeff_u word %zu not canonical", k);
  for (int q = 0; q < 4; q++) R0H_REQUIRE(mix_host[q] < P, "r0h_deep_subtract_heads: mix words must be canonical (< p)");
  const Fp4 mixv{{mix_host[0], mix_host[1], mix_host[2], mix_host[3]}};
  return subtract_heads(ctx, combos, po2, n_combos, regs, n_regs, n_taps, (const Fp4*)coeff_u_host, nullptr, &mixv, nullptr);
  R0H_GUARD_END
}

}  // extern "C"
