// Host-side seal verifier (no device work): replays the Fiat-Shamir transcript of prover.hip, re-evaluates the
// constraint program at the out-of-domain point from the opened interpolants, and checks every Merkle opening and FRI
// fold of the 50 queries.  Replaces risc0-zkp 3.0.4 verify/{mod.rs, merkle.rs, fri.rs, read_iop.rs} as reached from
// `receipt.verify(image_id)` (host/src/main.rs:622-624, verifier/src/main.rs:124-126) -- SURVEY.md 8(f) rank 1.
// Written against the seal layout the sequencer emits; the tests cross-check its verdicts with the CPU restatement's verifier.
// One seam lets a device help the PROVING side's own checks (verify_seals_batch / r0h_verify_seals_on): a second instantiation of the
// walk records the Merkle openings instead of hashing them, the batch is hashed by merkle_climb.hip (or here, without a context), and
// every comparison and verdict stays on the host.  The entry points of a verifier proper do not come near it.
#include "../../include/r0hip_circuit.h"
#include "seal_layout.hpp"

#include <algorithm>
#include <atomic>
#include <memory>
#include <stdexcept>
#include <thread>

namespace r0h {
namespace {

struct Reject { int code; };  // unwinds the verifier; never crosses the C ABI

// A position in the seal; the queries each get their own (their openings have a fixed size, so query q starts at a known word).
struct Cursor {
  const uint32_t* w;
  size_t n, pos;
  const uint32_t* take(size_t count) {
    if (count > n - pos) throw Reject{R0H_VERIFY_TRUNCATED};
    const uint32_t* p = w + pos;
    pos += count;
    return p;
  }
};

// The transcript and every hash go through the seal's hash suite (internal.hpp HashSuite).  Under SHA-256 a digest word is any 32-bit
// value, so "word < P" is asked of field-element positions only; under Poseidon2 it is asked of digests too, as before.
class SealReader {
 public:
  SealReader(const HashSuite& suite, const uint32_t* w, size_t n) : suite_(suite), rng_(suite.rng()), w_(w), n_(n) {}
  const uint32_t* take(size_t n) {
    if (n > n_ - pos_) throw Reject{R0H_VERIFY_TRUNCATED};
    const uint32_t* p = w_ + pos_;
    pos_ += n;
    return p;
  }
  const uint32_t* take_elems(size_t n) {
    const uint32_t* p = take(n);
    for (size_t i = 0; i < n; i++)
      if (p[i] >= P) throw Reject{R0H_VERIFY_BAD_ELEM};
    return p;
  }
  const uint32_t* take_digests(size_t n) { return suite_.digests_are_elems() ? take_elems(8 * n) : take(8 * n); }
  bool exhausted() const { return pos_ == n_; }
  Cursor cursor() const { return Cursor{w_, n_, pos_}; }
  void skip_to(size_t pos) { pos_ = pos < n_ ? pos : n_; }
  void commit(const uint32_t digest[8]) { rng_->mix(digest); }  // (Poseidon2: canonical, every digest is checked when it is read)
  void commit_elems(const uint32_t* e, size_t n) {
    uint32_t d[8];
    suite_.hash_elems(e, n, d);
    commit(d);
  }
  uint32_t elem() { return rng_->elem(); }
  Fp4 ext() { return rng_->ext(); }
  uint32_t bits(uint32_t n) { return rng_->bits(n); }
  const HashSuite& suite() const { return suite_; }

 private:
  const HashSuite& suite_;
  std::unique_ptr<SuiteRng> rng_;
  const uint32_t* w_;
  size_t n_, pos_ = 0;
};

// An opening whose hashing is put off (the collecting verifier): where its packed words lie in the seal, its shape, the reject code of
// its tree and the digest its path must reach.  A seal's walk leaves them in seal order, query by query, with each query's own verdict.
struct Deferred {
  const uint32_t* values;  // `cols` values, then `path` sibling digests
  uint32_t cols, path, row;
  int reject;
  uint32_t want[8];
};
struct Collected {
  std::vector<Deferred> jobs;
  uint32_t first_job[R0H_QUERIES + 1] = {0};  // query q recorded jobs [first_job[q], first_job[q + 1])
  int walk[R0H_QUERIES] = {0};                // what the walk of query q ended with, its openings taken as good
  bool trailing = false;
};

// The verifier's view of one committed matrix: the elided top layer (read from the seal) folded down to the root.
class TreeVerifier {
 public:
  TreeVerifier(SealReader& io, size_t rows, size_t cols, int reject_code) : shape_(rows, cols), reject_(reject_code) {
    const size_t top_size = shape_.top_size;
    top_.assign(2 * top_size * 8, 0);
    memcpy(&top_[top_size * 8], io.take_digests(top_size), top_size * 32);  // Poseidon2: digest words are field elements
    for (size_t i = top_size; i-- > 1;) io.suite().hash_pair(&top_[2 * i * 8], &top_[(2 * i + 1) * 8], &top_[i * 8]);
    io.commit(&top_[8]);
  }
  // the opened row (cols_ canonical words) if its path leads to the committed top layer
  const uint32_t* open(Cursor& io, const HashSuite& k, size_t row) const {
    if (row >= shape_.rows) throw Reject{reject_};
    const uint32_t* values = io.take(shape_.cols);
    for (size_t i = 0; i < shape_.cols; i++)
      if (values[i] >= P) throw Reject{reject_};
    uint32_t cur[8];
    k.hash_elems(values, shape_.cols, cur);
    size_t node = row + shape_.rows;
    for (; node >= 2 * shape_.top_size; node >>= 1) {
      const uint32_t* sibling = io.take(8);
      for (int i = 0; i < 8 && k.digests_are_elems(); i++)
        if (sibling[i] >= P) throw Reject{R0H_VERIFY_BAD_ELEM};  // two word sequences must not name one digest
      uint32_t parent[8];
      if (node & 1) k.hash_pair(sibling, cur, parent); else k.hash_pair(cur, sibling, parent);
      memcpy(cur, parent, 32);
    }
    if (memcmp(&top_[node * 8], cur, 32) != 0) throw Reject{reject_};
    return values;
  }

  // The collecting form: every host check of open() in its order -- the row bound, canonical values, every sibling present and
  // (Poseidon2) canonical -- and no hashing.  The opening is recorded with this tree's reject code and the node of top_ its path must
  // reach; whoever hashes the batch makes the comparison open() ends with.
  const uint32_t* open_later(Cursor& io, const HashSuite& k, size_t row, std::vector<Deferred>& later) const {
    if (row >= shape_.rows) throw Reject{reject_};
    const uint32_t* values = io.take(shape_.cols);
    for (size_t i = 0; i < shape_.cols; i++)
      if (values[i] >= P) throw Reject{reject_};
    size_t node = row + shape_.rows;
    for (; node >= 2 * shape_.top_size; node >>= 1) {
      const uint32_t* sibling = io.take(8);
      for (int i = 0; i < 8 && k.digests_are_elems(); i++)
        if (sibling[i] >= P) throw Reject{R0H_VERIFY_BAD_ELEM};
    }
    Deferred d{values, (uint32_t)shape_.cols, (uint32_t)shape_.path_digests(), (uint32_t)row, reject_, {0}};
    memcpy(d.want, &top_[node * 8], 32);
    later.push_back(d);
    return values;
  }

  const uint32_t* root() const { return &top_[8]; }
  size_t opening_words() const { return shape_.opening_words(); }

 private:
  MerkleShape shape_;
  int reject_;
  std::vector<uint32_t> top_;
};

Fp4 horner(const Fp4* coeffs, size_t n, const Fp4& x) {
  Fp4 acc = fp4_zero();
  for (size_t i = n; i-- > 0;) acc = acc * x + coeffs[i];
  return acc;
}
Fp4 lift(uint32_t a) { Fp4 r = fp4_zero(); r.e[0] = a; return r; }

// risc0-zkp adapter.rs `PolyExtStepDef::step` over extension values: the constraint polynomial at z
Fp4 constraint_at_z(const r0h_circuit& c, const Fp4& poly_mix, const std::vector<Fp4>& taps_at_z, const uint32_t* global, const uint32_t* mix) {
  struct MixState { Fp4 tot, mul; };
  std::vector<Fp4> fp;
  std::vector<MixState> mx;
  fp.reserve(c.fp_step.size());
  mx.reserve(c.mix_step.size());
  for (const Step& s : c.steps) {
    switch (s.op) {
      case R0H_OP_CONST: fp.push_back(lift(enc(s.a))); break;
      case R0H_OP_GET: fp.push_back(taps_at_z[s.a]); break;
      case R0H_OP_GET_GLOBAL: fp.push_back(lift(s.a == 0 ? global[s.b] : mix[s.b])); break;
      case R0H_OP_ADD: fp.push_back(fp[s.a] + fp[s.b]); break;
      case R0H_OP_SUB: fp.push_back(fp[s.a] - fp[s.b]); break;
      case R0H_OP_MUL: fp.push_back(fp[s.a] * fp[s.b]); break;
      case R0H_OP_TRUE: mx.push_back({fp4_zero(), fp4_one()}); break;
      case R0H_OP_AND_EQZ: mx.push_back({mx[s.a].tot + mx[s.a].mul * fp[s.b], mx[s.a].mul * poly_mix}); break;
      case R0H_OP_AND_COND: mx.push_back({mx[s.a].tot + fp[s.b] * mx[s.c].tot * mx[s.a].mul, mx[s.a].mul * mx[s.c].mul}); break;
      default: break;
    }
  }
  return mx[c.ret].tot;
}

// COLLECT = false is the immediate verifier: every opening hashed where it is read, the queries on a few host threads, `collected`
// unused.  COLLECT = true walks the same seal with open_later in place of open, the queries one after the other on the calling thread
// (what is left of a query is a few hundred field operations), and returns with the openings in `collected` instead of a verdict on
// them; a Reject thrown before the queries is final in either form (no opening precedes it).
template <bool COLLECT>
void verify(const r0h_circuit& c, const HashSuite& k, const uint32_t* seal, size_t seal_words, uint32_t* po2_out, const uint32_t* expected_code_root,
            uint32_t* code_root_out, uint32_t* data_root_out = nullptr, Collected* collected = nullptr) {
  SealReader io(k, seal, seal_words);
  const uint32_t* global = io.take_elems((size_t)c.n_global + 1);
  const uint32_t po2 = dec(global[c.n_global]);
  if (po2 < 9 || po2 > 24) throw Reject{R0H_VERIFY_BAD_PO2};
  if (po2_out) *po2_out = po2;
  transcript_open(io, c, global, po2);  // (the late public inputs follow the DATA commitment)
  const size_t n = (size_t)1 << po2, domain = n * R0H_INV_RATE;
  const uint32_t n_taps = (uint32_t)c.taps.size(), n_regs = (uint32_t)c.regs.size(), n_combos = (uint32_t)c.combo_begin.size() - 1;
  const uint32_t n_u = n_taps + R0H_CHECK_SIZE;

  // commitments, in the order the prover made them
  std::unique_ptr<TreeVerifier> group[4];  // ACCUM, CODE, DATA, CHECK
  group[R0H_GROUP_CODE].reset(new TreeVerifier(io, domain, c.group_size[R0H_GROUP_CODE], R0H_VERIFY_MERKLE_GROUP));
  // risc0-zkp verify/mod.rs `check_code(po2, root)`: the CODE commitment is the program's identity at this trace size.  Without
  // this comparison a prover may commit any CODE columns (e.g. selectors that switch constraints off).
  if (code_root_out) memcpy(code_root_out, group[R0H_GROUP_CODE]->root(), 32);
  if (expected_code_root && memcmp(expected_code_root, group[R0H_GROUP_CODE]->root(), 32) != 0) throw Reject{R0H_VERIFY_CODE_ROOT};
  group[R0H_GROUP_DATA].reset(new TreeVerifier(io, domain, c.group_size[R0H_GROUP_DATA], R0H_VERIFY_MERKLE_GROUP));
  if (data_root_out) memcpy(data_root_out, group[R0H_GROUP_DATA]->root(), 32);
  if (c.n_late) io.commit_elems(global + (c.n_global - c.n_late), c.n_late);
  std::vector<uint32_t> mix(c.n_mix);
  for (uint32_t& m : mix) m = io.elem();
  group[R0H_GROUP_ACCUM].reset(new TreeVerifier(io, domain, c.group_size[R0H_GROUP_ACCUM], R0H_VERIFY_MERKLE_GROUP));
  const Fp4 poly_mix = io.ext();
  group[3].reset(new TreeVerifier(io, domain, R0H_CHECK_SIZE, R0H_VERIFY_MERKLE_GROUP));
  const Fp4 z = io.ext(), z4 = fp4_pow(z, 4);
  const uint32_t back_one = rou_rev(po2);

  // interpolant coefficients of every register (and the 16 check values at z^4)
  std::vector<Fp4> coeff_u(n_u);
  {
    const uint32_t* cu = io.take_elems(4 * (size_t)n_u);
    memcpy(coeff_u.data(), cu, 16 * (size_t)n_u);
    io.commit_elems(cu, 4 * (size_t)n_u);
  }
  std::vector<Fp4> tap_point(n_taps), taps_at_z(n_taps);
  for (uint32_t t = 0; t < n_taps; t++) tap_point[t] = scale(z, fpow(back_one, c.taps[t].back));
  for (const Reg& r : c.regs)
    for (uint32_t i = 0; i < r.size; i++) taps_at_z[r.first_tap + i] = horner(&coeff_u[r.first_tap], r.size, tap_point[r.first_tap + i]);

  // the constraint identity  C(z) == check(z) * (Z_H(3z)),  check(z) reassembled from its 4 x 4 split
  {
    const Fp4 lhs = constraint_at_z(c, poly_mix, taps_at_z, global, mix.data());
    Fp4 check = fp4_zero(), zr = fp4_one();
    for (uint32_t r = 0; r < 4; r++) {
      const uint32_t block = ((r & 1) << 1) | (r >> 1);  // the split polynomials sit in bit-reversed order
      Fp4 part = fp4_zero();
      for (uint32_t j = 4; j-- > 0;) {
        // part = sum_j coeff[4j + block] * X^j  in  Fp[X]/(X^4 - 11):  multiply the accumulated value by X, add the next
        Fp4 shifted{{mul(part.e[3], enc(11)), part.e[0], part.e[1], part.e[2]}};
        part = shifted + coeff_u[n_taps + 4 * j + block];
      }
      check = check + part * zr;
      zr = zr * z;
    }
    const Fp4 vanishing = fp4_pow(scale(z, enc(3)), n) - fp4_one();
    if (!(check * vanishing == lhs)) throw Reject{R0H_VERIFY_CHECK_MISMATCH};
  }

  // DEEP batching: the per-combo mixes of the interpolants
  const Fp4 deep_mix = io.ext();
  size_t widest = 1;
  for (uint32_t kq = 0; kq < n_combos; kq++) widest = std::max<size_t>(widest, c.combo_begin[kq + 1] - c.combo_begin[kq]);
  std::vector<Fp4> combo_u((size_t)(n_combos + 1) * widest, fp4_zero());
  std::vector<Fp4> reg_weight(n_regs), check_weight(R0H_CHECK_SIZE);
  {
    Fp4 cur = fp4_one();
    for (uint32_t r = 0; r < n_regs; r++) {
      reg_weight[r] = cur;
      for (uint32_t i = 0; i < c.regs[r].size; i++) {
        Fp4& dst = combo_u[(size_t)c.regs[r].combo * widest + i];
        dst = dst + cur * coeff_u[c.regs[r].first_tap + i];
      }
      cur = cur * deep_mix;
    }
    for (uint32_t i = 0; i < R0H_CHECK_SIZE; i++) {
      check_weight[i] = cur;
      combo_u[(size_t)n_combos * widest] = combo_u[(size_t)n_combos * widest] + cur * coeff_u[n_taps + i];
      cur = cur * deep_mix;
    }
  }
  std::vector<Fp4> combo_points;  // z * w^-back for every (combo, back)
  for (size_t b = 0; b < c.combo_backs.size(); b++) combo_points.push_back(scale(z, fpow(back_one, c.combo_backs[b])));

  // FRI commitments and the final polynomial
  struct Round { std::unique_ptr<TreeVerifier> tree; Fp4 mix; size_t rows; };
  std::vector<Round> rounds;
  const FriSchedule fri(n);
  for (const FriRound& fr : fri.rounds) {
    Round rd;
    rd.rows = fr.rows;
    rd.tree.reset(new TreeVerifier(io, rd.rows, R0H_FRI_FOLD * 4, R0H_VERIFY_FRI_MERKLE));
    rd.mix = io.ext();
    rounds.push_back(std::move(rd));
  }
  const size_t degree = fri.final_degree;
  std::vector<Fp4> final_poly(degree);
  {
    const uint32_t* fc = io.take_elems(4 * degree);
    io.commit_elems(fc, 4 * degree);
    for (size_t i = 0; i < degree; i++)
      for (int q = 0; q < 4; q++) final_poly[i].e[q] = fc[(size_t)q * degree + i];
  }

  // the size-16 inverse DFT matrix of a fold, shared by all queries
  uint32_t idft[R0H_FRI_FOLD][R0H_FRI_FOLD];
  {
    const uint32_t zeta_inv = rou_rev(4), inv16 = fpow(enc(R0H_FRI_FOLD), P - 2);
    for (uint32_t j = 0; j < R0H_FRI_FOLD; j++)
      for (uint32_t kq = 0; kq < R0H_FRI_FOLD; kq++) idft[j][kq] = mul(inv16, fpow(zeta_inv, (uint64_t)j * kq));
  }
  const uint32_t w_domain = rou_fwd(log2u(domain)), w_final = rou_fwd(log2u(degree * R0H_INV_RATE));
  // The query positions depend only on the transcript, and every query's openings have the same size: the 50 queries are
  // independent and run on a few host threads.  The verdict is that of the first failing query, as in a sequential walk.
  size_t pos_of[R0H_QUERIES];
  for (uint32_t q = 0; q < R0H_QUERIES; q++) pos_of[q] = io.bits(log2u(domain)) % domain;
  size_t words_per_query = 0;
  for (int g = 0; g < 4; g++) words_per_query += group[g]->opening_words();
  for (const Round& rd : rounds) words_per_query += rd.tree->opening_words();
  const Cursor base = io.cursor();
  auto open = [&](const TreeVerifier& t, Cursor& cur, size_t row) {
    if constexpr (COLLECT) return t.open_later(cur, k, row, collected->jobs);
    else return t.open(cur, k, row);
  };
  auto one_query = [&](uint32_t q) {
    Cursor cur{base.w, base.n, base.pos + (size_t)q * words_per_query < base.n ? base.pos + (size_t)q * words_per_query : base.n};
    std::vector<Fp4> combo_tot(n_combos + 1, fp4_zero());
    size_t pos = pos_of[q];
    const uint32_t* row[4];
    for (int g = 0; g < 4; g++) row[g] = open(*group[g], cur, pos);
    const Fp4 x = lift(fpow(w_domain, pos));
    for (uint32_t r = 0; r < n_regs; r++) {
      Fp4& t = combo_tot[c.regs[r].combo];
      t = t + scale(reg_weight[r], row[c.regs[r].group][c.regs[r].offset]);
    }
    for (uint32_t i = 0; i < R0H_CHECK_SIZE; i++) combo_tot[n_combos] = combo_tot[n_combos] + scale(check_weight[i], row[3][i]);
    Fp4 goal = fp4_zero();
    for (uint32_t kq = 0; kq < n_combos; kq++) {
      const uint32_t b0 = c.combo_begin[kq], b1 = c.combo_begin[kq + 1];
      Fp4 den = fp4_one();
      for (uint32_t b = b0; b < b1; b++) den = den * (x - combo_points[b]);
      goal = goal + (combo_tot[kq] - horner(&combo_u[(size_t)kq * widest], b1 - b0, x)) * fp4_inv(den);
    }
    goal = goal + (combo_tot[n_combos] - combo_u[(size_t)n_combos * widest]) * fp4_inv(x - z4);

    size_t rows_above = domain;
    for (const Round& rd : rounds) {
      const size_t quot = pos / rd.rows, grp = pos % rd.rows;
      const uint32_t* col = open(*rd.tree, cur, grp);
      Fp4 v[R0H_FRI_FOLD];
      for (uint32_t i = 0; i < R0H_FRI_FOLD; i++)
        for (int e = 0; e < 4; e++) v[i].e[e] = col[e * R0H_FRI_FOLD + i];
      if (!(v[quot] == goal)) throw Reject{R0H_VERIFY_FRI_GOAL};
      // interpolate the 16 values over the coset w^grp * <zeta>, then evaluate the interpolant's fold at the round mix
      const uint32_t untwist = fpow(rou_rev(log2u(rows_above)), grp);
      Fp4 tot = fp4_zero(), mixpow = fp4_one();
      uint32_t tw = ONE;
      for (uint32_t j = 0; j < R0H_FRI_FOLD; j++) {
        Fp4 cj = fp4_zero();
        for (uint32_t i = 0; i < R0H_FRI_FOLD; i++) cj = cj + scale(v[i], idft[j][i]);
        tot = tot + scale(cj, tw) * mixpow;
        mixpow = mixpow * rd.mix;
        tw = mul(tw, untwist);
      }
      goal = tot;
      pos = grp;
      rows_above = rd.rows;
    }
    if (!(horner(final_poly.data(), degree, lift(fpow(w_final, pos))) == goal)) throw Reject{R0H_VERIFY_FRI_FINAL};
  };
  if constexpr (COLLECT) {  // seal order: query by query, a query's openings in the order the walk reads them
    for (uint32_t q = 0; q < R0H_QUERIES; q++) {
      collected->first_job[q] = (uint32_t)collected->jobs.size();
      try { one_query(q); collected->walk[q] = R0H_VERIFY_OK; }
      catch (const Reject& r) { collected->walk[q] = r.code; }
    }
    collected->first_job[R0H_QUERIES] = (uint32_t)collected->jobs.size();
    io.skip_to(base.pos + (size_t)R0H_QUERIES * words_per_query);
    collected->trailing = !io.exhausted();
    return;
  }
  int verdict_of[R0H_QUERIES];
  std::atomic<uint32_t> next{0};
  auto worker = [&]() {
    for (uint32_t q; (q = next.fetch_add(1)) < R0H_QUERIES;) {
      try { one_query(q); verdict_of[q] = R0H_VERIFY_OK; }
      catch (const Reject& r) { verdict_of[q] = r.code; }
      catch (...) { verdict_of[q] = -1; }  // e.g. bad_alloc: reported below, never left to terminate the thread
    }
  };
  unsigned n_threads = std::thread::hardware_concurrency();
  n_threads = n_threads < 1 ? 1 : n_threads > 16 ? 16 : n_threads;
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < n_threads; t++) pool.emplace_back(worker);
  worker();
  for (std::thread& t : pool) t.join();
  for (uint32_t q = 0; q < R0H_QUERIES; q++) {
    if (verdict_of[q] == -1) throw std::runtime_error("r0h_verify_seal: a query worker failed (out of memory?)");
    if (verdict_of[q] != R0H_VERIFY_OK) throw Reject{verdict_of[q]};
  }
  io.skip_to(base.pos + (size_t)R0H_QUERIES * words_per_query);
  if (!io.exhausted()) throw Reject{R0H_VERIFY_TRAILING};
}

// the verdict of a collected seal once its openings are hashed (reached[j][8] for job j): the reject code of the first job in seal
// order that does not reach its node, a query's own verdict where all its jobs do -- every recorded job precedes the point where its
// query's walk stopped, and the immediate verifier reports the first failing query -- then the trailing-words check
int settle(const Collected& col, const uint32_t* reached) {
  for (uint32_t q = 0; q < R0H_QUERIES; q++) {
    for (uint32_t j = col.first_job[q]; j < col.first_job[q + 1]; j++)
      if (memcmp(col.jobs[j].want, reached + 8 * (size_t)j, 32) != 0) return col.jobs[j].reject;
    if (col.walk[q] != R0H_VERIFY_OK) return col.walk[q];
  }
  return col.trailing ? R0H_VERIFY_TRAILING : R0H_VERIFY_OK;
}

}  // namespace

const char* verify_seals_batch(r0h_ctx* ctx, int host_hashfn, SealCheck* seals, size_t n, size_t* upload_bytes_out) {
  const int hashfn = ctx ? ctx->hashfn : host_hashfn;
  const std::unique_ptr<HashSuite> suite = make_suite(hashfn, ctx ? &ctx->p2_host : &p2_default());
  if (upload_bytes_out) *upload_bytes_out = 0;
  std::vector<Collected> walks(n);
  std::vector<char> open_verdict(n, 0);  // the seal's verdict waits for its openings
  // the walks, one after the other on the calling thread (what is left of a seal is about 1.5 ms: profiles/r16/verify_on_device.md)
  auto walk = [&](size_t s) {
    SealCheck& sc = seals[s];
    sc.err = nullptr; sc.verdict = -1; sc.po2 = 0;
    memset(sc.code_root, 0, 32);
    memset(sc.data_root, 0, 32);
    if (!sc.blob || (!sc.seal && sc.seal_words)) { sc.err = make_error("r0h_verify_seal: NULL argument"); return; }
    for (int i = 0; i < 8 && sc.expected_code_root && hashfn == HASH_POSEIDON2; i++)
      if (sc.expected_code_root[i] >= P) { sc.err = make_error("r0h_verify_seal: expected code root word %d not canonical", i); return; }
    try {
      r0h_circuit c;
      if ((sc.err = parse_blob(&c, sc.blob, sc.blob_words))) return;
      verify<true>(c, *suite, sc.seal, sc.seal_words, &sc.po2, sc.expected_code_root, sc.code_root, sc.data_root, &walks[s]);
      open_verdict[s] = 1;
    } catch (const Reject& r) {
      sc.verdict = r.code;
    } catch (const std::exception& ex) {
      sc.err = make_error("exception: %s", ex.what());
    } catch (...) {
      sc.err = make_error("unknown exception");
    }
  };
  for (size_t s = 0; s < n; s++) walk(s);
  // an error of the batch as a whole takes the per-seal errors with it: the caller gets one string to free
  auto failed = [&](const char* err) {
    for (size_t s = 0; s < n; s++)
      if (seals[s].err) { r0h_free_error(seals[s].err); seals[s].err = nullptr; }
    return err;
  };
  size_t n_jobs = 0;
  for (size_t s = 0; s < n; s++)
    if (open_verdict[s]) n_jobs += walks[s].jobs.size();
  std::vector<uint32_t> reached(8 * n_jobs);
  if (ctx) {
    // a seal's openings lie back to back behind its final polynomial: one span per seal, from its first recorded opening to the end
    // of its last, goes up as it is
    std::vector<ClimbSpan> spans;
    std::vector<ClimbJob> jobs;
    jobs.reserve(n_jobs);
    size_t at = 0;
    for (size_t s = 0; s < n; s++) {
      const std::vector<Deferred>& dj = walks[s].jobs;
      if (!open_verdict[s] || dj.empty()) continue;
      const uint32_t* lo = dj.front().values;
      const uint32_t* hi = dj.back().values + dj.back().cols + 8 * (size_t)dj.back().path;
      for (const Deferred& d : dj) jobs.push_back(ClimbJob{(uint32_t)(at + (size_t)(d.values - lo)), d.cols, d.path, d.row});
      spans.push_back(ClimbSpan{lo, (size_t)(hi - lo)});
      at += (size_t)(hi - lo);
      if (at >= ((size_t)1 << 32)) return failed(make_error("r0h_verify_seals_on: %zu words of openings in one batch", at));
    }
    if (const char* err = merkle_climb_spans(ctx, spans.data(), spans.size(), jobs.data(), jobs.size(), reached.data(), upload_bytes_out)) return failed(err);
  } else {
    size_t j = 0;
    for (size_t s = 0; s < n; s++)
      for (const Deferred& d : walks[s].jobs) {
        if (!open_verdict[s]) break;
        uint32_t* cur = &reached[8 * j++];
        uint32_t parent[8];
        suite->hash_elems(d.values, d.cols, cur);
        for (uint32_t l = 0; l < d.path; l++) {
          const uint32_t* sibling = d.values + d.cols + 8 * (size_t)l;
          if ((d.row >> l) & 1) suite->hash_pair(sibling, cur, parent); else suite->hash_pair(cur, sibling, parent);
          memcpy(cur, parent, 32);
        }
      }
  }
  size_t j = 0;
  for (size_t s = 0; s < n; s++) {
    if (!open_verdict[s]) continue;
    seals[s].verdict = settle(walks[s], reached.data() + 8 * j);
    j += walks[s].jobs.size();
  }
  return nullptr;
}
}  // namespace r0h

namespace r0h {
const char* sponge_trace_args(const char* caller, const uint32_t* words, size_t n_words, uint32_t po2, size_t* n_perm_out) {
  R0H_REQUIRE(po2 >= 6 && po2 <= R0H_MAX_PO2, "%s: po2 %u outside [6, %u]", caller, po2, R0H_MAX_PO2);
  const size_t n = (size_t)1 << po2, n_perm = n_words ? (n_words + P2_RATE - 1) / P2_RATE : 1;
  R0H_REQUIRE(n_perm * R0H_SPONGE_PERIOD < n, "%s: %zu words take %zu rows, the trace has 2^%u", caller, n_words, n_perm * R0H_SPONGE_PERIOD, po2);
  for (size_t i = 0; i < n_words; i++) R0H_REQUIRE(words[i] < P, "%s: word %zu is not a canonical field element", caller, i);
  *n_perm_out = n_perm;
  return nullptr;
}
}  // namespace r0h

using namespace r0h;

extern "C" {

const char* r0h_verify_reason(int verdict) {
  static const char* const names[] = {"ok", "seal truncated", "bad po2", "group merkle path rejected", "constraint check mismatch at z",
                                      "fri merkle path rejected", "fri fold goal mismatch", "fri final polynomial mismatch",
                                      "trailing words in seal", "non-canonical field element", "code root is not the expected control root"};
  return verdict >= 0 && verdict <= R0H_VERIFY_CODE_ROOT ? names[verdict] : "unknown";
}

const char* r0h_seal_digest(const uint32_t* seal, size_t seal_words, uint32_t digest_out[8]) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE((seal || seal_words == 0) && digest_out, "r0h_seal_digest: NULL argument");
  // every word of a well-formed seal is a canonical field element (globals, digests, interpolants, opened columns): reducing
  // mod p here would give two different word sequences the same name
  for (size_t i = 0; i < seal_words; i++) R0H_REQUIRE(seal[i] < P, "r0h_seal_digest: word %zu is not a canonical field element", i);
  p2_hash_elems_host(p2_default(), seal, seal_words, digest_out);
  return nullptr;
  R0H_GUARD_END
}

// The rows of the recursion circuit's in-circuit sponge over `words` (include/r0hip_circuit.h SPONGE): R0H_SPONGE_DATA_COLUMNS columns
// of 2^po2 rows, zero behind the last permutation.  Pure host code; what r0h_lift / r0h_join plant into a node's witness.
const char* r0h_sponge_trace(const uint32_t* words, size_t n_words, uint32_t po2, uint32_t* cols_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE((words || n_words == 0) && cols_out, "r0h_sponge_trace: NULL argument");
  size_t n_perm = 0;
  R0H_TRY(sponge_trace_args("r0h_sponge_trace", words, n_words, po2, &n_perm));
  const size_t n = (size_t)1 << po2;
  memset(cols_out, 0, (size_t)R0H_SPONGE_DATA_COLUMNS * n * 4);
  size_t used = 0;
  p2_sponge_rows_host(p2_default(), words, n_words, cols_out, n, &used);
  return nullptr;
  R0H_GUARD_END
}

static const char* verify_entry(int hashfn, const uint32_t* blob, size_t blob_words, const uint32_t* p2_round_constants, const uint32_t* p2_diag_m1,
                                const uint32_t* seal, size_t seal_words, const uint32_t* expected_code_root, int* verdict_out, uint32_t* po2_out,
                                uint32_t* code_root_out, uint32_t* data_root_out = nullptr) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(blob && (seal || seal_words == 0) && verdict_out, "r0h_verify_seal: NULL argument");
  R0H_REQUIRE((p2_round_constants == nullptr) == (p2_diag_m1 == nullptr), "r0h_verify_seal: pass both Poseidon2 tables or neither");
  if (expected_code_root && hashfn == HASH_POSEIDON2)
    for (int i = 0; i < 8; i++) R0H_REQUIRE(expected_code_root[i] < P, "r0h_verify_seal: expected code root word %d not canonical", i);
  r0h_circuit c;
  R0H_TRY(parse_blob(&c, blob, blob_words));
  std::unique_ptr<P2Consts> own;  // a caller's table
  if (p2_round_constants) {
    for (size_t i = 0; i < (size_t)P2_ROUNDS * P2_CELLS; i++) R0H_REQUIRE(p2_round_constants[i] < P, "r0h_verify_seal: round constant %zu not canonical", i);
    for (size_t i = 0; i < P2_CELLS; i++) R0H_REQUIRE(p2_diag_m1[i] < P, "r0h_verify_seal: diagonal entry %zu not canonical", i);
    own.reset(new P2Consts);
    fill_p2(*own, p2_round_constants, p2_diag_m1);
  }
  if (po2_out) *po2_out = 0;
  if (code_root_out) memset(code_root_out, 0, 32);
  try {
    verify<false>(c, *make_suite(hashfn, own ? own.get() : &p2_default()), seal, seal_words, po2_out, expected_code_root, code_root_out, data_root_out);
    *verdict_out = R0H_VERIFY_OK;
  } catch (const Reject& r) {
    *verdict_out = r.code;
  }
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_verify_seal(const uint32_t* blob, size_t blob_words, const uint32_t* p2_round_constants, const uint32_t* p2_diag_m1,
                            const uint32_t* seal, size_t seal_words, int* verdict_out, uint32_t* po2_out) {
  return verify_entry(HASH_POSEIDON2, blob, blob_words, p2_round_constants, p2_diag_m1, seal, seal_words, nullptr, verdict_out, po2_out, nullptr);
}

const char* r0h_verify_seal_bound(const uint32_t* blob, size_t blob_words, const uint32_t* p2_round_constants, const uint32_t* p2_diag_m1,
                                  const uint32_t* seal, size_t seal_words, const uint32_t* expected_code_root, int* verdict_out,
                                  uint32_t* po2_out, uint32_t* code_root_out) {
  return verify_entry(HASH_POSEIDON2, blob, blob_words, p2_round_constants, p2_diag_m1, seal, seal_words, expected_code_root, verdict_out, po2_out, code_root_out);
}

// the same check of a seal made under the named hash suite ("poseidon2": the compiled-in table; "sha-256")
const char* r0h_verify_seal_hashfn(const uint32_t* blob, size_t blob_words, const char* hashfn, const uint32_t* seal, size_t seal_words,
                                   const uint32_t* expected_code_root, int* verdict_out, uint32_t* po2_out, uint32_t* code_root_out) {
  int fn = 0;
  R0H_TRY(hashfn_parse("r0h_verify_seal_hashfn", hashfn, &fn));
  return verify_entry(fn, blob, blob_words, nullptr, nullptr, seal, seal_words, expected_code_root, verdict_out, po2_out, code_root_out);
}

// the same, also returning the DATA group's Merkle root as the seal's transcript recomputes it: what a session's common challenge is
// derived from (csrc/claim.cpp)
const char* r0h_verify_seal_roots(const uint32_t* blob, size_t blob_words, const uint32_t* seal, size_t seal_words, const uint32_t* expected_code_root, int* verdict_out,
                                  uint32_t* po2_out, uint32_t* data_root_out) {
  R0H_REQUIRE(data_root_out, "r0h_verify_seal_roots: NULL argument");
  memset(data_root_out, 0, 32);
  return verify_entry(HASH_POSEIDON2, blob, blob_words, nullptr, nullptr, seal, seal_words, expected_code_root, verdict_out, po2_out, nullptr, data_root_out);
}

// n seals of one circuit (back to back in `seals`), their Merkle openings hashed in one batch: on `ctx` (one upload, one launch; suite and Poseidon2 table the
// context's) or, ctx == NULL, on the host (Poseidon2, the compiled-in table).  Verdicts are r0h_verify_seal_roots's.
const char* r0h_verify_seals_on(r0h_ctx* ctx, const uint32_t* blob, size_t blob_words, const uint32_t* seals, const size_t* seal_words, size_t n,
                                const uint32_t* expected_code_roots, int* verdicts_out, uint32_t* po2_out, uint32_t* data_roots_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(blob && ((seals && seal_words && verdicts_out) || !n), "r0h_verify_seals_on: NULL argument");
  std::vector<SealCheck> checks(n);
  size_t at = 0;
  for (size_t s = 0; s < n; s++) {
    checks[s] = SealCheck{blob, blob_words, seals + at, seal_words[s], expected_code_roots ? expected_code_roots + 8 * s : nullptr};
    at += seal_words[s];
    verdicts_out[s] = -1;
  }
  const char* err = verify_seals_batch(ctx, HASH_POSEIDON2, checks.data(), n);
  for (SealCheck& sc : checks) {  // one circuit, one suite: a per-seal error is the call's
    if (sc.err && !err) err = sc.err;
    else if (sc.err) r0h_free_error(sc.err);
  }
  if (err) return err;
  for (size_t s = 0; s < n; s++) {
    verdicts_out[s] = checks[s].verdict;
    if (po2_out) po2_out[s] = checks[s].po2;
    if (data_roots_out) memcpy(data_roots_out + 8 * s, checks[s].data_root, 32);
  }
  return nullptr;
  R0H_GUARD_END
}

// ---- the control root of a circuit's own CODE columns, on the host.  A verifier is handed control roots (risc0's has a table of
// them compiled in); this lets it derive them from the circuit blob alone instead of trusting the prover's word: the CODE columns of
// the blob's column program (first-row / last-row indicator, row index, seeded column -- what r0h_witgen generates on the device),
// interpolated, shifted by 3, evaluated on the 4N coset, rows hashed, folded.  Plain radix-2 transforms and one Poseidon2 permutation
// per row and node: seconds at 2^20 rows, spread over the host's threads.
}  // extern "C"
namespace {
// in place, natural order in and out; w = a primitive 2^log_n-th root of unity (Montgomery words throughout)
void ntt_host(uint32_t* a, uint32_t log_n, uint32_t w) {
  const size_t n = (size_t)1 << log_n;
  for (size_t i = 0; i < n; i++) {
    const size_t j = bitrev((uint32_t)i, log_n);
    if (i < j) std::swap(a[i], a[j]);
  }
  std::vector<uint32_t> tw(n / 2);
  uint32_t x = ONE;
  for (size_t i = 0; i < n / 2; i++) { tw[i] = x; x = mul(x, w); }
  for (uint32_t s = 1; s <= log_n; s++) {
    const size_t half = (size_t)1 << (s - 1), step = n >> s;
    for (size_t base = 0; base < n; base += 2 * half)
      for (size_t k = 0; k < half; k++) {
        const uint32_t u = a[base + k], v = mul(a[base + k + half], tw[k * step]);
        a[base + k] = add(u, v);
        a[base + k + half] = sub(u, v);
      }
  }
}
template <class F>
void in_parallel(size_t n, F f) {
  const size_t workers = std::max<size_t>(1, std::min<size_t>(std::thread::hardware_concurrency(), 16));
  std::vector<std::thread> ts;
  for (size_t t = 0; t < workers; t++) ts.emplace_back([=] { for (size_t i = n * t / workers; i < n * (t + 1) / workers; i++) f(i); });
  for (auto& t : ts) t.join();
}
}  // namespace
extern "C" {

static const char* control_root_host(int hashfn, const uint32_t* blob, size_t blob_words, const uint32_t* p2_round_constants, const uint32_t* p2_diag_m1,
                                     uint32_t po2, uint32_t root_out[8]) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(blob && root_out, "r0h_control_root_host: NULL argument");
  R0H_REQUIRE((p2_round_constants == nullptr) == (p2_diag_m1 == nullptr), "r0h_control_root_host: pass both Poseidon2 tables or neither");
  R0H_REQUIRE(po2 >= 4 && po2 <= R0H_MAX_PO2, "r0h_control_root_host: po2 %u outside [4, %u]", po2, (unsigned)R0H_MAX_PO2);
  r0h_circuit c;
  R0H_TRY(parse_blob(&c, blob, blob_words));
  R0H_REQUIRE(c.has_column_program, "r0h_control_root_host: the circuit has no column program: its CODE columns come from elsewhere");
  std::unique_ptr<P2Consts> own;  // a caller's table
  if (p2_round_constants) { own.reset(new P2Consts); fill_p2(*own, p2_round_constants, p2_diag_m1); }
  const std::unique_ptr<HashSuite> suite = make_suite(hashfn, own ? own.get() : &p2_default());
  const uint32_t count = c.group_size[R0H_GROUP_CODE];
  const size_t n = (size_t)1 << po2, m = 4 * n;
  R0H_REQUIRE(c.code_cols.size() == count && count >= 1, "r0h_control_root_host: %zu CODE columns described, %u in the group", c.code_cols.size(), count);
  const uint64_t seed = splitmix64(CODE_SEED);
  std::vector<uint32_t> periodic(c.periodic);  // Montgomery form, as fixed_cell reads it
  for (uint32_t& v : periodic) v = enc(v);
  const uint32_t w_n_inv = rou_rev(po2), w_m = rou_fwd(po2 + 2), n_inv = inv(enc((uint32_t)n)), three = enc(3);
  std::vector<uint32_t> evals((size_t)count * m);
  for (uint32_t col = 0; col < count; col++) {
    uint32_t* a = &evals[(size_t)col * m];
    const uint32_t kind = c.code_cols[col].kind, arg = code_col_arg(c.code_cols[col], col);
    R0H_REQUIRE(kind <= 6, "r0h_control_root_host: CODE column %u has kind %u", col, kind);
    for (uint32_t r = 0; r < n; r++) a[r] = fixed_cell(kind, arg, r, (uint32_t)n, seed, periodic.data(), c.period);
    ntt_host(a, po2, w_n_inv);  // values on the 2^po2 subgroup -> coefficients (times n)
    uint32_t shift = n_inv;     // ... scaled back and moved to the coset 3 <w>: coefficient i times 3^i
    for (size_t i = 0; i < n; i++) { a[i] = mul(a[i], shift); shift = mul(shift, three); }
    std::fill(a + n, a + m, 0u);
    ntt_host(a, po2 + 2, w_m);  // evaluations on the 4N coset, natural order
  }
  std::vector<uint32_t> nodes(2 * m * 8);
  in_parallel(m, [&](size_t r) {
    uint32_t row[64];
    std::vector<uint32_t> wide;
    uint32_t* v = row;
    if (count > 64) { wide.resize(count); v = wide.data(); }
    for (uint32_t col = 0; col < count; col++) v[col] = evals[(size_t)col * m + r];
    suite->hash_elems(v, count, &nodes[(m + r) * 8]);
  });
  for (size_t level = m / 2; level >= 1; level /= 2)
    in_parallel(level, [&](size_t i) { suite->hash_pair(&nodes[2 * (level + i) * 8], &nodes[(2 * (level + i) + 1) * 8], &nodes[(level + i) * 8]); });
  memcpy(root_out, &nodes[8], 32);
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_control_root_host(const uint32_t* blob, size_t blob_words, const uint32_t* p2_round_constants, const uint32_t* p2_diag_m1,
                                  uint32_t po2, uint32_t root_out[8]) {
  return control_root_host(HASH_POSEIDON2, blob, blob_words, p2_round_constants, p2_diag_m1, po2, root_out);
}
const char* r0h_control_root_host_hashfn(const uint32_t* blob, size_t blob_words, const char* hashfn, uint32_t po2, uint32_t root_out[8]) {
  int fn = 0;
  R0H_TRY(hashfn_parse("r0h_control_root_host_hashfn", hashfn, &fn));
  return control_root_host(fn, blob, blob_words, nullptr, nullptr, po2, root_out);
}

}  // extern "C"
