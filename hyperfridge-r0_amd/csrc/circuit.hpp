// Parsed circuit blob (include/r0hip_circuit.h): filled by blob.cpp (parse_blob), planned and turned into source text by
// evalcheck_emit.cpp, compiled, loaded and launched by circuit.hip, walked by prover.hip (sequencer) and verify.cpp.
#pragma once
#include <algorithm>
#include <functional>
#include <mutex>
#include <unordered_map>

#include "../../include/r0hip_circuit.h"
#include "internal.hpp"

namespace r0h {

struct Tap { uint32_t group, offset, back; };
struct Reg { uint32_t group, offset, first_tap, size, combo; };
struct Step { uint32_t op, a, b, c; };
struct CodeCol { uint32_t kind, param; };
struct DataCol { uint32_t kind, a, b, c, e; };
struct AccCol { uint32_t first, a, b; };
struct Term { uint32_t pow, v; std::vector<uint32_t> conds; };
// the log-derivative argument (R0H_SEC_LOGUP): fractions numerator / (sum of challenge x linear form), four to an accumulator
struct LfTerm { uint32_t coef, global, col; };  // canonical coefficient; public input + 1 or 0; column ref + 1 or 0 (the constant one)
struct Lf { std::vector<LfTerm> terms; };
struct LogupPart { uint32_t ch_kind, ch_idx; Lf lf; };
struct LogupFraction { uint32_t table; Lf num; std::vector<LogupPart> parts; };
struct LogupAcc { uint32_t final_global; std::vector<LogupFraction> fr; };
struct LogupTable { uint32_t data_col, kind; };
struct Logup {
  std::vector<LogupTable> tables;
  std::vector<LogupAcc> accs;
  uint32_t n_chain = 0;  // the first n_chain accumulators are links of the chain
};

// ---- the fixed columns of the synthetic column program (blob section WITGEN), one statement for the device (circuit.hip
// witgen_fixed_kernel) and for the host (verify.cpp control_root_host)
R0H_HD uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
R0H_HD uint32_t synth_word(uint64_t seed_mixed, uint32_t stream, uint32_t row) {
  uint64_t h = splitmix64(seed_mixed ^ (((uint64_t)stream << 32) | row));
  return (uint32_t)(((h >> 32) * (uint64_t)P) >> 32);
}
constexpr uint64_t CODE_SEED = 0xC0DEull;  // the CODE group's seed (a program's CODE columns do not depend on the witness seed); splitmix64 of it is seed_mixed
// what fixed_cell takes beside the kind of CODE column `col`: a periodic column names its schedule, every other its stream of the generator
inline uint32_t code_col_arg(const CodeCol& cc, uint32_t col) { return cc.kind == 6 ? cc.param : (1u << 16) | col; }
// The word (Montgomery form) a fixed column of kind 0..6 holds at row r of n (include/r0hip_circuit.h WITGEN); `periodic` is the PERIODIC
// section in Montgomery form, [column][period].  Any other kind is not a fixed column: 0.
R0H_HD uint32_t fixed_cell(uint32_t kind, uint32_t arg, uint32_t r, uint32_t n, uint64_t seed_mixed, const uint32_t* periodic, uint32_t period) {
  if (kind == 0) return r == 0 ? ONE : 0u;
  if (kind == 1) return r == n - 1 ? ONE : 0u;
  if (kind == 2) return enc(r);
  if (kind == 3) return synth_word(seed_mixed, arg, r);
  if (kind == 4) return r < 65536u ? enc(r) : 0u;                                                     // the 16-bit range table
  if (kind == 5) return enc(R0H_TAG_AND + (r < 65536u ? r + 65536u * ((r & 255u) & (r >> 8)) : 0u));  // the byte-AND table
  if (kind == 6) return r < (n / period) * period ? periodic[arg * period + r % period] : 0u;         // a periodic schedule
  return 0u;
}

// ---- the balance check (r0h_logup_check_balance, include/r0hip.h), one statement for the device (balance.hip) and the host
// (logup_host.cpp's walk_tuples, for balance_host.cpp): a tuple's class is known by two linear hashes over F_p of its per-identity part sums, h_j = sum_i w_j(i) s_i.
// The weights are fixed words in [1, p) of the challenge's identity (kind << 32 | index; 0 is "one"); the key is never 0 (an empty slot).
R0H_HD uint32_t balance_weight(uint32_t j, uint64_t identity) {
  const uint64_t h = splitmix64(splitmix64(identity) + 0xBA1A9CEull * (j + 1));
  return 1u + (uint32_t)(((h >> 32) * (uint64_t)(P - 1)) >> 32);
}
R0H_HD uint64_t balance_key(uint32_t h0, uint32_t h1) { return (((uint64_t)h0 << 31) | h1) + 1; }
inline std::vector<uint32_t> balance_weights(const std::vector<uint64_t>& ids) {  // [2][ids.size()]: row j is balance_weight(j, .) of each
  std::vector<uint32_t> w(2 * ids.size());
  for (size_t k = 0; k < w.size(); k++) w[k] = balance_weight((uint32_t)(k / ids.size()), ids[k % ids.size()]);
  return w;
}

struct Plan {                      // how the constraint program is cut into kernels
  std::vector<Term> terms;         // flattened, in chain order
  std::vector<uint32_t> cut;       // kernel k owns terms [cut[k], cut[k+1])
  uint32_t n_pow = 0;
  std::vector<bool> late;          // term t reaches an ACCUM tap or a word of the accumulation mix: it has no value before the mix is drawn
};

}  // namespace r0h

struct r0h_circuit {
  r0h_ctx* ctx = nullptr;
  uint32_t group_size[3] = {0, 0, 0};
  std::vector<r0h::Tap> taps;
  std::vector<r0h::Reg> regs;
  std::vector<uint32_t> combo_begin, combo_backs;
  uint32_t group_tap_begin[4] = {0, 0, 0, 0};
  uint32_t n_global = 0, n_mix = 0;
  std::vector<uint32_t> global_cols;
  std::vector<r0h::Step> steps;
  uint32_t ret = 0;
  std::vector<uint32_t> fp_step, mix_step;  // variable index -> step index
  std::vector<r0h::CodeCol> code_cols;
  std::vector<r0h::DataCol> data_cols;
  std::vector<r0h::AccCol> acc_cols;
  r0h::Logup logup;
  uint32_t period = 0;               // R0H_SEC_PERIODIC: what CODE columns of kind 6 repeat, [n_periodic][period] canonical values
  std::vector<uint32_t> periodic;
  bool has_sponge = false;           // R0H_SEC_SPONGE: the in-circuit Poseidon2 sponge, its first CODE / DATA column, the first public input of its digest
  uint32_t sponge_code = 0, sponge_data = 0, sponge_global = 0;
  uint32_t n_late = 0;  // the last n_late public inputs enter the transcript after the DATA commitment (R0H_SEC_LATE)
  bool has_column_program = false;  // WITGEN + ACCUM present (synthetic circuits); imported circuits bring their own witness
  std::vector<uint32_t> blob;
  uint8_t info[16] = {'R', '0', 'H', 'I', 'P', '_', 'S', 'Y', 'N', 'T', 'H', ':', 'v', '1', '_', '_'};  // circuit ProtocolInfo tag
  r0h::Plan plan;
  hipModule_t module = nullptr;
  std::vector<hipFunction_t> kernels;
  // the witness checker (r0h_check_witness): its own module, compiled on first use -- or loaded from a code object by
  // r0h_circuit_load_check -- under check_mu: one loaded circuit serves every context of its device, from any thread
  mutable std::mutex check_mu;
  mutable hipModule_t check_module = nullptr;
  mutable std::vector<hipFunction_t> check_kernels;
};

namespace r0h {
// fills the host tables of `c` from a blob (no device work); validates every index the sequencer and the verifier follow
const char* parse_blob(r0h_circuit* c, const uint32_t* blob, size_t n_words);
// evalcheck_emit.cpp: c->plan from the parsed tables (flattened terms, their cut into kernels), then the eval_check and the
// witness-checker source text of that plan (kernels eval_check_<k> / check_witness_<k>, one per cut)
void make_plan(r0h_circuit* c);
std::string emit_source(const r0h_circuit* c);
std::string emit_check_source(const r0h_circuit* c);
// the rows of the in-circuit sponge over `words` written into the circuit's sponge columns of `data`, zero behind the last permutation
// (sponge.hip: the host runs the chain, sponge_rows_kernel expands the rows; stream-ordered)
const char* sponge_plant(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const uint32_t* words, size_t n_words, r0h_buf* data);
// the same for a caller that has run the chain already (p2_sponge_chain_host: r0h_lift / r0h_join need its digest anyway): the
// 24 words each of the n_perm permutations starts from; the host words may be released on return
const char* sponge_plant_states(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const uint32_t* states, size_t n_perm, r0h_buf* data);
// what r0h_sponge_trace and r0h_sponge_trace_device refuse, in the same words (verify.cpp); *n_perm_out: the permutations the words take
const char* sponge_trace_args(const char* caller, const uint32_t* words, size_t n_words, uint32_t po2, size_t* n_perm_out);
// r0h_check_witness with the first violated term turned into an error that starts with `caller` (the sequencer under
// r0h_ctx_set_check_witness); global / mix are host words as r0h_eval_check takes them
const char* require_witness(const char* caller, r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* accum, const r0h_buf* code, const r0h_buf* data,
                            const uint32_t* global, const uint32_t* mix);
// r0h_logup_check_balance with the lowest imbalanced class turned into an error that starts with `caller` (balance.hip; the sequencer
// under r0h_ctx_set_check_balance)
const char* require_balance(const char* caller, r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, const uint32_t* global);
// The log-derivative accumulation on the device (logup.hip): multiplicities into DATA, the ACCUM group (logup_accum_kept), totals of the
// public accumulators.  The public accumulators' scanned terms of one segment, kept from the totals step for the accumulation that follows it on the same
// context under the same public inputs (session.cpp): the accumulation then unpacks them into ACCUM instead of evaluating and scanning
// them again.  logup_totals_keep is r0h_logup_totals with `keep` filled; logup_accum_kept uses `kept` (nullptr, or one that holds
// nothing: they are evaluated and scanned here).
struct LogupKept {
  DevBuf terms;  // [n_own][2^po2] packed extension elements, inclusive prefix sums
  uint32_t po2 = 0, n_own = 0;
};
// r0h_logup_multiplicities without its wait (logup.hip), and what its error word means
const char* logup_multiplicities_enqueue(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, r0h_buf* data, const uint32_t* global, r0h_buf* err_out, size_t err_word_offset);
const char* logup_multiplicities_verdict(uint32_t err);
const char* logup_totals_keep(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, uint32_t* global_io, LogupKept* keep);
const char* logup_accum_kept(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, const uint32_t* global, const uint32_t* mix, r0h_buf* accum,
                             const LogupKept* kept);
// the two with the public inputs (and the mix) in device buffers: challenges and coefficients are resolved by a kernel, the totals are
// left in `globals`, nothing is read back and nothing waits for the stream (r0h_logup_totals_device, r0h_accum_public_device)
const char* logup_totals_keep_device(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, r0h_buf* globals, LogupKept* keep);
const char* logup_accum_kept_device(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, const r0h_buf* globals, const r0h_buf* mix, r0h_buf* accum,
                                    const LogupKept* kept);
// The lookups of every table as a flat list (logup_host.cpp; what the device's counting kernel walks): per entry the numerator form
// and the value form, form = n, (coefficient, DATA column + 1 or 0)..., coefficients in Montgomery form with the public inputs folded
// in (absent public inputs count as 0).  Table k owns words [begin[k], begin[k + 1]) and `entries[k]` entries.
struct LookupList {
  std::vector<uint32_t> words;
  uint32_t begin[3] = {0, 0, 0}, entries[2] = {0, 0};
  uint32_t n_cols = 0;  // distinct DATA columns read
};
const char* logup_lookup_list(const r0h_circuit* c, const uint32_t* global, LookupList* out);
// ---- the host's plain-loop statements of the argument (logup_host.cpp), shared by every host check.  A linear form at row r of n over
// host words (Montgomery form, column-major; absent public inputs count as 0), and what it needs of `caller`'s arguments:
// "<caller>: a form reads the CODE group and none was given" / "... a public input and none were given"
uint32_t eval_lf(const Lf& lf, const uint32_t* code, const uint32_t* data, const uint32_t* global, size_t n, size_t r);
const char* require_lf_inputs(const char* caller, const Lf& lf, const uint32_t* code, const uint32_t* global);
// The tuples of accumulators [first, first + count): `each` is called for every fraction (numbered 4 * accumulator + slot, in order)
// and every row on which its numerator is not zero, and what it returns other than nullptr ends the walk as its error.  `sums` are the
// canonical per-identity sums of the fraction's parts, one per entry of tuple_identities (the challenge identities kind << 32 | index,
// 0 for "one", in order of first appearance: as many as the accumulators have); `key` is the balance_key of their two hashes.
inline uint64_t part_identity(const LogupPart& q) { return q.ch_kind ? (uint64_t)q.ch_kind << 32 | q.ch_idx : 0; }
std::vector<uint64_t> tuple_identities(const r0h_circuit& c, uint32_t first, uint32_t count);
struct HostTuple { uint64_t key; uint32_t numerator /* canonical */, row, fraction; const uint32_t* sums; };
const char* walk_tuples(const char* caller, const r0h_circuit& c, uint32_t first, uint32_t count, uint32_t po2, const uint32_t* code, const uint32_t* data, const uint32_t* global,
                        const std::function<const char*(const HostTuple&)>& each);

// ---- the session balance (r0h_session_balance_*, include/r0hip.h): the balance check's definitions over the accumulators with a
// public total, across the segments of a session and what the verifier adds.  The handle, its host half and the entry points that need
// no device are in balance_host.cpp; the device's table and kernels in balance.hip behind the session_table_* functions.
struct SessionClass {  // a class of a host handle
  uint64_t sum = 0, first = ~0ull /* source << 32 | row << 8 | fraction of the lowest member */, members = 0;
  uint32_t values[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // canonical per-identity sums, as the first member has them
};
struct SessionTable;  // the device's table (balance.hip)
constexpr uint32_t SESSION_MAX_IDS = 8, SESSION_OUTSIDE_FRACTION = 255;
constexpr size_t SESSION_MAX_LIST = (size_t)1 << 24;
R0H_HD uint64_t session_first(uint32_t source, uint32_t row, uint32_t fraction) { return (uint64_t)source << 32 | (uint64_t)row << 8 | fraction; }
// a report's entry of the class whose lowest member is `first` (session_first), from a host handle's classes or the device's slots
inline r0h_session_imbalance session_entry(uint64_t first, uint64_t sum, uint64_t members, size_t n_values, const uint32_t (&values)[8]) {
  r0h_session_imbalance e = {(uint32_t)(first >> 32), (uint32_t)(first & 255u), (uint32_t)(first >> 8) & 0xffffffu, (uint32_t)(sum % P), (uint32_t)std::min<uint64_t>(members, 0xffffffffull),
                             (uint32_t)n_values, {0, 0, 0, 0, 0, 0, 0, 0}};
  memcpy(e.values, values, sizeof e.values);
  return e;
}
}  // namespace r0h

struct r0h_session_balance {
  r0h_ctx* ctx = nullptr;             // nullptr: a host handle
  r0h_circuit circuit;                // parsed from the blob it was made with (no device side)
  std::vector<uint64_t> ids;          // the challenge identities (kind << 32 | index; 0 is "one") in order of first appearance
  std::vector<uint32_t> weights;      // [2][ids.size()]: balance_weight of each
  bool reads_global = false;          // some numerator or part reads an (early) public input
  uint64_t tuples = 0, grows = 0;
  uint64_t room = 0;                  // device handle: no more classes than this are held (tuples added, entries merged): what the table is sized from
  std::unordered_map<uint64_t, r0h::SessionClass> classes;  // host handle: by balance_key
  r0h::SessionTable* table = nullptr;                       // device handle
};

namespace r0h {
// balance.hip.  `keys` are the tuples' balance_key, `numerators` / `values` ([n][n_ids]) canonical; `report` returns the `capacity`
// lowest imbalanced classes in order and counts all of them
const char* session_table_add_list(r0h_session_balance* sb, uint32_t source, const uint64_t* keys, const uint32_t* numerators, const uint32_t* values, size_t n);
const char* session_table_report(r0h_session_balance* sb, r0h_session_imbalance* out, size_t capacity, size_t* n_out);
const char* session_table_stats(r0h_session_balance* sb, uint64_t* slots_out, uint64_t* occupied_out);
// every class held, in no order (the caller orders them), and a list of classes into the table (checked by the caller; `distinct` of its keys differ)
const char* session_table_export(r0h_session_balance* sb, std::vector<r0h_session_class>* out);
const char* session_table_merge(r0h_session_balance* sb, const r0h_session_class* classes, size_t n, uint64_t distinct);
void session_table_free(r0h_session_balance* sb);
}  // namespace r0h
