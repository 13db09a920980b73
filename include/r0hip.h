/* r0hip -- C ABI of the MI355X-native RISC Zero segment prover (hot path only: prove_segment).
 *
 * This is the drop-in boundary for the path the reference reaches through
 *     host/src/main.rs:420   let prover = default_prover();
 *     host/src/main.rs:423   prover.prove(env, HYPERFRIDGE_ELF)
 * i.e. (inside the un-vendored risc0 crates pinned in Cargo.lock:3195-3197, 3121-3123, 3174-3176) the
 * `risc0_zkp::hal::Hal` + `CircuitHal` operations that a native backend implements and that risc0's own
 * CUDA/Metal backends bind as `extern "C"` launchers from risc0-sys / risc0-circuit-rv32im-sys.
 * A Rust `HipHal` would bind exactly these entry points (INTEGRATION.md shows the stub).
 *
 * Conventions (mirroring risc0-sys's launcher convention):
 *   - every function returns `const char*`: NULL on success, otherwise a heap-allocated message the caller
 *     releases with r0h_free_error().  Nothing aborts or throws across the ABI.
 *   - field elements are uint32_t BabyBear words in Montgomery form (R = 2^32), always < p = 2013265921;
 *     extension elements are 4 consecutive words (x^4 = 11); digests are 8 words.
 *   - matrices are column-major: column c of a [count][size] buffer starts at word c*size.
 *   - a context is bound to one device and one stream and is not re-entrant; different contexts are independent.
 *     Operations are stream-ordered; only r0h_buf_d2h, r0h_sync and the functions that return host data block.
 *   - the caller owns host memory; the library owns device memory behind r0h_buf handles.
 */
#ifndef R0HIP_H
#define R0HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define R0H_P 2013265921u
#define R0H_INV_RATE 4
#define R0H_QUERIES 50
#define R0H_FRI_FOLD 16
#define R0H_FRI_MIN_DEGREE 256
#define R0H_CHECK_SIZE 16
#define R0H_DIGEST_WORDS 8
#define R0H_GROUP_ACCUM 0
#define R0H_GROUP_CODE 1
#define R0H_GROUP_DATA 2
#define R0H_MAX_PO2 24 /* trace rows of a segment: risc0's default segment size is 2^20, its largest 2^24.  The evaluation domain is
                        * 4x that and the NTT entry points take up to 2^26 points: two passes up to 2^23, three above
                        * (a 256-column segment of 2^22 rows keeps about 32 GiB resident, one of 2^24 rows about 128 GiB) */

typedef struct r0h_ctx r0h_ctx;
typedef struct r0h_buf r0h_buf;
typedef struct r0h_circuit r0h_circuit;

void r0h_free_error(const char* msg);
const char* r0h_version(void);

/* ---- context and buffers: Hal::alloc_*, copy_from_*, Buffer::{slice, view} ---- */
const char* r0h_ctx_create(int device, r0h_ctx** out);
const char* r0h_ctx_destroy(r0h_ctx* ctx);
const char* r0h_sync(r0h_ctx* ctx);
/* The context's hash suite (risc0 `ProverOpts::hashfn`): "poseidon2" (the default) or "sha-256"; any other name is an error.
 * r0h_hash_rows, r0h_hash_fold[_io], r0h_merkle_build, r0h_merkle_open_top, r0h_code_root, r0h_code_commit_new and every r0h_prove_segment* / r0h_proof_*
 * entry follow it; under "poseidon2" they compute what they always did.  A r0h_code_commit remembers the suite it was made under
 * (using it from a context on the other suite is an error that names both), and so does a proof between begin and finish.
 * Receipts, sessions, image proofs and recursion nodes name Poseidon2 only: r0h_prove_elf*, r0h_session_begin, r0h_prove_image,
 * r0h_lift and r0h_join return an error on a "sha-256" context.  r0h_ctx_hashfn returns a static string. */
const char* r0h_ctx_set_hashfn(r0h_ctx* ctx, const char* name);
const char* r0h_ctx_hashfn(const r0h_ctx* ctx);
const char* r0h_buf_alloc(r0h_ctx* ctx, size_t bytes, r0h_buf** out);
const char* r0h_buf_wrap(r0h_ctx* ctx, void* device_ptr, size_t bytes, r0h_buf** out); /* memory owned elsewhere */
const char* r0h_buf_slice(r0h_buf* parent, size_t offset_bytes, size_t bytes, r0h_buf** out);
const char* r0h_buf_free(r0h_buf* buf);
const char* r0h_buf_h2d(r0h_ctx* ctx, r0h_buf* dst, size_t offset_bytes, const void* src, size_t bytes);
const char* r0h_buf_d2h(r0h_ctx* ctx, const r0h_buf* src, size_t offset_bytes, void* dst, size_t bytes);
const char* r0h_buf_zero(r0h_ctx* ctx, r0h_buf* buf);
void* r0h_buf_device_ptr(const r0h_buf* buf);
size_t r0h_buf_bytes(const r0h_buf* buf);

/* ---- Hal: NTT family (risc0-zkp hal `batch_interpolate_ntt`, `batch_expand_into_evaluate_ntt`,
 *      `batch_bit_reverse`, `zk_shift`) ---- */
/* count columns of 2^po2 natural-order evaluations -> bit-reversed coefficients, in place */
const char* r0h_batch_interpolate_ntt(r0h_ctx* ctx, r0h_buf* io, uint32_t count, uint32_t po2);
/* count columns of 2^in_po2 bit-reversed coefficients -> natural-order evaluations on the 2^(in_po2+expand_bits) domain */
const char* r0h_batch_expand_into_evaluate_ntt(r0h_ctx* ctx, r0h_buf* out, const r0h_buf* in, uint32_t count,
                                               uint32_t in_po2, uint32_t expand_bits);
const char* r0h_batch_bit_reverse(r0h_ctx* ctx, r0h_buf* io, uint32_t count, uint32_t po2);
/* coefficient at bit-reversed position i is multiplied by 3^brev(i): f(x) -> f(3x) */
const char* r0h_zk_shift(r0h_ctx* ctx, r0h_buf* io, uint32_t count, uint32_t po2);
/* `batch_interpolate_ntt` followed by `zk_shift` as the prover issues them (prove/prover.rs commit_group), in one call: the shift
 * rides on the last pass of the inverse transform instead of sweeping the coefficients again.  Same words as the two calls. */
const char* r0h_batch_interpolate_ntt_zk_shift(r0h_ctx* ctx, r0h_buf* io, uint32_t count, uint32_t po2);

/* ---- Hal: Poseidon2 Merkle commitment (`hash_rows`, `hash_fold`; prove/merkle.rs) ---- */
/* rc: 24*29 canonical round constants, diag_m1: 24 canonical (mu_i - 1); the default table is compiled in */
const char* r0h_poseidon2_set_consts(r0h_ctx* ctx, const uint32_t* rc, const uint32_t* diag_m1);
/* The Poseidon2 kernels exist for two schedules of the conditional subtractions in the partial rounds' dot products: a tight one
 * derived from the compiled-in diagonal, and a safe one for any canonical table.  *tight = 1 when the table the context holds is
 * covered by the tight schedule (the default table is), 0 when its kernels run the safe one.  The digests are the same either way. */
const char* r0h_poseidon2_dot_schedule(const r0h_ctx* ctx, int* tight);
/* digests[r] = sponge(matrix[0][r], matrix[1][r], ..., matrix[cols-1][r]) for r < rows */
const char* r0h_hash_rows(r0h_ctx* ctx, r0h_buf* digests, const r0h_buf* matrix, uint32_t rows, uint32_t cols);
/* nodes[i] = H(nodes[2i] || nodes[2i+1]) for output_size <= i < 2*output_size (digest units) */
const char* r0h_hash_fold(r0h_ctx* ctx, r0h_buf* nodes, uint32_t output_size);
/* The top of a tree in at most two launches.  With the level of 2 * output_size digests in place (output_size a power of two, at
 * most 8192; anything else is refused, 0 does nothing) r0h_hash_fold_top fills the levels output_size, output_size / 2, .., 1 with the
 * words the loop `for (sz = output_size; sz >= 1; sz /= 2) r0h_hash_fold(ctx, nodes, sz)` leaves there, under the context's hash
 * suite: merkle_subtree_kernel folds a subtree per workgroup, a level handing its digests to the next through LDS, and workgroups
 * hand nothing to one another inside a launch -- 128 workgroups fold down to the level of 128 nodes, one workgroup in a second
 * launch folds from there to the root (one launch when output_size <= 64).  `nodes` as for r0h_hash_fold: 4 * output_size digests,
 * 16-byte aligned.
 * r0h_ctx_set_merkle_fused_tops(ctx, on != 0): r0h_merkle_build, and with it every tree the sequencer commits on this context,
 * runs r0h_hash_fold down to the level of 16384 parents and then r0h_hash_fold_top once, instead of r0h_hash_fold for all levels.
 * OFF BY DEFAULT; a context that was never told follows the environment (R0H_MERKLE_FUSED_TOPS=1: on).  The helper contexts of
 * sessions and of r0h_compress follow their owner.  The same nodes word for word, so the same seals and receipts; what it saves is
 * launches (profiles/r24/merkle_fused_tops.md).  r0h_hash_fold itself is the same with the switch on or off. */
const char* r0h_hash_fold_top(r0h_ctx* ctx, r0h_buf* nodes, uint32_t output_size);
const char* r0h_ctx_set_merkle_fused_tops(r0h_ctx* ctx, int on);
/* nodes has 2*rows digests: leaves at [rows, 2rows), root at index 1 */
const char* r0h_merkle_build(r0h_ctx* ctx, r0h_buf* nodes, const r0h_buf* matrix, uint32_t rows, uint32_t cols);
/* A tree kept as its top.  A Merkle path needs the whole tree only because the sibling at level l covers 2^l leaves; kept from the
 * root down to `levels` levels above the leaves a tree is 2 * rows >> levels digests (2^-levels of it), and the bottom `levels`
 * siblings of an opened leaf are hashed again from the 2^levels matrix rows of its subtree when the opening is made.
 * `levels` lies in [1, min(R0H_MERKLE_TOP_MAX_LEVELS, path_digests)], path_digests = log2(rows) - top_layer being the sibling digests
 * of an opening (the layer a seal carries instead of the root, the deepest one of at most 50 nodes, must lie in the kept part);
 * anything else is an error that names the bounds.
 * r0h_merkle_top: digests [0, 2 * rows >> levels) of the tree r0h_merkle_build left in `nodes` into top_out (index 0 unused, the root
 * at 1); stream-ordered like every operation of the context.
 * r0h_merkle_open_top: n_q packed openings into `out` -- per query the `cols` values of row idx_host[q], then the path_digests sibling
 * digests nodes[((row + rows) >> l) ^ 1], l = 0 .. path_digests - 1, as the sequencer packs them -- read from (matrix, top) under the
 * context's hash suite.  idx_host[q] < rows is checked here.  Every query's subtree must hash to the node the top has for it; if one
 * does not the openings are still written, *first_mismatch_out (optional; 0xffffffff otherwise) is the lowest such query and the call
 * returns "r0h_merkle_open_top: tree top does not match the matrix under query q (row r)".  Blocks until the report is back. */
#define R0H_MERKLE_TOP_MAX_LEVELS 8
const char* r0h_merkle_top(r0h_ctx* ctx, const r0h_buf* nodes, uint32_t rows, uint32_t levels, r0h_buf* top_out);
const char* r0h_merkle_open_top(r0h_ctx* ctx, r0h_buf* out, const r0h_buf* matrix, const r0h_buf* top, uint32_t levels,
                                const uint32_t* idx_host, uint32_t n_q, uint32_t rows, uint32_t cols, uint32_t* first_mismatch_out);
/* The way back: n_q packed openings in `openings` (device; what r0h_merkle_open_top and the sequencer pack: `cols` values, then the
 * path_digests sibling digests l = 0 .. path_digests - 1) hashed from the row upwards under the context's hash suite -- the row sponge
 * of r0h_hash_rows over the values, then per sibling H(cur || sib) when bit l of idx_host[q] is 0 and H(sib || cur) when it is 1.
 * reached_host[q][8] is the digest at node (idx_host[q] + rows) >> path_digests of the tree the opening belongs to, i.e. in the
 * layer a seal carries; path_digests = log2(rows) - top_layer as above, and path_digests == 0 is legal (the leaf digest is what is
 * reached).  idx_host[q] < rows and cols >= 1 are checked here.  The device computes digests and compares nothing: whether they are the committed
 * nodes is the caller's to say.  One launch on the context's stream; blocks until the digests are back. */
const char* r0h_merkle_climb(r0h_ctx* ctx, const r0h_buf* openings, const uint32_t* idx_host, uint32_t n_q, uint32_t rows,
                             uint32_t cols, uint32_t* reached_host);
/* The SHA-256 suite (recalled from risc0-zkp core/hash/sha and risc0-sys sha256.h; unpinned: the reference vendors neither).
 * A digest is 8 words, word j = bswap32 of SHA-256 state word j, so its bytes in memory are the standard big-endian digest; message
 * word i of a compression = bswap32 of input word i.  Pair: one compression of the IV over the 16 words a || b, no padding, no
 * length.  Slice (risc0 `hash_raw_data_slice`; what r0h_hash_rows computes per row): 16-word blocks chained from the IV, the last
 * partial block zero-filled, no length block, over the 32-bit words as the buffers hold them (Montgomery form); an EMPTY slice
 * hashes to the IV taken as a digest.  Digest words under this suite are arbitrary 32-bit values, not field elements.
 * The two suites on the host, by name (pure host code: a caller's own transcript hashing; "poseidon2" uses the compiled-in table
 * and wants canonical words): */
const char* r0h_hash_pair_host(const char* hashfn, const uint32_t a[8], const uint32_t b[8], uint32_t out[8]);
const char* r0h_hash_elems_host(const char* hashfn, const uint32_t* words, size_t n, uint32_t out[8]);

/* ---- Hal: streaming ops (`batch_evaluate_any`, `mix_poly_coeffs`, `eltwise_*`, `gather_sample`, `scatter`,
 *      `fri_fold`, `prefix_products`; core/poly.rs `poly_divide`) ---- */
/* out[k] = poly which[k] (2^po2 natural-order coefficients) evaluated at the extension point xs[4k..4k+4);
 * which / xs are small host arrays (upstream uploads them from the host as well) */
const char* r0h_batch_evaluate_any(r0h_ctx* ctx, const r0h_buf* coeffs, uint32_t po2, const uint32_t* which_host,
                                   const uint32_t* xs_host, uint32_t n_eval, r0h_buf* out);
const char* r0h_mix_poly_coeffs(r0h_ctx* ctx, r0h_buf* combos, const uint32_t mix_start[4], const uint32_t mix[4],
                                const r0h_buf* input, const uint32_t* combo_of_host, uint32_t input_count,
                                uint32_t po2);
const char* r0h_eltwise_add_elem(r0h_ctx* ctx, r0h_buf* out, const r0h_buf* a, const r0h_buf* b, uint32_t n);
const char* r0h_eltwise_copy_elem(r0h_ctx* ctx, r0h_buf* out, const r0h_buf* in, uint32_t n);
const char* r0h_eltwise_sum_extelem(r0h_ctx* ctx, r0h_buf* out, const r0h_buf* in, uint32_t count, uint32_t n);
/* cells still holding Elem::INVALID (0xffffffff) become zero (risc0 `eltwise_zeroize_elem`, run on the witness before commit) */
const char* r0h_eltwise_zeroize_elem(r0h_ctx* ctx, r0h_buf* io, uint32_t n);
const char* r0h_gather_sample(r0h_ctx* ctx, r0h_buf* dst, const r0h_buf* src, uint32_t idx, uint32_t size,
                              uint32_t stride);
const char* r0h_scatter(r0h_ctx* ctx, r0h_buf* into, const r0h_buf* index, const r0h_buf* offsets,
                        const r0h_buf* values, uint32_t n_index);
const char* r0h_fri_fold(r0h_ctx* ctx, r0h_buf* out, const r0h_buf* in, const uint32_t mix[4], uint32_t n_out);
/* The same operations with the operand placement of the risc0-zkp `Hal` trait (as recalled): `which` (u32), `xs` (extension
 * elements) and `combos` (u32) are device Buffers there, `scatter` takes host slices, `hash_fold` names both level sizes.  A Rust
 * `HipHal` calls these directly; the grouping the kernels rely on is made on the host, so the Buffer forms read the small index
 * buffers back themselves (one copy of a few KB). */
const char* r0h_batch_evaluate_any_buf(r0h_ctx* ctx, const r0h_buf* coeffs, uint32_t po2, const r0h_buf* which, const r0h_buf* xs,
                                       uint32_t n_eval, r0h_buf* out);
const char* r0h_mix_poly_coeffs_buf(r0h_ctx* ctx, r0h_buf* combos, const uint32_t mix_start[4], const uint32_t mix[4],
                                    const r0h_buf* input, const r0h_buf* combo_of, uint32_t input_count, uint32_t po2);
/* r0h_fri_fold with the mix read from device memory: the four words at mix_buf[mix_word_offset ..], e.g. where r0h_iop_draw_ext
 * wrote them (canonical words, as every field word on the device).  Refused when those four words would end beyond the buffer. */
const char* r0h_fri_fold_buf(r0h_ctx* ctx, r0h_buf* out, const r0h_buf* in, const r0h_buf* mix_buf, size_t mix_word_offset,
                             uint32_t n_out);
/* values[k] goes to into[offsets[k]] for index[0] <= k < index[n_index - 1] (offsets / values hold n_values host words) */
const char* r0h_scatter_slices(r0h_ctx* ctx, r0h_buf* into, const uint32_t* index, uint32_t n_index, const uint32_t* offsets,
                               const uint32_t* values, uint32_t n_values);
const char* r0h_hash_fold_io(r0h_ctx* ctx, r0h_buf* io, uint32_t input_size, uint32_t output_size);
const char* r0h_prefix_products(r0h_ctx* ctx, r0h_buf* io, uint32_t n);
const char* r0h_prefix_sums(r0h_ctx* ctx, r0h_buf* io, uint32_t n); /* io[i] = sum_{j <= i} io[j] over extension elements (AoS), n a power of two */
/* in-place synthetic division of an extension-coefficient polynomial (AoS, natural order) by (x - z) */
const char* r0h_poly_divide(r0h_ctx* ctx, r0h_buf* poly, uint32_t n, const uint32_t z[4], uint32_t remainder[4]);

/* ---- The device-challenge forms of steps 4-6 of a proof (what the sequencer runs under r0h_ctx_set_device_finish), callable on their
 * own.  r0h_fri_fold_buf's conventions: a challenge or a table in device memory is a (buffer, word offset) pair, refused when it would
 * end beyond the buffer and aligned to a word only; small index arrays are host arrays; no call waits for the stream unless it returns
 * host words.  Every word is a canonical Montgomery word; extension elements are four words. */
/* out[out_word_offset + 4k ..) = base^(exps ? exps[k] : k) for k < n; exps_buf may be NULL; x^0 = 1 for every x */
const char* r0h_ext_powers_buf(r0h_ctx* ctx, r0h_buf* out, size_t out_word_offset, const r0h_buf* base_buf, size_t base_word_offset,
                               const r0h_buf* exps_buf, size_t exps_word_offset, uint32_t n);
/* r0h_batch_evaluate_any whose request k is evaluated at point pt_idx_host[k] of a table of n_points points in device memory */
const char* r0h_batch_evaluate_any_points(r0h_ctx* ctx, const r0h_buf* coeffs, uint32_t po2, const uint32_t* which_host,
                                          const uint32_t* pt_idx_host, uint32_t n_eval, const r0h_buf* points_buf,
                                          size_t points_word_offset, uint32_t n_points, r0h_buf* out);
/* r0h_mix_poly_coeffs whose column c is weighed by mix^(first_exp + c), the mix read from four device words */
const char* r0h_mix_poly_coeffs_mixbuf(r0h_ctx* ctx, r0h_buf* combos, uint32_t first_exp, const r0h_buf* mix_buf,
                                       size_t mix_word_offset, const r0h_buf* input, const uint32_t* combo_of_host,
                                       uint32_t input_count, uint32_t po2);
/* polys: n-coefficient extension polynomials (AoS, natural order, n a power of two).  Job j divides polynomial poly_idx_host[j] in
 * place by (x - points_host[4j ..)); jobs on one polynomial are applied in the order given.  remainders_out (4 words per job, in the
 * order given; may be NULL) is filled by one blocking copy. */
const char* r0h_poly_divide_batch(r0h_ctx* ctx, r0h_buf* polys, uint32_t n, const uint32_t* poly_idx_host,
                                  const uint32_t* points_host, uint32_t n_jobs, uint32_t* remainders_out);
/* The same with job j's point named by its index pt_idx_host[j] in a device table, and no read-back: the word at
 * report_buf[report_word_offset] becomes 0, or 1 + the first job, in the order given, whose remainder is not zero (0 for no jobs) */
const char* r0h_poly_divide_batch_points(r0h_ctx* ctx, r0h_buf* polys, uint32_t n, const uint32_t* poly_idx_host,
                                         const uint32_t* pt_idx_host, uint32_t n_jobs, const r0h_buf* points_buf,
                                         size_t points_word_offset, uint32_t n_points, r0h_buf* report_buf,
                                         size_t report_word_offset);
/* the DEEP point table: points_out[i] = z * wpow_host[i] (base-field words) for i < n_backs, points_out[n_backs] = z^4; 1 <= n_backs <= 64 */
const char* r0h_deep_points_buf(r0h_ctx* ctx, r0h_buf* points_out, const r0h_buf* z_buf, size_t z_word_offset,
                                const uint32_t* wpow_host, uint32_t n_backs);
/* Pure host: the coefficients, low to high, of the polynomial of degree < n through n points (xs[4i ..), ys[4i ..)), 1 <= n <= 64,
 * the xs distinct */
const char* r0h_poly_interpolate_host(const uint32_t* xs, const uint32_t* ys, uint32_t n, uint32_t* out);
/* Every register's interpolant on the device.  eval_u and coeff_u_out hold n_taps + 16 extension elements: tap t was opened at point
 * tap_pt_host[t] of the table with the value eval_u[t]; register r is the taps [regs_host[2r], +regs_host[2r + 1]) and its interpolant
 * goes to coeff_u_out at its first tap; the last sixteen elements (CHECK's openings) are copied.  Refused before any launch: a
 * register of no or of more than 64 taps, registers that overlap or run past n_taps, a tap_pt outside the table.  The points of one
 * register must be distinct (not looked at: they are device words). */
const char* r0h_poly_interpolate_regs(r0h_ctx* ctx, r0h_buf* coeff_u_out, const r0h_buf* eval_u, const r0h_buf* points_buf,
                                      size_t points_word_offset, uint32_t n_points, const uint32_t* tap_pt_host,
                                      const uint32_t* regs_host, uint32_t n_regs, uint32_t n_taps);
/* The head fix-up of the DEEP combos: combos holds n_combos + 1 polynomials of 2^po2 extension coefficients (natural order), the
 * last one CHECK's.  With a running power of the mix per register in the order given, then one per CHECK column, coefficient i of
 * combo k loses sum over the registers (k, first tap, taps > i) of power * coeff_u[first tap + i]; CHECK's combo loses, at coefficient
 * 0, the sum over its sixteen columns.  regs_host: (combo, first tap, taps) per register.  coeff_u (n_taps + 16 elements) and the mix
 * are both host words (the *_host pointers, buffers NULL) or both device words (the *_host pointers NULL). */
const char* r0h_deep_subtract_heads(r0h_ctx* ctx, r0h_buf* combos, uint32_t po2, uint32_t n_combos, const uint32_t* regs_host,
                                    uint32_t n_regs, uint32_t n_taps, const uint32_t* coeff_u_host, const r0h_buf* coeff_u_buf,
                                    size_t coeff_u_word_offset, const uint32_t* mix_host, const r0h_buf* mix_buf,
                                    size_t mix_word_offset);

/* ---- CircuitHal: circuit blob (format: r0hip_circuit.h), witness generation, accumulation, eval_check ---- */
/* Pure host: emit the HIP source of the circuit's eval_check kernels (caller frees with r0h_free_error). */
const char* r0h_circuit_emit_hip(const uint32_t* blob, size_t n_words, char** source_out);
/* code_object_path: a gfx950 code object built from r0h_circuit_emit_hip's output, or NULL to compile in-process. */
const char* r0h_circuit_load(r0h_ctx* ctx, const uint32_t* blob, size_t n_words, const char* code_object_path,
                             r0h_circuit** out);
const char* r0h_circuit_free(r0h_circuit* c);
uint32_t r0h_circuit_group_size(const r0h_circuit* c, uint32_t group);
uint32_t r0h_circuit_n_global(const r0h_circuit* c);
uint32_t r0h_circuit_n_mix(const r0h_circuit* c);
uint32_t r0h_circuit_n_taps(const r0h_circuit* c);
const char* r0h_witgen(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, uint64_t seed, r0h_buf* code, r0h_buf* data,
                       uint32_t* global_out_host);
/* the same with the public inputs chosen by the caller: global_in[k] (a canonical Montgomery word) is planted at row 0 of the
 * column global k is read from, before the dependent columns are derived -- how a recursion-shaped segment is bound to the
 * digests of the seals it stands for (hyperfridge-r0_amd/recursion.py) */
const char* r0h_witgen_public(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, uint64_t seed, const uint32_t* global_in_host,
                              r0h_buf* code, r0h_buf* data);
const char* r0h_accum(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data,
                      const uint32_t* mix_host, r0h_buf* accum);
/* r0h_accum with the mix read from device memory, the circuit's n_mix words at mix_buf[mix_word_offset ..) -- where a device transcript
 * drew them (r0h_proof_begin_committed_enqueue, r0h_proof_late_device).  The same accumulation word for word; waits for nothing.
 * Canonicity of the device words is the producer's business (one of the device-challenge forms listed with r0h_ext_powers_buf). */
const char* r0h_accum_mixbuf(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data,
                             const r0h_buf* mix_buf, size_t mix_word_offset, r0h_buf* accum);
const char* r0h_eval_check(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* eval_accum,
                           const r0h_buf* eval_code, const r0h_buf* eval_data, const uint32_t* global_host,
                           const uint32_t* mix_host, const uint32_t poly_mix[4], r0h_buf* check);
/* r0h_eval_check with poly_mix read from device memory, the four words at poly_mix_buf[poly_mix_word_offset ..): its powers are made
 * on the device (one of the device-challenge forms listed with r0h_ext_powers_buf) */
const char* r0h_eval_check_mixbuf(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* eval_accum,
                                  const r0h_buf* eval_code, const r0h_buf* eval_data, const uint32_t* global_host,
                                  const uint32_t* mix_host, const r0h_buf* poly_mix_buf, size_t poly_mix_word_offset,
                                  r0h_buf* check);
/* ---- the witness checker: which constraint a witness violates, and where.  Term t of a circuit is the t-th AndEqz of its
 * constraint program once the AndCond gates are flattened into their inner terms -- numbered by the power of poly_mix it is folded
 * with, 0 <= t < r0h_circuit_n_terms -- and its value on row r of a 2^po2-row trace is the AndEqz value times the product of its
 * gates, tap (group, column, back) read from the WITNESS columns (natural row order, not the coset) at row (r - back) mod 2^po2.
 * The witness satisfies the circuit iff every term is zero on every row: no row is exempt, the circuit divides by x^N - 1.
 * r0h_check_witness evaluates every term on every row on the device (generated HIP like eval_check's, one lane per row) and reports
 * the violated terms in term order: `rows` rows leave the term non-zero, the first of them is `first_row`.  n_out is their number,
 * also beyond `capacity`.  accum == NULL checks only the terms that reach no ACCUM tap and no word of the mix -- what can be checked
 * before the mix is drawn (mix_host may then be NULL).  The checker's text (r0h_circuit_emit_hip_check, pure host) is compiled
 * in-process on first use and kept with the circuit; r0h_circuit_load_check loads a gfx950 code object built from that text instead.
 * Lookups of values outside their table are r0h_logup_multiplicities' to report, not the checker's; whether the tuples and lookups of
 * a log-derivative argument cancel is r0h_logup_check_balance's (below). */
typedef struct { uint32_t term, rows, first_row, reserved; } r0h_violation;
const char* r0h_circuit_emit_hip_check(const uint32_t* blob, size_t n_words, char** source_out);
const char* r0h_circuit_load_check(r0h_circuit* c, const char* code_object_path /* NULL: compile in-process now */);
uint32_t r0h_circuit_n_terms(const r0h_circuit* c);
const char* r0h_check_witness(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* accum, const r0h_buf* code,
                              const r0h_buf* data, const uint32_t* global_host, const uint32_t* mix_host, r0h_violation* out,
                              size_t capacity, size_t* n_out);
/* on != 0: from now on r0h_prove_segment*, r0h_proof_finish and the sessions of this context run the checker on every segment
 * before they commit its ACCUM group, and a violated segment returns an error that names the first violated term, its row count
 * and its first row instead of a seal no verifier accepts.  Between r0h_proof_begin* and r0h_proof_finish the CODE and DATA
 * witness buffers must then stay as they were given.  Off (the default): nothing is checked, seals and timing are unchanged. */
const char* r0h_ctx_set_check_witness(r0h_ctx* ctx, int on);
/* ---- the transcript on the device: the Fiat-Shamir generator of the context's hash suite over a state in device memory (a block
 * from the context's pool), driven in stream order.  What a sequencer does with a host transcript -- commit a root, hash and commit
 * words of the seal, draw a challenge, draw the query rows -- without a round trip: digests are read from device buffers (a tree's
 * root is its node 1, words [8, 16) of its nodes), challenges are written to device buffers where the next kernel reads them
 * (r0h_fri_fold_buf).  A handle belongs to the suite its context was on when it was made and is refused once the context has changed
 * suite.  r0h_iop_set_state / r0h_iop_state block: they are the hand-over between a host generator and this one.  The state is the
 * generator's words as the host holds them, then pool_used -- Poseidon2: 24 cells (Montgomery form) + pool_used <= 16, 25 words;
 * SHA-256: pool0[8], pool1[8] + pool_used <= 8, 17 words; a wrong count, a Poseidon2 cell >= p or a pool_used above that is refused.
 * Everything else is stream-ordered and touches no host memory; offsets count 32-bit words.
 *   r0h_iop_commit        mixes the digest at buf[word_offset .. +8)
 *   r0h_iop_commit_elems  the suite's hash of the n words at buf[word_offset ..] (r0h_hash_elems_host's), then the mix
 *   r0h_iop_draw_ext      `count` extension elements, 4 words each, to out[word_offset ..]
 *   r0h_iop_draw_queries  per query pos = bits(log2 domain) % domain; for the trees from the fifth on pos %= tree_rows[t], carried on
 *                         from tree to tree; the table idx_out[word_offset + t * n_queries + q].  domain a power of two, at most 16 trees.
 * r0h_ctx_set_device_transcript(ctx, on != 0): r0h_proof_finish (and every entry point that runs it: r0h_prove_segment*, sessions,
 * recursion) runs its last two steps, the FRI commitments and the queries, on such a transcript, with one read-back for both instead
 * of 2 R + 5 (R FRI rounds).  Off (the default): the steps are what they always were.  The seal is the same words either way.
 * r0h_ctx_blocking_waits: how many times the library has waited for this context's stream so far (every r0h_buf_d2h, r0h_sync and
 * wait inside an entry point). ---- */
typedef struct r0h_iop r0h_iop;
const char* r0h_iop_new(r0h_ctx* ctx, r0h_iop** iop_out);
const char* r0h_iop_free(r0h_iop* iop);
const char* r0h_iop_set_state(r0h_iop* iop, const uint32_t* words, size_t n);
const char* r0h_iop_state(r0h_iop* iop, uint32_t* words_out, size_t capacity, size_t* n_out);
const char* r0h_iop_commit(r0h_iop* iop, const r0h_buf* buf, size_t word_offset);
const char* r0h_iop_commit_elems(r0h_iop* iop, const r0h_buf* buf, size_t word_offset, size_t n);
const char* r0h_iop_draw_ext(r0h_iop* iop, r0h_buf* out, size_t word_offset, size_t count);
const char* r0h_iop_draw_queries(r0h_iop* iop, uint32_t domain, const uint32_t* tree_rows, uint32_t n_trees, uint32_t n_queries,
                                 r0h_buf* idx_out, size_t word_offset);
const char* r0h_ctx_set_device_transcript(r0h_ctx* ctx, int on);
const char* r0h_ctx_blocking_waits(const r0h_ctx* ctx, uint64_t* count_out);
/* ---- the balance check: which tuples a log-derivative argument (blob section LOGUP, r0hip_circuit.h) fails to cancel.  A witness
 * whose reads do not return what was written, whose boundary rows or multiplicities are off, still has running sums: the checker
 * above sees one chain-link term violated on the wrap row and nothing else.  This check names the fractions instead.
 * Only the links of the chain are looked at (accumulators whose `final` is 0xffffffff); an accumulator with a public total -- the
 * trace circuit's session sum -- balances across segments and the verifier only, and is left out (r0h_session_balance_*, below, is its check).  Fraction f = 4 * accumulator + slot,
 * 0 <= f < r0h_circuit_n_chain_fractions.  Fraction f contributes a TUPLE on row r iff its numerator n(f, r) is not zero.  The tuple's
 * CLASS is its denominator as a polynomial in the challenges: per challenge identity -- "one", (1, index), (2, index) -- the sum of the
 * values of the parts under it, identities whose sum is zero dropped; two tuples are of one class iff these vectors are equal (the
 * order of the parts, a challenge split over several parts, and a part whose value is zero make no difference).  The argument
 * BALANCES iff in every class the numerators sum to 0 mod p; a lookup and its table's multiplicity fraction are ordinary members of
 * one class.  DATA, CODE and the public inputs are read and no mix: the check can run before anything is committed.
 * Classes are told apart by a 62-bit fingerprint, two linear hashes over F_p of the per-identity sums under fixed weights: two given
 * distinct classes share it with probability about p^-2 < 2^-61 over the choice of weights, and two that do are reported as one (their
 * sums added).  The weights are public and fixed: this is a diagnostic for honest mistakes, not a verifier.
 * One r0h_imbalance per class that does not balance: (first_row, fraction) is the lexicographically smallest (row, fraction) among its
 * members, `net` the sum of the numerators as a canonical integer in [1, p) (1: produced once too often, p - 1: consumed once too
 * often), `members` its tuples (saturating at 2^32 - 1; more than 2^32 - 1 tuple slots, fractions x rows, are refused).  Entries come
 * in (first_row, fraction) order; *n_out counts all of them, also beyond `capacity`, and `out` then holds the `capacity` lowest.
 * Every field is a minimum, a sum or a count: the answer does not depend on scheduling.  po2 in [4, R0H_MAX_PO2]; a circuit without
 * chain fractions gives *n_out = 0.  code may be NULL for a circuit whose chain reads no CODE column.  The device takes its table
 * from the context's pool, sized from the tuples there are (load <= 1/2); a probe sequence that runs out of slots returns
 * "r0h_logup_check_balance: table full".  r0h_logup_check_balance_host is the same contract in plain loops over host words (Montgomery
 * form, column-major, as the device buffers hold them).  r0h_logup_check_balance_stats: of the context's last device call, the tuples,
 * the inserts that reached the global table (the rest were merged in LDS) and the table's slots. */
typedef struct { uint32_t fraction, first_row, net, members; } r0h_imbalance;
uint32_t r0h_circuit_n_chain_fractions(const r0h_circuit* c);
const char* r0h_logup_check_balance(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data,
                                    const uint32_t* global_host, r0h_imbalance* out, size_t capacity, size_t* n_out);
const char* r0h_logup_check_balance_host(const uint32_t* blob, size_t blob_words, uint32_t po2, const uint32_t* code,
                                         const uint32_t* data, const uint32_t* global, r0h_imbalance* out, size_t capacity,
                                         size_t* n_out);
const char* r0h_logup_check_balance_stats(const r0h_ctx* ctx, uint64_t stats_out[3]);
/* on != 0: from now on r0h_prove_segment*, r0h_proof_begin* and the sessions of this context run the balance check on the caller's
 * CODE and DATA witness before the DATA group is committed, and a segment that does not balance returns "...: fraction F does not
 * balance: net N over M tuples, first at row R; K classes in all".  Independent of r0h_ctx_set_check_witness.  Off (the default):
 * nothing is checked, seals and timing are unchanged. */
const char* r0h_ctx_set_check_balance(r0h_ctx* ctx, int on);
/* ---- the session balance: the same check for the accumulators the one above leaves out, those whose `final` is a public input (the
 * trace circuit's session sum, fractions 36..39: session:consume, session:produce, session:image, session:journal).  Their tuples
 * cancel across the segments of a session and against what the verifier adds (the program image's words, the journal's words), and
 * when they do not, r0h_receipt_verify_elf says verdict 14 and nothing else.  A tuple's class does not depend on the challenge's
 * value, so a whole session can be checked before the challenge exists.
 * The definitions are r0h_logup_check_balance's: fractions keep their global numbering f = 4 * accumulator + slot; fraction f on row r
 * of a segment is a tuple iff its numerator there is not zero; its class is, per challenge identity, the sum of the parts' values
 * under that identity.  The identities are those of the public-total accumulators in order of first appearance in the blob
 * (r0h_session_balance_identity: kind 0 "one", 1 a mix element, 2 four public inputs; at most 8, more is refused by _new, as are more
 * than 255 fractions in all).  A numerator or part that reads the VALUE of a late public input is refused by _new: late inputs do
 * not exist yet when this runs (a late input as a challenge's identity is what the session sum is made of).
 * A handle collects tuples: r0h_session_balance_add takes a segment's CODE / DATA witness on the device (handle made with a context;
 * the work goes on that context's stream, the buffers may belong to any context of the same device and must be complete),
 * r0h_session_balance_add_host the same as host words (handle made with ctx = NULL; Montgomery form, column-major), and
 * r0h_session_balance_add_tuples a list from outside -- the verifier's side: numerators[n] and values[n][n_identities], canonical words
 * (anything >= p is refused), n <= 2^24 a call.  r0h_session_balance_add_verifier_side is that list for the trace circuit: numerator
 * p - 1 for every image word of the ELF (source R0H_SESSION_SOURCE_IMAGE) and every journal word (R0H_SESSION_SOURCE_JOURNAL) under
 * R0H_SESSION_TAG_IMAGE / R0H_SESSION_TAG_JOURNAL, the fingerprints r0h_receipt_verify_elf forms; either of elf / journal may be
 * NULL to leave that side out.  Every tuple has a key (source, row, fraction): `source` is the caller's u32 per addition (the
 * sequencer: the segment's index), a tuple from outside has its index in its list as row and fraction 255.  The session BALANCES iff
 * every class's numerators sum to 0 mod p over everything added.  po2 in [4, R0H_MAX_PO2]; at most 2^32 - 1 tuples a handle.
 * r0h_session_balance_report: one entry per class that does not balance, in (source, row, fraction) order of the lowest member
 * (source, first_row, fraction); `net` in [1, p); `members` saturating at 2^32 - 1; values[0 .. n_values) the class's canonical
 * per-identity sums (the trace circuit: 1, -address, -lo, -hi, -tag or -segment).  *n_out counts all of them, `out` holds the
 * `capacity` lowest.  It may be called between additions and again after more.  Every field is a sum, a count, a minimum or
 * class-constant: the answer depends neither on scheduling nor on the order of the additions.  A circuit without public-total
 * accumulators gives *n_out = 0.  r0h_session_balance_message: NULL text when the session balances, else (caller frees with
 * r0h_free_error) "session fraction F does not balance: net N over M tuples, first in source S at row R, class (v0, v1, ...); K
 * classes in all" for the lowest entry.  r0h_session_balance_stats: tuples added, the table's slots, how often it grew, classes held.
 * Classes are told apart by the 62-bit fingerprint of the balance check above (same weights); two that collide are reported as one.
 * The weights are public and fixed: a diagnostic for honest mistakes, not a verifier -- r0h_receipt_verify_elf stays the judge.
 * The device keeps an open-addressed table of 64-byte slots that belongs to the handle, starts at 1,024 slots and is rehashed into
 * the next power of two whenever an addition would take the load above 1/2; "r0h_session_balance: table full" if a probe sequence
 * runs out all the same.  One handle is used from one thread at a time.
 * EXPORT AND MERGE: a handle's classes leave it and enter another one, so that ranks which each hold a share of a session's additions
 * reach the answer of one handle that had them all.  r0h_session_balance_export gives one 64-byte r0h_session_class per class HELD,
 * those that already balance included (a class balanced here still adds its members and its lowest member to the merged answer, a
 * class open here may be closed elsewhere): `key` the fingerprint, `net` the canonical residue of the numerators' sum in [0, p) (it
 * may be 0), `members` saturating at 2^32 - 1, (source, first_row, fraction) the lowest member, values[0 .. n_values) the per-identity
 * sums and zeros behind them.  Entries come in ascending `key` order, so two exports of the same content are the same bytes whatever
 * the scheduling or the order of the additions; *n_out counts the classes held and `out` receives the `capacity` lowest keys; an empty
 * handle gives 0.  Host and device handles alike.  The fingerprint of values v[0 .. n) under the handle's identities id[k] (kind << 32
 * | index, 0 for "one") is key = (h0 << 31 | h1) + 1 with h_j = sum_k w_j(id[k]) v[k] mod p and w_j(id) = 1 + (((splitmix64(
 * splitmix64(id) + 0xBA1A9CE (j + 1)) >> 32) (p - 1)) >> 32), splitmix64 the usual finaliser (add 0x9E3779B97F4A7C15; x ^= x >> 30,
 * times 0xBF58476D1CE4E5B9; x ^= x >> 27, times 0x94D049BB133111EB; x ^= x >> 31), all in 64-bit words.
 * r0h_session_balance_merge takes such a list from any handle made from the same blob and combines per class: the sums added mod p,
 * the members added (saturating at 2^32 - 1), the lowest member by (source, row, fraction), the values from whoever holds the class
 * first (the rule for colliding fingerprints above, unchanged).  Every one of these is associative and commutative: merging in any
 * order, pairwise or tree-wise, gives the report, the message, the class count and the export of one handle with every addition.  The
 * tuples counted by _stats grow by the merged members (saturating at 2^32 - 1, after which further additions are refused as above).
 * The same key may come more than once in a list; n may be 0; n <= 2^24 a call.  Refused by entry index, before anything is taken in:
 * n_values other than the handle's identity count, key 0, net or a value >= p, fraction > 255, first_row >= 2^24, a key that is not
 * the fingerprint of the entry's values.  The device counts first and grows its table when the merged load would pass 1/2. */
#define R0H_SESSION_SOURCE_IMAGE 0xfffffffeu
#define R0H_SESSION_SOURCE_JOURNAL 0xffffffffu
typedef struct { uint32_t source, fraction, first_row, net, members, n_values, values[8]; } r0h_session_imbalance;
typedef struct r0h_session_balance r0h_session_balance;
const char* r0h_session_balance_new(r0h_ctx* ctx /* NULL: a host handle */, const uint32_t* blob, size_t blob_words,
                                    r0h_session_balance** sb_out);
const char* r0h_session_balance_free(r0h_session_balance* sb);
uint32_t r0h_session_balance_n_identities(const r0h_session_balance* sb);
const char* r0h_session_balance_identity(const r0h_session_balance* sb, uint32_t k, uint32_t* kind_out, uint32_t* index_out);
const char* r0h_session_balance_add(r0h_session_balance* sb, uint32_t source, const r0h_circuit* c, uint32_t po2, const r0h_buf* code,
                                    const r0h_buf* data, const uint32_t* global_host);
const char* r0h_session_balance_add_host(r0h_session_balance* sb, uint32_t source, uint32_t po2, const uint32_t* code,
                                         const uint32_t* data, const uint32_t* global);
const char* r0h_session_balance_add_tuples(r0h_session_balance* sb, uint32_t source, const uint32_t* numerators, const uint32_t* values,
                                           size_t n);
const char* r0h_session_balance_add_verifier_side(r0h_session_balance* sb, const uint8_t* elf, size_t elf_len, const uint8_t* journal,
                                                  size_t journal_len);
const char* r0h_session_balance_report(r0h_session_balance* sb, r0h_session_imbalance* out, size_t capacity, size_t* n_out);
const char* r0h_session_balance_message(r0h_session_balance* sb, char** text_out);
const char* r0h_session_balance_stats(r0h_session_balance* sb, uint64_t stats_out[4]);
typedef struct { uint64_t key; uint32_t net, members, source, first_row, fraction, n_values; uint32_t values[8]; } r0h_session_class; /* 64 bytes */
const char* r0h_session_balance_export(r0h_session_balance* sb, r0h_session_class* out, size_t capacity, size_t* n_out);
const char* r0h_session_balance_merge(r0h_session_balance* sb, const r0h_session_class* classes, size_t n);
/* on != 0: from now on r0h_session_finish (and so r0h_prove_elf) of a trace-circuit session on this context checks the session balance
 * of all its segments' DATA witnesses (still resident, lean segments included; an evicted segment's is expanded again from its rows) with the verifier's side from the ELF and the run's
 * journal BEFORE the session challenge is derived, and a session that does not balance returns "r0h_prove_elf: session fraction F
 * does not balance: ..." (the message above) with its proofs aborted; the phase is `check_session` in the profile.  Single-rank
 * sessions only: a rank sees its own segments alone, and r0h_session_begin with parts > 1 refuses the switch (a multi-rank driver
 * would gather the tuples through the handle above).  The switch stays single-rank; the gathered form is beside it: every rank adds
 * its own share with r0h_session_balance_add_session (below, with the sessions), rank 0 the verifier's side, the ranks exchange their
 * r0h_session_balance_export lists and r0h_session_balance_merge the others' -- every rank then holds the same classes and gives the
 * same message (hyperfridge-r0_amd/driver.py: prove_elf_sharded(check_session=True)).  Off (the default): nothing is checked, seals, launches and timing are unchanged. */
const char* r0h_ctx_set_check_session(r0h_ctx* ctx, int on);

/* ---- the sequencer: risc0-circuit-rv32im `SegmentProver::prove` + risc0-zkp `Prover::{commit_group, finalize}` ---- */
/* code/data: witness columns resident in device memory ([group_size][2^po2]); global: host words.
 * seal_out receives *seal_words_out words (error if it exceeds seal_capacity_words). */
const char* r0h_prove_segment(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code,
                              const r0h_buf* data, const uint32_t* global_host, uint32_t* seal_out,
                              size_t seal_capacity_words, size_t* seal_words_out);
/* The same sequencer split around the accumulation step, as risc0-zkp's `Prover` is used by the segment driver
 * (commit_group(CODE), commit_group(DATA), draw the mix -> caller accumulates -> commit_group(ACCUM), finalize):
 * r0h_proof_begin commits CODE and DATA and returns the n_mix accumulation-mix words; the caller fills the ACCUM witness
 * ([group_size(ACCUM)][2^po2], e.g. with its own step_accum or r0h_accum) and hands it to r0h_proof_finish, which consumes
 * the proof object.  r0h_prove_segment == begin + r0h_accum + finish. */
typedef struct r0h_proof r0h_proof;
const char* r0h_proof_begin(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data,
                            const uint32_t* global_host, uint32_t* mix_out, r0h_proof** out);
const char* r0h_proof_finish(r0h_proof* proof, const r0h_buf* accum, uint32_t* seal_out, size_t seal_capacity_words,
                             size_t* seal_words_out);
const char* r0h_proof_abort(r0h_proof* proof);
/* r0h_ctx_set_device_finish(ctx, on != 0), off by default: r0h_proof_finish (and every entry point that runs it: r0h_prove_segment*,
 * sessions, image proofs, r0h_lift / r0h_join / r0h_compress) runs ALL its steps -- ACCUM, CHECK, the openings at z, DEEP, FRI, the
 * queries -- on a transcript on the device, whatever r0h_ctx_set_device_transcript says.  The host generator is handed over once the
 * accumulation mix has been drawn; poly_mix, z and the DEEP mix are drawn into device words, the tables that depend on them (the powers
 * of poly_mix, the points z * omega^-back and z^4, the registers' interpolants, the per-column powers and the head of the DEEP mix, the
 * division jobs) are filled by small kernels, and the remainders of the DEEP divisions are reduced to one word.  The seal is the same
 * words.  r0h_proof_finish then waits twice instead of six times: for the one read-back of every seal word the steps made, and for
 * the close of the per-phase profile (of a stream that has drained).  Helper contexts follow their owner's switch.
 *
 * With the switch on a proof can also be finished in two calls, so that one host thread keeps proofs in flight on several contexts:
 *   r0h_proof_finish_enqueue  enqueues the steps on the proof's stream and returns without waiting for it.  Refused unless the proof's
 *                             context has the switch on.  An error consumes the proof, as r0h_proof_finish's does.
 *   r0h_proof_finish_collect  the read-back, the host's verdicts (a DEEP remainder that is not zero, a tree top that does not match:
 *                             r0h_proof_finish's messages), the seal; consumes the proof either way.  Refused, and the proof left
 *                             as it is, if it was not enqueued.
 * r0h_proof_finish is one after the other.  Between the two calls `accum`, the CODE commitment (or the CODE columns) the proof was
 * begun with and, under r0h_ctx_set_check_witness, the witness buffers must stay as they were given: the steps read them on the
 * stream.  r0h_proof_abort of an enqueued proof waits for its stream before it releases anything.  With r0h_ctx_set_check_witness on,
 * the checker still reads its table back between accumulation and the ACCUM commitment: the seal is the same, the enqueue waits once.
 * The per-phase profile keeps its phase names and order: the phases' events are recorded at enqueue, the profile closes at collect (a
 * context reports one proof at a time: begin the next on it after the collect).  r0h_kernel_timing adds events around the launches and
 * no wait: the counts are the same with it on. */
const char* r0h_ctx_set_device_finish(r0h_ctx* ctx, int on);
const char* r0h_proof_finish_enqueue(r0h_proof* proof, const r0h_buf* accum);
const char* r0h_proof_finish_collect(r0h_proof* proof, uint32_t* seal_out, size_t seal_capacity_words, size_t* seal_words_out);
/* A proof waiting between its phases holds its DATA group three ways: coefficients, evaluations on the 4N coset (4/5 of the bytes:
 * 2 GiB for 128 columns of 2^20 rows) and Merkle nodes.  r0h_proof_shrink gives the evaluations back to the context's pool;
 * r0h_proof_finish computes them again from the coefficients (one expanding NTT, the same words: the seal does not change).  A
 * session does this by itself for the segments beyond its resident limit (r0h_ctx_set_session_resident_limit). */
const char* r0h_proof_shrink(r0h_proof* proof, size_t* bytes_freed_out);
size_t r0h_proof_resident_bytes(const r0h_proof* proof);
/* Late public inputs (blob section LATE: inputs that depend on commitments made outside this proof -- the trace circuit's session
 * challenge, derived from the DATA roots of ALL segments, and the segment's sum under it).  For such a circuit r0h_proof_begin stops
 * after the DATA commitment without drawing the mix: r0h_proof_data_root gives the root, r0h_proof_late takes the last n_late
 * public inputs (the transcript absorbs them; the seal's opening block receives them) and draws the accumulation mix into mix_out.
 * r0h_prove_segment[_committed] takes all public inputs at once and does the same internally.  r0h_proof_globals: all of them, as
 * the proof holds them. */
const char* r0h_proof_data_root(const r0h_proof* proof, uint32_t root_out[8]);
const char* r0h_proof_late(r0h_proof* proof, const uint32_t* late_globals, uint32_t* mix_out);
/* r0h_proof_late_device: r0h_proof_late with the late public inputs and the mix where the device has them, so that the host is out of
 * the loop from the DATA commitment on.  The generator goes up BEFORE the late inputs (r0h_ctx_set_device_finish hands it over after
 * the mix); `late` holds the circuit's n_late words on the device (exactly: a buffer of another size is refused), the generator absorbs
 * them there, and the n_mix mix words are drawn into device words: copied into mix_out (NULL: not wanted) and kept by the proof,
 * whose constraint check reads them there.  The call enqueues and returns: it waits for nothing and reads nothing back.  The late
 * words are seal words; they come home with the one read-back of r0h_proof_finish_collect, which patches them into the seal's
 * opening block -- the seal is word for word r0h_proof_late's -- and from then on r0h_proof_globals would have them.  Their
 * canonicity is checked on the device and reported at the collect: "late public input k is not canonical".  With n_late == 0 the form
 * is legal (`late` NULL or empty) and draws, on the device, the mix r0h_proof_begin has returned.  Refused: a second call, or one after
 * r0h_proof_late; a context whose hash suite changed since the begin; a context with r0h_ctx_set_device_finish off (the steps behind
 * the late inputs would ask the host generator).  A refusal leaves the proof as it was, and so does a step
 * that fails after the hand-over (the tail and the device generator are given back).  With r0h_ctx_set_check_witness on, the
 * checker takes host words: the enqueue reads the late inputs and the mix back for it (two more waits). */
const char* r0h_proof_late_device(r0h_proof* proof, const r0h_buf* late, r0h_buf* mix_out);
const char* r0h_proof_globals(const r0h_proof* proof, uint32_t* globals_out);
/* Control root of a program at trace size 2^po2: Merkle root of the committed CODE group (count columns of 2^po2 words),
 * computed exactly as the sequencer commits it.  What a verifier passes to r0h_verify_seal_bound. */
const char* r0h_code_root(r0h_ctx* ctx, const r0h_buf* code, uint32_t count, uint32_t po2, uint32_t root_out[8]);
/* The CODE group depends on (circuit, po2) only -- its Merkle root is the control root risc0 tabulates per po2 -- so it is committed
 * once and kept: bit-reversed zk-shifted coefficients, evaluations on the 4N coset, Merkle nodes, top layer and root.  Every proof of
 * that size on any context of the same device reads it (nothing writes it), and its seal is word for word the seal of
 * r0h_prove_segment on the same CODE columns.  r0h_code_commit_new blocks until the commitment is complete; free it only after
 * the proofs that use it have returned.  r0h_prove_segment == r0h_code_commit_new + r0h_prove_segment_committed. */
typedef struct r0h_code_commit r0h_code_commit;
const char* r0h_code_commit_new(r0h_ctx* ctx, const r0h_buf* code, uint32_t count, uint32_t po2, r0h_code_commit** out);
const char* r0h_code_commit_free(r0h_code_commit* cc);
const char* r0h_code_commit_root(const r0h_code_commit* cc, uint32_t root_out[8]); /* == r0h_code_root of the same columns */
const char* r0h_code_commit_columns(const r0h_code_commit* cc, const r0h_buf** columns_out); /* the committed columns themselves (device; owned by cc) */
const char* r0h_prove_segment_committed(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_code_commit* code,
                                        const r0h_buf* data, const uint32_t* global_host, uint32_t* seal_out,
                                        size_t seal_capacity_words, size_t* seal_words_out);
const char* r0h_proof_begin_committed(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_code_commit* code,
                                      const r0h_buf* data, const uint32_t* global_host, uint32_t* mix_out, r0h_proof** out);
/* A DATA commitment made once and carried as its tree top (r0h_merkle_top of the 4N-row DATA tree; `levels` as there).
 * r0h_proof_data_top: after a begin, the top of the proof's DATA tree into top_out (2 * 4N >> levels digests).
 * r0h_proof_begin_committed_top: r0h_proof_begin_committed for a DATA group whose top is known: the columns are interpolated and
 * evaluated, but no tree is built -- the seal's top layer and the transcript's root are read from `top` (copied: the caller's buffer
 * is free again when the call returns), so both receive the words of the first commitment.  r0h_proof_late, r0h_proof_shrink and
 * r0h_proof_finish take such a proof like any other; its openings are made by r0h_merkle_open_top's kernel, and if a queried subtree
 * of the evaluations does not hash to the top's node -- the top belongs to other columns -- r0h_proof_finish returns "r0h_proof_finish:
 * tree top does not match the matrix under query q (row r)" (the proof is consumed as always, the context stays usable).  The check
 * is made at the queries only: a top that is wrong elsewhere yields a seal whose DATA root is not the columns' -- the verifier remains
 * the judge of a seal.  r0h_proof_resident_bytes counts the kept top, not a whole tree. */
const char* r0h_proof_data_top(const r0h_proof* proof, uint32_t levels, r0h_buf* top_out);
const char* r0h_proof_begin_committed_top(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_code_commit* code,
                                          const r0h_buf* data, const uint32_t* global_host, const r0h_buf* top, uint32_t levels,
                                          uint32_t* mix_out, r0h_proof** out);
/* A proof's FIRST half enqueued: the hand-over before the DATA commitment, the earliest there is.  The generator goes to the device
 * once the seal's public block and CODE's top layer -- host words of a kept commitment -- are in; DATA is interpolated, evaluated and
 * hashed as ever, its top layer and root go device to device (the root into the device generator), and the call returns without
 * waiting for the stream.  The DATA top layer comes home with the one read-back of r0h_proof_finish_collect and stands in the seal
 * where the host form writes it: the seal is the same words.
 *   r0h_proof_begin_committed_enqueue      r0h_proof_begin_committed.  For a circuit without late inputs the mix is drawn on the device
 *                                          at once: copied into mix_out (a device buffer of n_mix words or more; NULL: not wanted) and
 *                                          kept by the proof; accumulate from it with r0h_accum_mixbuf / r0h_accum_public_device.
 *                                          For a circuit with late inputs the proof stops after DATA as ever and r0h_proof_late_device
 *                                          takes it from there (it finds the generator handed over; the host r0h_proof_late refuses).
 *   r0h_proof_begin_committed_top_enqueue  the same from a kept DATA tree top (r0h_proof_begin_committed_top): no tree is built.
 *   r0h_proof_data_root                    on such a proof WAITS: node 1 is read back, eight words, the first time it is asked for.
 *   r0h_proof_data_root_device             the root's eight words to out[word_offset ..), device to device, no wait (any proof): gather
 *                                          the roots of many proofs and read them back once.
 *   r0h_prove_segment_committed_enqueue    begin-enqueue + the late inputs (from global_host) + the accumulation + r0h_proof_finish_enqueue:
 *                                          a whole proof submitted.  The proof keeps its ACCUM witness until the collect.
 *   r0h_prove_segment_collect              r0h_proof_finish_collect of it: the seal of r0h_prove_segment_committed, word for word.
 * A whole proof then waits twice: the read-back and the close of its profile.  All of them need r0h_ctx_set_device_finish on and a
 * kept CODE commitment (r0h_code_commit_new: the columns forms commit CODE with a read-back that waits, and there is no enqueue form
 * of them); both are refused by name before anything is launched, and a refusal changes nothing.  An error behind that consumes the
 * proof (what was launched runs out first).  r0h_proof_late_device on such a proof cannot take the hand-over back: a step of it that
 * fails leaves the proof fit for r0h_proof_abort only.  Until the collect `data`, the CODE commitment, a kept top's matrix and
 * mix_out stay as they were given.  r0h_proof_abort waits for the proof's stream first; r0h_proof_shrink and
 * r0h_proof_resident_bytes work as on any proof (the shrink waits, as ever; the bytes include the ACCUM witness a proof submitted whole keeps).  A context whose hash suite changed since the begin is
 * refused by r0h_proof_late_device and the finish, as for every proof.  With r0h_ctx_set_check_balance on, the begin runs the checker
 * first, read-backs and all; with r0h_ctx_set_check_witness on, the finish-enqueue reads the mix, the late inputs (if any) and the
 * checker's table back: up to three waits more.  Phase names and their order are those of the blocking forms. */
const char* r0h_proof_begin_committed_enqueue(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_code_commit* code, const r0h_buf* data,
                                              const uint32_t* global_host, r0h_buf* mix_out, r0h_proof** out);
const char* r0h_proof_begin_committed_top_enqueue(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_code_commit* code, const r0h_buf* data,
                                                  const uint32_t* global_host, const r0h_buf* top, uint32_t levels, r0h_buf* mix_out, r0h_proof** out);
const char* r0h_proof_data_root_device(const r0h_proof* proof, r0h_buf* out, size_t word_offset);
const char* r0h_prove_segment_committed_enqueue(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_code_commit* code, const r0h_buf* data,
                                                const uint32_t* global_host, r0h_proof** out);
const char* r0h_prove_segment_collect(r0h_proof* proof, uint32_t* seal_out, size_t seal_capacity_words, size_t* seal_words_out);
/* Per-phase device time (ms) of the last proof on this context that came out -- r0h_prove_segment*, r0h_proof_finish, or the session check
 * that closes a profile; names are static strings, *n_out names and times, valid until the next one closes.  A proof in flight, aborted or failed
 * leaves the report as it was; a context that has closed none reports *n_out = 0. */
const char* r0h_last_profile(r0h_ctx* ctx, const char*** names_out, const float** ms_out, uint32_t* n_out);

/* ---- verifier: risc0-zkp verify/mod.rs as reached from `receipt.verify(image_id)` (host/src/main.rs:622-624,
 * verifier/src/main.rs:124-126).  Pure host code: no context, no GPU.  Returns NULL when the check itself ran (the outcome is
 * in *verdict_out: R0H_VERIFY_OK or the first reason for rejection) and an error string only for unusable arguments
 * (malformed circuit blob, non-canonical Poseidon2 tables).  p2_round_constants [29][24] / p2_diag_m1 [24] are canonical words,
 * or both NULL for the compiled-in risc0 table.  *po2_out (optional) receives the trace size the seal claims. ---- */
#define R0H_VERIFY_OK 0
#define R0H_VERIFY_TRUNCATED 1
#define R0H_VERIFY_BAD_PO2 2
#define R0H_VERIFY_MERKLE_GROUP 3
#define R0H_VERIFY_CHECK_MISMATCH 4
#define R0H_VERIFY_FRI_MERKLE 5
#define R0H_VERIFY_FRI_GOAL 6
#define R0H_VERIFY_FRI_FINAL 7
#define R0H_VERIFY_TRAILING 8
#define R0H_VERIFY_BAD_ELEM 9
#define R0H_VERIFY_CODE_ROOT 10
const char* r0h_verify_seal(const uint32_t* blob, size_t blob_words, const uint32_t* p2_round_constants,
                            const uint32_t* p2_diag_m1, const uint32_t* seal, size_t seal_words, int* verdict_out,
                            uint32_t* po2_out);
/* The same check, bound to a program: risc0-zkp verify/mod.rs calls `check_code(po2, root)` on the CODE commitment, which the
 * rv32im verifier answers from its table of control roots (one per po2).  expected_code_root (8 canonical words, e.g. from
 * r0h_code_root) is compared with the root the seal commits to; a mismatch is R0H_VERIFY_CODE_ROOT.  NULL skips the comparison
 * (then nothing ties the seal to a program: r0h_verify_seal is that form and is meant for tests of the proof system alone).
 * code_root_out (optional) receives the root found in the seal. */
const char* r0h_verify_seal_bound(const uint32_t* blob, size_t blob_words, const uint32_t* p2_round_constants,
                                  const uint32_t* p2_diag_m1, const uint32_t* seal, size_t seal_words,
                                  const uint32_t* expected_code_root, int* verdict_out, uint32_t* po2_out,
                                  uint32_t* code_root_out);
/* r0h_verify_seal_bound for a seal made under the named hash suite ("poseidon2": the compiled-in table; "sha-256": digest words in
 * the seal -- Merkle tops, path siblings, the roots -- are arbitrary 32-bit values, only field-element positions are held to < p).
 * A seal of the other suite is rejected with a verdict, like any other seal that does not verify. */
const char* r0h_verify_seal_hashfn(const uint32_t* blob, size_t blob_words, const char* hashfn, const uint32_t* seal,
                                   size_t seal_words, const uint32_t* expected_code_root, int* verdict_out, uint32_t* po2_out,
                                   uint32_t* code_root_out);
/* the same, also giving the DATA group's Merkle root as the seal's transcript recomputes it (the session challenge of the trace
 * circuit is derived from these roots: csrc/claim.cpp) */
const char* r0h_verify_seal_roots(const uint32_t* blob, size_t blob_words, const uint32_t* seal, size_t seal_words,
                                  const uint32_t* expected_code_root, int* verdict_out, uint32_t* po2_out, uint32_t* data_root_out);
/* n seals of one circuit, verified with the device hashing their Merkle openings.  `seals` holds the n seals back to back,
 * seal_words[s] words each; expected_code_roots (optional) holds one control root of 8 words per seal (the seals of a batch may
 * differ in po2); verdicts_out[n], po2_out[n] (optional) and data_roots_out[n][8] (optional) are what r0h_verify_seal_roots gives
 * for each seal, verdict and reason equal for every input.  The verifier walks every seal on the host as ever -- transcript,
 * constraint identity, DEEP, FRI folds, final polynomial, and of every opening the row bound and the canonical-word checks -- but puts
 * the hashing of the openings off: the openings of all n seals go to the device in one upload and are hashed by one launch of
 * r0h_merkle_climb's kernel on the context's stream, and the host compares each digest that comes back with the node of the top
 * layer it read from the seal.  The verdict is the reject code of the first opening in seal order that fails, else the walk's own.
 * The device decides nothing.  Suite and Poseidon2 table are the context's, so a SHA-256 context verifies SHA-256 seals.
 * ctx == NULL hashes the collected openings on the host (Poseidon2, the compiled-in table): the same seam without a device. */
const char* r0h_verify_seals_on(r0h_ctx* ctx, const uint32_t* blob, size_t blob_words, const uint32_t* seals, const size_t* seal_words,
                                size_t n, const uint32_t* expected_code_roots, int* verdicts_out, uint32_t* po2_out,
                                uint32_t* data_roots_out);
/* The control root of a circuit's own CODE columns at trace size 2^po2, computed on the HOST from the blob alone (circuits with a
 * column program: the CODE columns r0h_witgen generates) -- the same 8 words as r0h_code_root / r0h_code_commit_root on the device.
 * A verifier that has the circuit need not be told its control roots (risc0's verifier has them compiled in).  Seconds at po2 = 20. */
const char* r0h_control_root_host(const uint32_t* blob, size_t blob_words, const uint32_t* p2_round_constants, const uint32_t* p2_diag_m1,
                                  uint32_t po2, uint32_t root_out[8]);
/* the same under the named hash suite: what r0h_code_root gives on a context set to it */
const char* r0h_control_root_host_hashfn(const uint32_t* blob, size_t blob_words, const char* hashfn, uint32_t po2, uint32_t root_out[8]);
const char* r0h_verify_reason(int verdict); /* static string, do not free */
/* Poseidon2 sponge (compiled-in table) over a seal's words (all canonical field elements, else an error): the 8-word name a
 * recursion step commits to */
const char* r0h_seal_digest(const uint32_t* seal, size_t seal_words, uint32_t digest_out[8]);
/* The same sponge laid out as the rows of the recursion circuit's in-circuit hash (r0hip_circuit.h SPONGE; tools/sponge_component.py):
 * 65 columns (st[24], aux[24], in[16], act) of 2^po2 rows, 30 rows per permutation, zero behind the last one.  Host code; r0h_lift /
 * r0h_join plant exactly this into a node's witness, so that the digest among the node's public inputs is computed inside its proof.
 * Refused: words that are not canonical field elements, more words than the trace has rows for (30 rows per 16 words). */
const char* r0h_sponge_trace(const uint32_t* words, size_t n_words, uint32_t po2, uint32_t* cols_out /* [65][2^po2] */);
/* The same rows made on the device, as r0h_lift / r0h_join / r0h_prove_image plant them: the host runs the sequential chain once (24
 * words per permutation go up through the context's pinned ring), one lane per trace row expands them, rows behind the last permutation
 * included (written as zero).  cols_out: a device buffer of 65 * 2^po2 words.  Stream-ordered.  Refuses what r0h_sponge_trace refuses,
 * in the same words. */
const char* r0h_sponge_trace_device(r0h_ctx* ctx, const uint32_t* words, size_t n_words, uint32_t po2, r0h_buf* cols_out);

/* ---- data formats either side of the path (SURVEY.md 8(a) a0', a0'', a18): pure host code ----
 * serde word stream of a String: [u32 LE length][utf8][zero padding to 4] -- what `ExecutorEnv::builder().write(&s)` feeds the
 * guest (host/src/main.rs:389-417) and what `env::commit(&String)` leaves in `receipt.journal.bytes` (host/src/main.rs:258-267).
 * r0h_serde_encode_str with out == NULL only reports the size. */
const char* r0h_serde_encode_str(const uint8_t* utf8, size_t len, uint8_t* out, size_t capacity, size_t* out_len);
const char* r0h_serde_decode_str(const uint8_t* bytes, size_t n, size_t* str_off, size_t* str_len, size_t* consumed /* may be NULL */);
/* The input stream `ExecutorEnv::builder().write(..)` builds (host/src/main.rs:389-417: 12 Strings and one Vec<u8>), as the u32
 * words the guest's `env::read()` calls consume (methods/guest/src/main.rs:159-171).  A Vec<u8> goes one word per byte. */
typedef struct r0h_env r0h_env;
const char* r0h_env_new(r0h_env** out);
const char* r0h_env_write_str(r0h_env* e, const uint8_t* utf8, size_t len);
const char* r0h_env_write_u8_seq(r0h_env* e, const uint8_t* bytes, size_t len);
const char* r0h_env_words(const r0h_env* e, const uint32_t** words, size_t* n_words);
const char* r0h_env_free(r0h_env* e);
/* hyperfridge's reading of the commitment in a journal: first '{' .. last '}' (host/src/main.rs:258-267, verifier/src/main.rs:176-185) */
const char* r0h_journal_commitment_span(const uint8_t* bytes, size_t n, size_t* off, size_t* len);
/* Receipt JSON as `serde_json::to_string(&receipt)` writes it (host/src/main.rs:251-252) and `serde_json::from_slice` reads it
 * (verifier/src/main.rs:118-119).  Pinned by the reference's fixtures: {"inner":"Fake","journal":{"bytes":[u8..]}}, re-serialised
 * byte for byte.  The composite form follows risc0-zkvm 3.x as recalled (unpinned):
 *   {"inner":{"Composite":{"segments":[{"seal":[u32..],"index":n,"hashfn":"poseidon2","verifier_parameters":"<hex>","claim":
 *     {"pre":{"Value":{"pc":n,"merkle_root":"<hex>"}},"post":{..},"exit_code":{"Halted":0}|{"Paused":0}|"SystemSplit"|"SessionLimit",
 *      "input":{"Pruned":"<hex>"},"output":{"Pruned":"<hex>"}|{"Value":null}}},..],"assumption_receipts":[],"verifier_parameters":"<hex>"}},
 *    "journal":{"bytes":[..]},"metadata":{"verifier_parameters":"<hex>"}}
 * (serde_json is human-readable, so a risc0 `Digest` is a hex string).  Segments without a claim (this library's round-1 files) are
 * still read.  r0h_receipt_to_json's output is serde_json's compact form (caller frees it with r0h_free_error). */
#define R0H_RECEIPT_FAKE 0
#define R0H_RECEIPT_COMPOSITE 1
typedef struct r0h_receipt r0h_receipt;
/* risc0-binfmt `SystemState` and risc0-zkvm `ReceiptClaim`, flattened (field names, tags and digest layout are recalled from the
 * public risc0 sources: unpinned, see csrc/claim.cpp).  exit_system / exit_user: Halted(u) = (0, u), Paused(u) = (1, u),
 * SystemSplit = (2, 0), SessionLimit = (2, 2).  input_digest / output_digest: Digest::ZERO stands for None. */
typedef struct { uint32_t pc; uint8_t merkle_root[32]; } r0h_system_state;
typedef struct {
  r0h_system_state pre, post;
  uint32_t exit_system, exit_user;
  uint8_t input_digest[32];
  uint8_t output_digest[32];
} r0h_receipt_claim;
/* SHA-256 (FIPS 180-4) and risc0's tagged-struct digests over it */
const char* r0h_sha256(const uint8_t* bytes, size_t n, uint8_t digest_out[32]);
const char* r0h_tagged_struct(const char* tag, const uint8_t* down_digests /* n_down x 32 bytes */, size_t n_down, const uint32_t* data,
                              size_t n_data, uint8_t digest_out[32]);
const char* r0h_system_state_digest(const r0h_system_state* st, uint8_t digest_out[32]);
/* Output{journal, assumptions}.digest; assumptions_digest NULL = no assumptions (Digest::ZERO) */
const char* r0h_output_digest(const uint8_t* journal, size_t n, const uint8_t* assumptions_digest, uint8_t digest_out[32]);
const char* r0h_claim_digest(const r0h_receipt_claim* claim, uint8_t digest_out[32]);
/* the eight public-input words (canonical Montgomery words) that name a claim in a seal: Poseidon2 sponge over the sixteen 16-bit
 * halves of its digest.  The prover plants them as globals[0..8) (r0h_witgen_public / its own witness generator). */
const char* r0h_claim_globals(const uint8_t claim_digest[32], uint32_t globals_out[8]);

const char* r0h_receipt_parse(const char* json, size_t n, r0h_receipt** out);
const char* r0h_receipt_new(int kind, const uint8_t* journal, size_t journal_len, r0h_receipt** out);
const char* r0h_receipt_add_segment(r0h_receipt* rc, const uint32_t* seal, size_t seal_words, uint32_t index);
/* the same with the segment's claim (risc0-zkvm `SegmentReceipt.claim`); verifier_parameters may be NULL (zeros) */
const char* r0h_receipt_add_segment_claim(r0h_receipt* rc, const uint32_t* seal, size_t seal_words, uint32_t index,
                                          const r0h_receipt_claim* claim, const uint8_t* verifier_parameters);
const char* r0h_receipt_free(r0h_receipt* rc);
int r0h_receipt_kind(const r0h_receipt* rc);
size_t r0h_receipt_n_segments(const r0h_receipt* rc);
const char* r0h_receipt_journal(const r0h_receipt* rc, const uint8_t** bytes, size_t* n);
const char* r0h_receipt_segment(const r0h_receipt* rc, size_t i, const uint32_t** seal, size_t* seal_words, uint32_t* index);
/* *has_claim_out = 0 when the segment was read from a receipt without claims (claim_out untouched) */
const char* r0h_receipt_segment_claim(const r0h_receipt* rc, size_t i, r0h_receipt_claim* claim_out, int* has_claim_out);
const char* r0h_receipt_to_json(const r0h_receipt* rc, char** json_out);
/* `receipt.verify(image_id)` (verifier/src/main.rs:124-126, host/src/main.rs:622-624) for a composite receipt, as risc0-zkvm
 * receipt/composite.rs does it: every seal verifies against the control root of its trace size (control_roots: n_roots records of
 * 9 words [po2, root[8]], from r0h_code_root), its public inputs name the segment's claim, the segments chain (index, SystemSplit,
 * post-state == next pre-state), the last claim's output commits to SHA-256(journal.bytes) and exits Halted(0)/Paused(0), and the
 * first pre-state's digest is image_id (32 bytes; with NULL the outcome is at best R0H_RECEIPT_V_UNBOUND, never OK).  A seal of the
 * trace circuit must also carry its claim's first and last pc as public inputs 8 and 9.  Pure host code.  Returns NULL when the check
 * ran: *verdict_out is R0H_RECEIPT_V_*; *segment_out (optional) the segment at fault; *seal_verdict_out (optional) the R0H_VERIFY_*
 * code when the verdict is R0H_RECEIPT_V_SEAL. */
#define R0H_RECEIPT_V_OK 0
#define R0H_RECEIPT_V_NOT_COMPOSITE 1
#define R0H_RECEIPT_V_SEAL 2
#define R0H_RECEIPT_V_NO_CONTROL_ROOT 3
#define R0H_RECEIPT_V_NO_CLAIM 4
#define R0H_RECEIPT_V_CLAIM_MISMATCH 5
#define R0H_RECEIPT_V_CHAIN 6
#define R0H_RECEIPT_V_JOURNAL 7
#define R0H_RECEIPT_V_IMAGE_ID 8
#define R0H_RECEIPT_V_EXIT_CODE 9
#define R0H_RECEIPT_V_NO_BINDING 10
#define R0H_RECEIPT_V_HASHFN 11
#define R0H_RECEIPT_V_UNBOUND 12 /* everything else holds, but image_id was NULL: the receipt is not tied to a program */
#define R0H_RECEIPT_V_SESSION 13       /* trace circuit: a seal's session number / closing flags / challenge are not the session's */
#define R0H_RECEIPT_V_SESSION_SUM 14   /* trace circuit: the segments' sums, the program image and the journal do not balance */
#define R0H_RECEIPT_V_NEEDS_IMAGE 15   /* trace circuit: everything else holds, but the program image (the ELF) was not given */
#define R0H_RECEIPT_V_IMAGE_PROOF 16   /* r0h_receipt_verify_image: the image proof is missing, rejected, or about another image / session */
const char* r0h_receipt_verify(const r0h_receipt* rc, const uint32_t* blob, size_t blob_words, const uint32_t* control_roots,
                               size_t n_roots, const uint8_t* image_id, int* verdict_out, size_t* segment_out, int* seal_verdict_out);
/* `receipt.verify(image_id)` for receipts over the trace circuit (circuits/trace.r0c), where the program is bound by a session-wide
 * memory argument instead of in-circuit hashing: the verifier is given the ELF itself (the reference's host embeds it as
 * HYPERFRIDGE_ELF next to HYPERFRIDGE_ID, methods/build.rs:2).  Beyond what r0h_receipt_verify checks: the image id of the ELF is
 * the first pre-state; every seal carries the session challenge derived from ALL seals' DATA roots and early public inputs; segment
 * numbers count up, the closing segments are the run's last (or segments without cycles after it) with increasing address ranges;
 * and the sum of the segments' session sums equals the sum over the ELF's image words and the journal's words of their tuples'
 * fractions -- so every first touch of a word finds the image (or zero), every later one what the previous segment left, and the
 * journal is what the COMMIT rows read.  With r0h_receipt_verify (no ELF) such a receipt is at best R0H_RECEIPT_V_NEEDS_IMAGE. */
const char* r0h_receipt_verify_elf(const r0h_receipt* rc, const uint32_t* blob, size_t blob_words, const uint32_t* control_roots,
                                   size_t n_roots, const uint8_t* elf, size_t elf_len, int* verdict_out, size_t* segment_out,
                                   int* seal_verdict_out);
/* The same verdict WITHOUT the ELF: the receipt's image proof (r0h_receipt_image_proof; r0h_prove_elf attaches one when the context
 * was given the image circuit) stands for the image -- `receipt.verify(image_id)` as the reference calls it, with 32 bytes.  The image
 * seal is verified against `image_blob` bound to `image_control_root` (NULL: derived from the blob at the size the seal names). */
const char* r0h_receipt_verify_image(const r0h_receipt* rc, const uint32_t* blob, size_t blob_words, const uint32_t* control_roots,
                                     size_t n_roots, const uint32_t* image_blob, size_t image_blob_words, const uint32_t* image_control_root,
                                     const uint8_t* image_id, int* verdict_out, size_t* segment_out, int* seal_verdict_out);
const char* r0h_receipt_set_image_proof(r0h_receipt* rc, const uint32_t* seal, size_t seal_words);
const char* r0h_receipt_image_proof(const r0h_receipt* rc, const uint32_t** seal_out, size_t* seal_words_out); /* NULL / 0 when there is none */
/* r0h_receipt_verify_elf / _image with the seals' Merkle openings hashed on `ctx` (a Poseidon2 context; its table is the one the
 * seals are held to): the segment seals that the walk can reach, and the image seal when there is one, are verified as one batch of
 * r0h_verify_seals_on before the receipt is walked.  Same arguments otherwise, same verdict, segment and seal verdict for every input. */
const char* r0h_receipt_verify_elf_on(r0h_ctx* ctx, const r0h_receipt* rc, const uint32_t* blob, size_t blob_words, const uint32_t* control_roots,
                                      size_t n_roots, const uint8_t* elf, size_t elf_len, int* verdict_out, size_t* segment_out,
                                      int* seal_verdict_out);
const char* r0h_receipt_verify_image_on(r0h_ctx* ctx, const r0h_receipt* rc, const uint32_t* blob, size_t blob_words, const uint32_t* control_roots,
                                        size_t n_roots, const uint32_t* image_blob, size_t image_blob_words, const uint32_t* image_control_root,
                                        const uint8_t* image_id, int* verdict_out, size_t* segment_out, int* seal_verdict_out);
const char* r0h_receipt_verify_reason(int verdict); /* static string, do not free */
/* The image id as text, the reference's way (host/src/main.rs:445-449, verifier/src/main.rs:131-143, host/out/IMAGE_ID.hex): eight
 * u32 words printed `{:08x}`, each stored little-endian in the 32-byte digest (`Digest::from([u32; 8])`) -- NOT the digest's bytes
 * in order.  Strict: exactly 64 hex digits. */
const char* r0h_image_id_from_hex(const char* hex, uint8_t image_id_out[32]);
const char* r0h_image_id_to_hex(const uint8_t image_id[32], char hex_out[65]);

/* ---- EBICS pre-processing: what data/checkResponse.sh does with xmllint / openssl / zlib-flate / unzip
 * before `host` starts (host/src/main.rs:143-151), as pure host code.  r0h_ebics_parse cuts the guest's four XML inputs out of a
 * response and canonicalises them exactly as the script does (checkResponse.sh:151-155, 192, 200, 221); the checks below are the
 * script's (and the guest's) checks; r0h_ebics_env_inputs frames the thirteen `ExecutorEnv` inputs (host/src/main.rs:389-417).
 * Pinned by the reference's fixtures data/test/test.xml-* (tests/test_ebics.py). ---- */
typedef struct r0h_ebics r0h_ebics;
#define R0H_EBICS_AUTHENTICATED 0       /* "<xml>-authenticated": header, DataEncryptionInfo, ReturnCode, [TimestampBankParameter] */
#define R0H_EBICS_SIGNED_INFO 1         /* "<xml>-SignedInfo" */
#define R0H_EBICS_SIGNATURE_VALUE 2     /* "<xml>-SignatureValue" (element with its tags) */
#define R0H_EBICS_ORDER_DATA 3          /* "<xml>-OrderData" (element with its tags) */
#define R0H_EBICS_DIGEST_VALUE 4        /* text of <ds:DigestValue> */
#define R0H_EBICS_SIGNATURE_BIN 5       /* base64-decoded signature */
#define R0H_EBICS_TRANSACTION_KEY_BIN 6 /* base64-decoded <TransactionKey> (the RSA ciphertext) */
#define R0H_EBICS_ORDER_DATA_BIN 7      /* base64-decoded order data (AES ciphertext) */
#define R0H_EBICS_PAYLOAD_ZIP 8         /* decrypted and inflated payload (after r0h_ebics_decrypt_order_data) */
const char* r0h_ebics_parse(const char* xml, size_t n, r0h_ebics** out);
const char* r0h_ebics_free(r0h_ebics* e);
const char* r0h_ebics_part(const r0h_ebics* e, int which, const uint8_t** bytes, size_t* n);
/* each check returns NULL when it ran; *ok_out = 1 passed / 0 failed */
const char* r0h_ebics_check_digest(const r0h_ebics* e, int* ok_out);
const char* r0h_ebics_verify_bank_signature(const r0h_ebics* e, const char* pub_bank_pem, size_t pem_len, int* ok_out);
/* raw_block: the RSA-decrypted transaction key with its padding ("<xml>-TransactionKeyDecrypt.bin"); key_out: the AES key in it */
const char* r0h_ebics_check_transaction_key(const r0h_ebics* e, const char* pub_client_pem, size_t pem_len, const uint8_t* raw_block,
                                            size_t raw_len, uint8_t key_out[16], int* ok_out);
/* the two private-key steps of the script (checkResponse.sh:231-236, 276-279; `openssl pkeyutl -decrypt / -sign`): the raw
 * RSA-decrypted transaction key block ("<xml>-TransactionKeyDecrypt.bin") with the AES key in it, and the witness signature as the
 * `xxd -p` text of "<xml>-Witness.hex" (free with r0h_free_error).  PKCS#8 or PKCS#1 PEM; plain square-and-multiply, not constant
 * time: a tool for the key's owner, as the openssl command line in the script is. */
const char* r0h_ebics_decrypt_transaction_key(const r0h_ebics* e, const char* client_private_pem, size_t pem_len, uint8_t* raw_out,
                                              size_t raw_capacity, size_t* raw_len_out, uint8_t key_out[16], int* ok_out);
const char* r0h_ebics_witness_sign(const r0h_ebics* e, const char* witness_private_pem, size_t pem_len, char** hex_out);
const char* r0h_ebics_verify_witness(const r0h_ebics* e, const char* pub_witness_pem, size_t pem_len, const char* witness_hex,
                                     size_t hex_len, int* ok_out);
/* AES-128-CBC (zero IV) -> RFC 1950 inflate -> ZIP members; an error means the key or the data is wrong */
const char* r0h_ebics_decrypt_order_data(r0h_ebics* e, const uint8_t key[16]);
size_t r0h_ebics_n_documents(const r0h_ebics* e);
const char* r0h_ebics_document(const r0h_ebics* e, size_t i, const char** name, const uint8_t** data, size_t* n);
/* modulus and exponent of a PEM "PUBLIC KEY" as decimal strings (host/src/main.rs:383-387); free both with r0h_free_error */
const char* r0h_rsa_public_key_decimal(const char* pem, size_t pem_len, char** modulus_out, char** exponent_out);
const char* r0h_ebics_env_inputs(const r0h_ebics* e, const char* pub_bank_pem, size_t bank_len, const char* client_private_pem,
                                 size_t client_len, const uint8_t* decrypted_tx_key, size_t tx_len, const char* iban,
                                 const char* host_info, const char* witness_hex, size_t witness_len, const char* pub_witness_pem,
                                 size_t pub_witness_len, const char* verbose, r0h_env** out);
/* known-answer hooks: one AES-128 block (FIPS 197), one RFC 1950 stream (caller frees *out with r0h_free_error) */
/* The input word stream of this library's own camt53 guest (tools/guest_camt53.py, circuits/guest_camt53.elf) from the same things the
 * reference's host gives its guest (host/src/main.rs:389-417): the parsed response, the three public keys, the decrypted transaction
 * key block (256 bytes: r0h_ebics_decrypt_transaction_key or the script's TransactionKeyDecrypt.bin), the witness signature (hex),
 * iban and host info, the commitment form (1: with the three keys, as the current receipts; 0: the earlier form).  words_out is
 * malloc'd: release it with r0h_free_error (as every buffer this library hands out).  With it the compiled hosts go from response.xml
 * to a receipt without Python. */
const char* r0h_camt53_guest_input(const r0h_ebics* e, const char* pub_bank_pem, size_t bank_len, const char* pub_client_pem,
                                   size_t client_len, const char* pub_witness_pem, size_t witness_len, const uint8_t* tx_key_block,
                                   size_t tx_key_len, const char* witness_hex, size_t witness_hex_len, const char* iban,
                                   const char* host_info, uint32_t form, uint32_t** words_out, size_t* n_out);
const char* r0h_aes128_block(const uint8_t key[16], const uint8_t in[16], int decrypt, uint8_t out[16]);
const char* r0h_zlib_inflate(const uint8_t* in, size_t n, uint8_t** out, size_t* out_len);

/* ---- RV32IM executor, segmenter and preflight trace (csrc/rv32im.cpp): the part of `prover.prove(env, elf)`
 * that runs before prove_segment.  Pure host code.  Instruction semantics are the RISC-V specification's; the ecall ABI, the cycle
 * model and the page Merkle root are this library's own documented choices (risc0's are recalled in outline only: see the source).
 * Guest memory is the low 1 GiB (an access or a pc above it traps).
 * ecall (a7): 0 HALT(a0) | 1 READ_WORDS(a0 = dst, a1 = n words) | 2 COMMIT(a0 = src, a1 = n words) | 3 CYCLES -> a0 | 4 PAUSE(a0);
 * every ecall cycle reads a7 and a0 (its two register reads).  The two transfers move ONE word per cycle and keep no state
 * outside the registers: while a1 = j > 0 the instruction re-executes (next pc = pc) -- it moves word j - 1 of the buffer
 * (address a0 + 4 (j - 1)) and writes a1 = j - 1 -- and with a1 = 0 it falls through to pc + 4 (n + 1 cycles for n words).  So
 * every cycle has at most one memory access and is a function of what it reads -- what the trace circuit constrains -- and a
 * transfer of any length can be cut between two segments.  The buffer ends up in stream order; a1 is 0 afterwards, a0 as it was;
 * a0 is word-aligned. ---- */
typedef struct r0h_vm r0h_vm;
typedef struct {
  uint32_t segment_po2;     /* a segment holds at most 2^segment_po2 rows (cycles + paging + boundary rows) */
  uint32_t page_in_cycles;  /* charged once per 1 KiB page first touched in a segment */
  uint32_t page_out_cycles; /* charged once per page written in a segment */
  uint32_t keep_trace;      /* record one r0h_preflight_row per cycle and the boundary rows of every segment */
  uint64_t max_cycles;      /* stop (R0H_VM_LIMIT, ExitCode::SessionLimit) after this many cycles; 0 = no limit */
  uint32_t boundary_rows;   /* charge one row per distinct register / memory word touched in a segment: the rows the trace
                             * circuit spends on the first and last value of each (set by r0h_prove_elf for a trace circuit) */
  uint32_t reserved;
} r0h_vm_limits;
typedef struct {
  uint32_t index, exit_system, exit_user, pages_in, pages_out, boundary_rows;
  uint32_t closing, reserved; /* closing = 1: the boundary rows of this segment close the session (see r0h_preflight_bound) */
  uint64_t user_cycles, paging_cycles;
  r0h_system_state pre, post; /* pc + Merkle root of memory before the first and after the last instruction of the segment */
} r0h_vm_segment;
#define R0H_MEM_NONE 0
#define R0H_MEM_READ 1
#define R0H_MEM_WRITE 2
/* What witness generation replays, one row per cycle (18 words): the instruction, its register operands and result, its memory
 * transaction, and -- for the memory-consistency argument of the trace circuit -- when each of the five things the cycle touches
 * was last touched in this segment.  Access k of cycle c carries the timestamp 5 c + k + 1 (k = 0 x[rs1] read, 1 x[rs2] read,
 * 2 x[rd] write, 3 the memory word, 4 the instruction fetch); prev[k] is the timestamp of the previous access to the same
 * register / word in this segment, 0 when this is the first.  rs1 / rs2 are instruction bits 15..19 / 20..24 whatever the format. */
typedef struct {
  uint32_t cycle;  /* within the segment */
  uint32_t pc, insn, next_pc;
  uint32_t rs1_value, rs2_value;
  uint32_t rd, rd_before, rd_after;                    /* rd = 0: no register written */
  uint32_t mem_kind, mem_addr, mem_before, mem_after; /* word-aligned address, the word before and after */
  uint32_t prev[5];
} r0h_preflight_row;
/* One per register / memory word a segment touched, in increasing address order: the value the segment found there, the value it
 * left, and the timestamp of its last access.  addr: word index (byte address / 4) for memory, R0H_REG_BASE + i for x[i]. */
#define R0H_REG_BASE 0x10000000u
#define R0H_BOUND_IMAGE 1u
/* prev_seg: the number (index + 1) of the segment that last touched the address before this one, 0 if none did.  In a CLOSING
 * segment (the run's last, or segments of boundary rows only that follow it when those do not fit) there is a row for every word
 * and register the session touched and for every word of the program image, touched or not: init_value is what the address held
 * when the run began (the image's word, or zero) and flags says whether it is an image word. */
typedef struct { uint32_t addr, first_value, last_value, last_ts, prev_seg, init_value, flags, reserved; } r0h_preflight_bound;
/* the journal is a window of guest memory: journal word i is the word at R0H_JOURNAL_BASE + 4 i when COMMIT names it */
#define R0H_JOURNAL_BASE 0x20000000u
#define R0H_VM_HALTED 0
#define R0H_VM_PAUSED 1
#define R0H_VM_LIMIT 2
const char* r0h_vm_new(r0h_vm** out);
const char* r0h_vm_free(r0h_vm* vm);
const char* r0h_vm_load(r0h_vm* vm, uint32_t addr, const uint32_t* words, size_t n);
const char* r0h_vm_load_elf(r0h_vm* vm, const uint8_t* elf, size_t n); /* ELF32 LE RISC-V executable: PT_LOAD segments + entry */
/* the image id of an ELF -- risc0-binfmt `compute_image_id`, what `methods/build.rs` embeds as HYPERFRIDGE_ID: the digest of the
 * SystemState a run starts from (r0h_prove_elf returns the same 32 bytes).  Pure host code. */
const char* r0h_compute_image_id(const uint8_t* elf, size_t n, uint8_t image_id_out[32]);
const char* r0h_vm_set_input(r0h_vm* vm, const uint32_t* words, size_t n); /* the ExecutorEnv word stream (r0h_env_words) */
const char* r0h_vm_set_pc(r0h_vm* vm, uint32_t pc);
const char* r0h_vm_set_reg(r0h_vm* vm, uint32_t i, uint32_t value);
uint32_t r0h_vm_reg(const r0h_vm* vm, uint32_t i);
uint32_t r0h_vm_pc(const r0h_vm* vm);
const char* r0h_vm_read(const r0h_vm* vm, uint32_t addr, uint32_t* words, size_t n);
/* runs to HALT / PAUSE / max_cycles, cutting segments on the way; a guest trap (illegal instruction, misaligned access, unknown
 * ecall) is an error string, as a guest panic is an Err from `prove` (host/src/main.rs:327-330) */
const char* r0h_vm_run(r0h_vm* vm, const r0h_vm_limits* limits, int* exit_kind_out, uint32_t* exit_code_out);
/* the same run one segment at a time (a prover takes each segment as it is cut, while the guest runs on): returns after the next
 * segment is complete; *finished_out = 1 with the last one (then exit_kind / exit_code are set).  The limits of the first call hold
 * for the whole run.  r0h_vm_release_trace drops the rows of a segment that has been taken (its r0h_vm_segment stays). */
const char* r0h_vm_run_segment(r0h_vm* vm, const r0h_vm_limits* limits, int* finished_out, int* exit_kind_out, uint32_t* exit_code_out);
const char* r0h_vm_release_trace(r0h_vm* vm, size_t i);
size_t r0h_vm_n_segments(const r0h_vm* vm);
uint64_t r0h_vm_cycles(const r0h_vm* vm);
const char* r0h_vm_segment_info(const r0h_vm* vm, size_t i, r0h_vm_segment* out);
const char* r0h_vm_preflight(const r0h_vm* vm, size_t i, const r0h_preflight_row** rows, size_t* n);
const char* r0h_vm_boundary(const r0h_vm* vm, size_t i, const r0h_preflight_bound** rows, size_t* n);
/* ---- the trace circuit, version 5 (circuits/trace.r0c, tools/trace_circuit.py): a circuit whose DATA group IS the preflight trace of a
 * segment.  R0H_TRACE_COLUMNS columns of 2^po2 rows (po2 >= 16: two 2^16-row lookup tables sit in the CODE group), column-major,
 * Montgomery words: first the cycles (one row each), then the boundary rows (one per register / word touched; in a closing segment
 * one per word the whole session touched and per image word), then blank rows.  Per cycle: pc, next pc, the instruction word as
 * decoded fields with a one-hot opcode and funct3, five accesses -- the fetch, x[rs1], x[rs2], x[rd], the memory word, in this order of
 * timestamps (5 c + 1..5) -- each with the two looked-up limbs of the distance to the access it follows, and the work words of the
 * arithmetic units: two operands byte by byte with their AND (U, V), two words as 16-bit halves (Z, W), carries.  Ten quantities the
 * constraints speak of are linear forms of these columns rather than columns (the last flag of each one-hot group, V's low byte, Z's
 * low half, the memory and transfer flags, four of the five consumed timestamps): 128 columns, eight Poseidon2 permutations per
 * committed row.  What the circuit constrains (tools/trace_circuit.py trace_constraints: 302 polynomials of degree <= 5 over 193
 * taps; csrc/trace.hpp fills the columns):
 *   - the cycles form one contiguous run from the public first pc to the public last pc in the public number of cycles;
 *   - WHAT EVERY INSTRUCTION DOES: the word decodes to exactly one RV32IM instruction (an illegal encoding has no satisfying row);
 *     the value written to rd, the word written to memory, the address of a load / store and the next pc are the ones the ISA
 *     prescribes for the operands read -- a 32-bit adder over 16-bit halves (ADD[I], AUIPC, addresses, JALR; backwards for SUB,
 *     SLT[I][U] and the branches), AND / OR / XOR through a byte-AND lookup table, a byte-limb multiplier with a range-checked carry
 *     chain (MUL[H[S]U], the shifts as products with 2^s or 2^(32-s), DIV[U] / REM[U] as quotient x divisor + remainder = dividend
 *     with |remainder| < |divisor|), byte and half lanes of the narrow loads and stores; an ecall reads a7 and a0, and what it writes
 *     (a1 counted down and one word of the buffer for the transfers, a0 for CYCLES, nothing for HALT / PAUSE) is where its
 *     function says.  Every word written to a register or to memory is range-checked (16-bit lookups) or composed of such parts;
 *   - MEMORY CONSISTENCY over registers (x0 included: a register nothing ever writes) and memory: every access consumes the tuple
 *     (address, value, timestamp, space) the previous access to that address produced and produces one with a larger timestamp; the
 *     boundary rows produce each address's first tuple (timestamp 0) and consume its last; consumed = produced as multisets, by a
 *     log-derivative argument: every tuple is a fraction +-1 / (alpha - address - b1 lo - b2 hi - b3 t - b4 space) of ONE running
 *     sum through the ACCUM group that wraps around the trace, together with the lookups' fractions and the tables' multiplicities
 *     (csrc/logup.hip).  Boundary addresses (below 2^28 + 32) strictly increase, so an address has ONE history.  Hence a register
 *     or word read returns what was last written to it, and the instruction word at a pc is the word in memory;
 *   - THE SESSION (round 4): a boundary row consumes (address, value found, number of the segment that held the address before --
 *     an EARLIER one) and produces (address, value left, own number); the rows of a closing segment produce the address's initial
 *     tuple (address, initial value, 0) instead -- zero unless the row says "image word", then it also names (address, word) as an
 *     image tuple; an active COMMIT row names (address, word read) as a journal tuple.  These are fractions under a challenge all
 *     segments share (late public inputs R0H_TRACE_GAMMA..: derived from every segment's DATA root, r0h_session_challenge); their
 *     sum over the segment is the public input at R0H_TRACE_SUM.  r0h_receipt_verify_elf adds the segments' sums and compares with
 *     the sum over the ELF's image words and the journal's words: the tuples balance iff every first touch finds the image (or
 *     zero), every later one what the previous holder left, and the journal is what the COMMIT rows read.
 * What it does NOT constrain: the WORDS READ_WORDS moves (input words are the host's to choose, as in risc0) and the value CYCLES
 * returns.  It is this library's circuit for this library's executor, not risc0's rv32im circuit.  Public inputs
 * (R0H_TRACE_GLOBALS): 8 words naming the segment's ReceiptClaim (r0h_claim_globals), first pc, pc after the last cycle, number of
 * cycles, how the segment ends (0: cut, 1: HALT, 2: PAUSE -- such an ecall is the last cycle of its segment), that being non-zero,
 * the two halves of the exit code (a0), the segment's number (index + 1), whether it closes the session, number x (1 - closing), the
 * first and last boundary address; LATE (absorbed after the DATA commitment): the session challenge (16 words), the segment's sum
 * (4).  r0h_receipt_verify[_elf] holds them against the claims and against one another.  Trace sizes 2^16..2^21 rows (timestamps < 2^24). ---- */
#define R0H_TRACE_COLUMNS 128
#define R0H_TRACE_GLOBALS 40
#define R0H_TRACE_LATE_GLOBALS 20 /* the last 20 public inputs: the session's challenge (16 words) and the segment's sum under it (4) */
#define R0H_TRACE_GAMMA 20         /* where the session challenge sits among the public inputs; the segment's sum follows at 36 */
#define R0H_TRACE_SUM 36
#define R0H_SESSION_TAG_IMAGE ((1u << 20) + 1)   /* the "segment" coordinate of an image word's tuple in the session sum */
#define R0H_SESSION_TAG_JOURNAL ((1u << 20) + 2) /* ... and of a journal word's */
#define R0H_SESSION_RECORD_WORDS 28 /* what a segment contributes to the session challenge: its 20 early public inputs, its DATA root */
#define R0H_TRACE_MIN_PO2 16      /* the lookup tables have 2^16 rows */
#define R0H_TRACE_MAX_PO2 21
const char* r0h_trace_column_name(uint32_t column); /* static string; NULL past the last column */
/* host reference of the witness (what tests compare the device kernel with): data_out = R0H_TRACE_COLUMNS * 2^po2 words;
 * globals_out[8..15) = first pc, pc after the last cycle, cycles, how the segment ends, that being non-zero, exit code halves (globals_out[0..8) are left to the caller: the claim) */
const char* r0h_vm_trace_witness(const r0h_vm* vm, size_t i, uint32_t po2, uint32_t* data_out, uint32_t globals_out[R0H_TRACE_GLOBALS]);
/* the same on the device: the compact rows (72 B per cycle, 16 B per boundary row) are uploaded and one thread per row expands
 * them into the column-major Montgomery DATA group in `data` (R0H_TRACE_COLUMNS * 2^po2 words).  Stream-ordered; the host arrays
 * may be released when the call returns. */
typedef struct { uint32_t number /* index + 1 */, closing, idle_pc /* where a segment without cycles stands */, reserved; } r0h_trace_segment;
const char* r0h_trace_witgen(r0h_ctx* ctx, const r0h_preflight_row* rows, size_t n_rows, const r0h_preflight_bound* bounds,
                             size_t n_bounds, uint32_t po2, const r0h_trace_segment* segment, r0h_buf* data,
                             uint32_t globals_out[R0H_TRACE_GLOBALS]);
/* The two halves of r0h_trace_witgen, for a caller that expands the same rows more than once (a session that evicts a committed
 * segment and commits it again: r0h_ctx_set_session_device_limit).  r0h_trace_rows_upload checks the arguments as r0h_trace_witgen
 * does, copies the rows, the boundary rows and the expansion's tables into one device block owned by the handle, and gives the early
 * public inputs; the host arrays may be released when it returns.  r0h_trace_rows_expand launches the expansion from that block into
 * `data` (R0H_TRACE_COLUMNS * 2^po2 words, same device): stream-ordered on the handle's context, not synchronised, any number of
 * times, the same words every time -- those r0h_trace_witgen leaves.  r0h_trace_rows_bytes: the device bytes the handle keeps (72 per
 * cycle, 32 per boundary row, the tables; 0 for NULL).  The handle holds a reference on its context; r0h_trace_rows_free releases it
 * and the block (NULL is fine).  r0h_trace_witgen == upload + expand + free with one wait at the end. */
typedef struct r0h_trace_rows r0h_trace_rows;
const char* r0h_trace_rows_upload(r0h_ctx* ctx, const r0h_preflight_row* rows, size_t n_rows, const r0h_preflight_bound* bounds,
                                  size_t n_bounds, uint32_t po2, const r0h_trace_segment* segment, r0h_trace_rows** rows_out,
                                  uint32_t globals_out[R0H_TRACE_GLOBALS]);
const char* r0h_trace_rows_expand(const r0h_trace_rows* rows, r0h_buf* data);
size_t r0h_trace_rows_bytes(const r0h_trace_rows* rows);
const char* r0h_trace_rows_free(r0h_trace_rows* rows);
/* ---- the log-derivative argument of a circuit (blob section LOGUP): lookups, memory tuples, session tuples as fractions of running
 * sums in ACCUM.  Multiplicities: the table columns of DATA are filled from the lookups the rows make -- BEFORE the DATA group is
 * committed (r0h_trace_witgen and r0h_vm_trace_witness leave them zero).  Totals: the accumulators whose challenges are public inputs
 * (the trace circuit's session sum) are summed over the rows and written into global_io where the circuit reads them -- once those
 * challenges are known, before r0h_proof_late.  r0h_accum_public is r0h_accum for circuits whose accumulation reads public inputs.
 * Both multiplicity functions keep the contract of include/r0hip_circuit.h (LOGUP): entry v of a table counts the rows whose lookup
 * numerator is 1 and whose value is v; a numerator other than 0 or 1, a value outside its table on such a row, or more than p - 1
 * lookup slots of one table is an error. */
const char* r0h_logup_multiplicities(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, r0h_buf* data, const uint32_t* global);
const char* r0h_logup_multiplicities_host(const uint32_t* blob, size_t blob_words, uint32_t po2, uint32_t* data, const uint32_t* global);
const char* r0h_logup_totals(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, uint32_t* global_io);
const char* r0h_accum_public(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data,
                             const uint32_t* global, const uint32_t* mix, r0h_buf* accum);
/* The two with the public inputs (and the mix) in device buffers, for a caller whose challenges never reach the host
 * (r0h_proof_late_device): `globals` holds the circuit's n_global words, `mix` its n_mix words.  A small kernel multiplies the tape's
 * coefficients by the public inputs they take and fills the tape's challenge block from both buffers; the term kernel is the one of
 * the host forms.  r0h_logup_totals_device leaves every total in the words of globals_io the circuit reads it from, device to device.
 * Neither reads anything back nor waits for the stream: tape, tables and temporaries return to the context's pool in stream order.
 * Canonicity of the device words is the producer's business (r0h_proof_late_device reports it).  r0h_accum_public_device is for
 * circuits with a log-derivative argument; the synthetic circuits' r0h_accum takes its mix from the host. */
const char* r0h_logup_totals_device(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, r0h_buf* globals_io);
const char* r0h_accum_public_device(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data,
                                    const r0h_buf* globals, const r0h_buf* mix, r0h_buf* accum);
const char* r0h_vm_journal(const r0h_vm* vm, const uint8_t** bytes, size_t* n);
/* the ReceiptClaim of segment i: system states and exit code from the run, Output{journal} on the last segment */
const char* r0h_vm_segment_claim(const r0h_vm* vm, size_t i, r0h_receipt_claim* out);

/* ---- `default_prover().prove(env, elf)` (host/src/main.rs:420-423) in one call: execute the ELF on the word stream of `env`,
 * cut the run into segments of at most 2^segment_po2 rows, prove each at the smallest trace size that holds it, return the
 * composite receipt with every segment's claim bound to its seal, plus the image id `receipt.verify` is given.  A guest that
 * traps, exits non-zero or exceeds max_cycles is an error, as it is an Err from `prove`; max_cycles = 0 selects
 * R0H_DEFAULT_SESSION_LIMIT (risc0's executor has a session limit as well).
 * With the trace circuit (circuits/trace.r0c) every seal attests the segment it stands for: the executor keeps the preflight
 * rows, r0h_trace_witgen expands them on the device, the public inputs carry the claim, the first and last pc and the cycle count,
 * and the guest runs ahead on its own thread while the device proves.  With any other circuit the witness is that circuit's
 * synthetic column program with the claim planted (the seal then proves only that a satisfying trace naming the claim exists). ---- */
#define R0H_DEFAULT_SESSION_LIMIT ((uint64_t)1 << 32)
/* How many bytes of committed DATA evaluations the sessions begun on this context keep on the device between their two phases; the
 * segments beyond it keep coefficients and Merkle nodes only (0.6 instead of 2.7 GiB per 2^20-row segment) and are evaluated again
 * when their proofs are finished (about 2 ms each).  0 = the default: an eighth of the device's memory.  The reference's own run is
 * 37 segments (docs/runtime.md: session_cycles = 39,265,237): 100 GiB resident without a limit, per session in flight. */
const char* r0h_ctx_set_session_resident_limit(r0h_ctx* ctx, uint64_t bytes);
/* How many bytes the committed segments of a trace-circuit session begun on this context may keep on the device between its two
 * phases.  A segment counts as its DATA witness, what its proof holds (r0h_proof_resident_bytes, after the shrink of a lean segment)
 * and its rows handle.  A segment whose commitment would take the count above the limit is EVICTED as soon as its DATA root and early
 * public inputs are recorded: its proof is aborted, its witness released, and only its compact rows stay on the device (r0h_trace_rows:
 * a seventeenth of what a lean segment holds; they are on top of the limit).  r0h_session_finish commits such a segment a second time
 * on its lane -- commitment is deterministic: the root must be the recorded one, else "r0h_session_finish: segment I committed another
 * root when it was replayed" -- and finishes it like any other; a lane replays one segment at a time, so a session holds at most the
 * limit, its evicted rows and one segment in flight per lane.  The seals are the ones an unlimited session makes.  The cost is one more
 * expansion and DATA commitment per evicted segment.  0 = the default: no limit, nothing is kept or counted differently.  Taken per
 * session at r0h_session_begin; other circuits are proved at once and have nothing to evict.
 * r0h_last_session_device: of the last session finished on this context -- segments evicted, segments replayed, the largest value
 * the count reached (bytes; kept with or without a limit), the most bytes held in rows handles (0 without a limit).
 * r0h_ctx_session_held_bytes: what the unfinished sessions begun on this context hold on the device right now by the same count,
 * evicted segments' rows included; 0 once every session is finished or freed. */
const char* r0h_ctx_set_session_device_limit(r0h_ctx* ctx, uint64_t bytes);
const char* r0h_last_session_device(r0h_ctx* ctx, uint64_t out[4]);
uint64_t r0h_ctx_session_held_bytes(const r0h_ctx* ctx);
/* What an evicted segment keeps besides its rows: with levels in [1, R0H_MERKLE_TOP_MAX_LEVELS] the top of its DATA tree
 * (r0h_proof_data_top: 2 * 4N >> levels digests -- 4 MiB for 2^20 rows at levels = 6 -- copied device to device before the proof is
 * aborted, its root held against the recorded one).  r0h_session_finish then commits the segment again through
 * r0h_proof_begin_committed_top: expansion, iNTT and the expanding NTT, no row hashing and no folds.  The comparison of the replayed
 * root with the recorded one, which the hashing replay makes, is replaced by the subtree check at the 50 queries of
 * r0h_proof_finish; the seals are the same.  0 = the default: off.  Every trace-circuit segment has at least 13 path digests, so
 * every value up to 8 fits every segment.  Taken per session at r0h_session_begin; it matters only for segments that are evicted
 * (r0h_ctx_set_session_device_limit).  The tops count in r0h_ctx_session_held_bytes, on top of the limit like the rows.
 * r0h_last_session_tree_tops: of the last session finished on this context -- segments replayed from their top, the most bytes held
 * in tops, the levels in force (0 for a session without a device limit: nothing is evicted, no top is kept). */
const char* r0h_ctx_set_session_tree_tops(r0h_ctx* ctx, uint32_t levels);
const char* r0h_last_session_tree_tops(r0h_ctx* ctx, uint64_t out[3]);
const char* r0h_prove_elf(r0h_ctx* ctx, const r0h_circuit* c, const uint8_t* elf, size_t elf_len, const uint32_t* input_words,
                          size_t n_input, uint32_t segment_po2, uint64_t max_cycles, r0h_receipt** receipt_out,
                          uint8_t image_id_out[32], uint64_t* cycles_out);
/* One rank's share of a session that is proved on several GPUs: the guest is executed in full on every rank (it is deterministic and
 * costs a tenth of a second per ten million cycles -- less than moving 72 MiB of rows per segment between GPUs), segments part,
 * part + parts, ... are proved.  The receipt holds those segments only; r0h_receipt_merge puts the ranks' receipts together into the
 * receipt r0h_prove_elf would have returned (same seals: a segment's proof does not depend on who makes it).  No collective is
 * involved: the receipts travel as JSON (hyperfridge-r0_amd/driver.py: prove_elf_sharded over torch.distributed). */
const char* r0h_prove_elf_part(r0h_ctx* ctx, const r0h_circuit* c, const uint8_t* elf, size_t elf_len, const uint32_t* input_words,
                               size_t n_input, uint32_t segment_po2, uint64_t max_cycles, uint32_t part, uint32_t parts,
                               r0h_receipt** receipt_out, uint8_t image_id_out[32], uint64_t* cycles_out);
/* The two phases of a trace-circuit session, for ranks that share one (r0h_prove_elf is begin + finish on one rank): `begin` executes
 * the guest and commits the DATA group of this rank's segments (part, part + parts, ...); `records` gives what they contribute to the
 * session challenge; the ranks exchange their records (28 words per segment: an all-gather); `finish` takes the records of ALL
 * segments in index order, derives the challenge, finishes this rank's proofs and returns their receipt (r0h_receipt_merge joins
 * the ranks' receipts).  A session holds device memory (about 3 GiB per 2^20-row segment) until it is finished or freed. */
/* the challenge itself (public inputs R0H_TRACE_GAMMA .. +16 of every seal of the session): alpha_g, gamma, gamma^2, gamma^3 drawn
 * from the Poseidon2 digest of all records in index order -- what r0h_session_finish and r0h_receipt_verify[_elf] both compute */
const char* r0h_session_challenge(const uint32_t* records, size_t n_records, uint32_t challenge_out[16]);
typedef struct r0h_session r0h_session;
const char* r0h_session_begin(r0h_ctx* ctx, const r0h_circuit* c, const uint8_t* elf, size_t elf_len, const uint32_t* input_words,
                              size_t n_input, uint32_t segment_po2, uint64_t max_cycles, uint32_t part, uint32_t parts,
                              r0h_session** session_out);
size_t r0h_session_n_segments(const r0h_session* s); /* of the whole session */
const char* r0h_session_records(const r0h_session* s, uint32_t* indices_out, uint32_t* records_out, size_t capacity, size_t* n_out);
const char* r0h_session_finish(r0h_session* s, const uint32_t* all_records, size_t n_records, r0h_receipt** receipt_out,
                               uint8_t image_id_out[32], uint64_t* cycles_out);
const char* r0h_session_free(r0h_session* s);
/* The session's own share of the session balance (above): the additions r0h_ctx_set_check_session's check makes for this rank's
 * pending segments and nothing else -- `source` is the segment's index, a resident or lean DATA witness is used as it is, an evicted
 * segment's is expanded again from its rows; the verifier's side is NOT added (one rank adds it: r0h_session_balance_add_verifier_side).
 * Between r0h_session_begin and r0h_session_finish, any `parts`, a trace-circuit session and a device handle made from its circuit's
 * blob on the session's device; anything else is an error that says so.  r0h_session_journal: the run's journal, which every rank has
 * (the guest is executed in full on each); the bytes are the session's until it is freed. */
const char* r0h_session_balance_add_session(r0h_session_balance* sb, r0h_session* s);
const char* r0h_session_journal(const r0h_session* s, const uint8_t** bytes, size_t* n);
/* composite receipts that each hold some segments of one session -> one receipt with all of them in index order.  Refused: a
 * segment index missing or present twice, journals that differ, a receipt that is not composite. */
const char* r0h_receipt_merge(const r0h_receipt* const* parts, size_t n, r0h_receipt** out);
/* per-stage timing of the last r0h_prove_elf on this context (for tools/bench_session.py): names are static strings */
/* r0h_ctx_set_session_enqueue(ctx, on != 0): the trace-circuit sessions begun on this context finish (phase 2) from the thread that
 * calls r0h_session_finish / r0h_prove_elf alone -- no lane threads.  Off by default; a context that was never told follows the
 * environment (R0H_SESSION_ENQUEUE=1: on).  Taken per session at r0h_session_begin; the session's lane contexts run
 * r0h_ctx_set_device_finish for the length of the phase.  Per segment the thread uploads the public inputs, then enqueues on the
 * segment's lane context: the session sum (r0h_logup_totals_device), the late inputs and the mix (r0h_proof_late_device), the
 * accumulation (r0h_accum_public_device) and r0h_proof_finish_enqueue -- none of which waits.  Every lane context keeps the segments phase 1 dealt it as a queue of
 * its own, and the thread goes round the lanes that still have one: on each it collects the segment that lane has in flight
 * (r0h_proof_finish_collect; the oldest enqueue of all, since every other lane was served after it) and enqueues the lane's next.  A
 * lane context has at most one segment in flight, so the extra device memory is one ACCUM group and one set of finish temporaries
 * per lane, as in the blocking form, and while one lane is collected the others' streams have a segment to run.  WHAT WAITS: per segment the
 * collect's read-back and the close of the lane's profile (two waits of a stream); the blocking second commitment of an evicted
 * segment, on the calling thread right before its enqueue; the image proof, which the calling thread proves with the blocking
 * r0h_prove_image after the first round, when every lane that holds a segment has had its first enqueue (what is in flight on the session's own context is collected first);
 * r0h_ctx_set_check_witness's read-backs.  The session check runs before the phase as always; phase 1 keeps its lanes.  An error at
 * the enqueue or the collect of a segment is the session's error: what is in flight is collected, every other proof is aborted.  The
 * seals, and so the receipt, are the ones of the lanes' form.  r0h_session_stats.prove_ms counts an enqueued segment from its enqueue
 * to its collect (wall time, so segments in flight on several lanes overlap in it).
 * r0h_last_session_phase2: of the last trace-circuit session finished on this context -- the host threads phase 2 ran on (1, or the
 * session's lanes), the blocking waits the lanes' contexts made during it, how many of those were the staging ring wrapping around
 * (stage uploads wait when the 8 MiB pinned ring of a context is used up), and how many were made by replays of evicted segments and
 * the image proof. */
const char* r0h_ctx_set_session_enqueue(r0h_ctx* ctx, int on);
const char* r0h_last_session_phase2(r0h_ctx* ctx, uint64_t out[4]);
/* r0h_ctx_set_session_enqueue_begin(ctx, on != 0): a switch of its own beside the one above, off by default (a context that was never
 * told follows R0H_SESSION_ENQUEUE_BEGIN=1), taken per session at r0h_session_begin; it implies r0h_ctx_set_session_enqueue for the
 * session.  The trace-circuit session is then driven by its calling thread and its executor thread and nothing else:
 *   phase 1   no lane threads.  The thread inside r0h_prove_elf / r0h_session_begin takes each segment from the executor's queue and
 *             enqueues, on the next lane's stream, the upload of its rows, the expansion, the multiplicity kernels and
 *             r0h_proof_begin_committed_enqueue.  The DATA roots (and the multiplicity kernels' error words) are gathered device to
 *             device (r0h_proof_data_root_device) into one buffer per lane and read back once per lane at the phase's end: WHAT WAITS
 *             is that read-back, once per lane that had a segment; per evicted segment (r0h_ctx_set_session_device_limit) the
 *             read-back of its root before it gives up its proof; per lean segment r0h_proof_shrink, as ever; a lane that holds the
 *             rows of more than two segments whose copies have not run (the rows go back to the executor behind their copy); and
 *             the CODE commitment of a trace size a context has not seen.  A lookup outside its table is reported at the phase's end.
 *   phase 2   as under r0h_ctx_set_session_enqueue, and: an evicted segment is committed again through the enqueue begin (or its
 *             _top form), so a replay no longer blocks -- the root it commits comes home behind its seal and is held against the
 *             recorded one there (one read-back); the image proof is enqueued as soon as the challenge exists
 *             (r0h_prove_image_enqueue) on a helper context of its own -- a context reports one proof at a time -- and collected
 *             behind the last segment.
 * The records, r0h_session_challenge, the seals and the receipt are the default form's byte for byte.  Sharded sessions
 * (r0h_session_begin with parts > 1) refuse the switch.
 * r0h_last_session_phase1: of the last trace-circuit session begun on this context -- host threads started for phase 1 (0 under the
 * switch, lanes - 1 otherwise), the blocking waits the lanes' contexts made in it, its segments, and of them the evicted. */
const char* r0h_ctx_set_session_enqueue_begin(r0h_ctx* ctx, int on);
const char* r0h_last_session_phase1(r0h_ctx* ctx, uint64_t out[4]);
typedef struct { uint32_t segments, lean_segments /* proved without resident evaluations: r0h_ctx_set_session_resident_limit */; uint64_t cycles; double executor_s, witgen_ms, prove_ms, wall_s; } r0h_session_stats;
const char* r0h_last_session_stats(r0h_ctx* ctx, r0h_session_stats* out);

/* ---- the image proof: `receipt.verify(image_id)` without the program image (verifier/src/main.rs:124-126).  r0h_receipt_verify_elf
 * completes a trace-circuit session's memory argument with the ELF's own words; a verifier who holds only the 32 bytes of the image id
 * cannot.  The image circuit (circuits/image.r0c, tools/image_circuit.py; W = 8 ACCUM + 30 CODE + 69 DATA) proves the image's side
 * for it: its rows run the Poseidon2 sponge over the image's word list -- blocks of four (word index, low half, high half) and a mask
 * -- whose digest is the root of the initial memory state the image id names (public inputs 0..7), and add every word's fraction
 * 1 / (alpha_g - index - gamma lo - gamma^2 hi - gamma^3 TAG_IMAGE) under the session's challenge (inputs 8..23) to a running sum
 * whose total is public (inputs 24..27).  r0h_prove_elf attaches such a seal to the receipt when the context has been given the image
 * circuit (r0h_ctx_set_image_circuit); r0h_receipt_verify_image checks it and balances the session with its total. ---- */
#define R0H_IMAGE_COLUMNS 69
#define R0H_IMAGE_GLOBALS 28
#define R0H_IMAGE_LATE_GLOBALS 20
#define R0H_IMAGE_GAMMA 8
#define R0H_IMAGE_SUM 24
/* smallest trace that holds the image's sponge (30 rows per four words; at least 2^9) */
const char* r0h_image_po2(const uint8_t* elf, size_t elf_len, uint32_t* po2_out);
/* host: the image circuit's DATA group for an ELF ([R0H_IMAGE_COLUMNS][2^po2], Montgomery, column-major) and its public inputs with
 * the digest filled in (challenge and total left zero) */
const char* r0h_image_witness(const uint8_t* elf, size_t elf_len, uint32_t po2, uint32_t* data_out, uint32_t globals_out[R0H_IMAGE_GLOBALS]);
/* sessions begun on `ctx` afterwards (r0h_prove_elf, r0h_session_begin with part 0) attach an image proof to their receipts; NULL stops
 * that.  The circuit must have been loaded on this context and must outlive the sessions. */
const char* r0h_ctx_set_image_circuit(r0h_ctx* ctx, const r0h_circuit* image_circuit);
/* device: one image proof under `challenge` (r0h_session_challenge); seal_out may be NULL to ask for the size */
const char* r0h_prove_image(r0h_ctx* ctx, const r0h_circuit* image_circuit, const uint8_t* elf, size_t elf_len, const uint32_t challenge[16],
                            uint32_t* seal_out, size_t seal_capacity_words, size_t* seal_words_out);
/* The same proof in two calls (r0h_ctx_set_device_finish on), so that the thread that makes it can go on enqueueing elsewhere.
 * r0h_prove_image_enqueue plants the witness, adds up the total on the device (r0h_logup_totals_device) and submits the proof through
 * r0h_proof_begin_committed_enqueue, r0h_proof_late_device (the challenge and the total are the circuit's late inputs),
 * r0h_accum_public_device and r0h_proof_finish_enqueue; it waits for nothing, except on the first call for a (context, trace size,
 * suite): the image circuit's CODE group is committed then, once, and kept by the circuit's context like a session's CODE commitment.
 * r0h_prove_image_collect is the read-back: the seal of r0h_prove_image, word for word; it consumes the handle either way
 * (r0h_prove_image_abort: the handle given up, after its stream has drained).  A challenge word that is not canonical, a circuit that
 * is not the image circuit and a context with the switch off are refused at the enqueue.  The ELF's bytes are not read after the
 * enqueue returns.  A context reports one proof at a time: begin the next proof on `ctx` after the collect. */
typedef struct r0h_image_proof r0h_image_proof;
const char* r0h_prove_image_enqueue(r0h_ctx* ctx, const r0h_circuit* image_circuit, const uint8_t* elf, size_t elf_len, const uint32_t challenge[16],
                                    r0h_image_proof** out);
const char* r0h_prove_image_collect(r0h_image_proof* handle, uint32_t* seal_out, size_t seal_capacity_words, size_t* seal_words_out);
const char* r0h_prove_image_abort(r0h_image_proof* handle);

/* ---- recursion: risc0-zkvm `ProverServer::{lift, join, compress}` (risc0-circuit-recursion 4.0.4, Cargo.lock:3050-3085; BASELINE.json
 * configs[4]).  `lift` stands one recursion-circuit proof for one segment seal and its claim; `join` folds two nodes into one whose
 * claim is the composition {pre: a.pre, post: b.post, exit_code: b.exit_code, input: a.input, output: b.output}, and refuses two
 * nodes that do not follow one another (a must end in SystemSplit with a.post == b.pre); `compress` lifts every segment of a composite
 * receipt and joins the nodes into one root.  A node's 16 public inputs are the 8 words naming its composed claim (r0h_claim_globals)
 * and the Poseidon2 digest of what it consumed -- the segment seal's words for a lift, the two child seals' digests for a join.  That
 * digest is computed INSIDE the node's proof: the circuit's sponge component runs the permutation one round per row over witness cells
 * holding the consumed words and ties the result to public inputs 8..15, so a witness holding other words than the digest names
 * satisfies no trace.  A lift of a 2^20-row trace-circuit seal (61k words: 3.8k permutations of 30 rows) needs a recursion trace of
 * 2^17 rows or more.
 * NOT risc0's recursion circuit: that in-circuit hash is the first and only in-circuit step.  Every node is a proof over this
 * repository's recursion circuit (circuits/recursion.r0c) made with the same kernels, and the SEALS it consumes are verified BESIDE
 * that proof (host threads, while the device proves), not inside it -- a root is a checkable tree of seals carrying the end-to-end
 * claim, not a succinct receipt.
 * WHAT A ROOT CARRIES.  Its seal, its composed claim, and -- when every leaf below it is a trace-circuit segment -- its leaves' session
 * parts in leaf order, R0H_NODE_SESSION_WORDS words each, all taken from the segment seal r0h_lift verified: [0, 20) the seal's early
 * public inputs, [20, 28) the root of its DATA commitment (together the segment's R0H_SESSION_RECORD_WORDS record), [28, 44) the
 * session challenge as the seal carries it, [44, 48) the segment's sum.  A lift over any other circuit leaves the part empty; a join
 * concatenates left then right and has none unless both children have one.  A trace-circuit seal binds its memory to the program
 * image and to the journal only through the session argument -- segment numbers, closing flags and ranges, the common challenge, the
 * balance of the sums -- and neither r0h_lift nor r0h_join nor r0h_node_verify checks that argument.  r0h_root_verify_session_elf /
 * _image do: they hold a root to everything r0h_receipt_verify_elf / _image hold a receipt to beyond the seals themselves (the leaves
 * chain from the claim's first pc to its last, the way of ending and the exit code are the claim's, the journal is the one the claim
 * commits to, numbers 1..n, the closing rules, every leaf's challenge is r0h_session_challenge over all records, the sums balance with
 * the image's words -- the ELF's, or the image proof's total -- and the journal's, the claim's pre-state is the image id), with the
 * same R0H_RECEIPT_V_* verdicts (one difference in order: the image id is looked at before the session section, so another program's
 * ELF gets R0H_RECEIPT_V_IMAGE_ID where r0h_receipt_verify_elf, which reaches the balance first, says R0H_RECEIPT_V_SESSION_SUM).  Without that call a root built by honest lift / join calls over seals made under a self-chosen
 * challenge, or whose sums do not balance, passes r0h_node_verify.
 * THE LIMIT, in plain words.  The session part is not among the node's public inputs: it travels BESIDE the node, as the claim does.
 * What binds it is that r0h_lift takes it from the seal it verified.  Someone who holds only a root trusts whoever ran lift / join for
 * it -- exactly as for the validity of the children, which is also checked beside the proofs.  Someone who holds the tree can recheck
 * it: r0h_trace_seal_session_part gives a leaf's part from its seal.
 * Moving nodes between ranks (the tree's levels) is the caller's: hyperfridge-r0_amd/recursion.py does it over torch.distributed
 * point-to-point. ---- */
#define R0H_NODE_SESSION_WORDS 48
typedef struct r0h_recursor r0h_recursor;
typedef struct r0h_node r0h_node;
/* segment_control_roots: n_roots records of 9 words [po2, root[8]] (r0h_code_root of the segment circuit); with n_roots = 0 the
 * leaves are verified against the segment circuit alone */
const char* r0h_recursor_new(r0h_ctx* ctx, const uint32_t* recursion_blob, size_t recursion_words, const char* code_object_path,
                             uint32_t po2, const uint32_t* segment_blob, size_t segment_words, const uint32_t* segment_control_roots,
                             size_t n_roots, r0h_recursor** out);
const char* r0h_recursor_free(r0h_recursor* rc);
/* on != 0: r0h_lift, r0h_join and r0h_compress verify the seals they consume through r0h_verify_seals_on's batch form on the lane's
 * context, enqueued before the node's proof (r0h_compress: all leaves in one batch), instead of on host threads beside it.  Off by
 * default; refusals and their messages are the same either way, and so is every node. */
const char* r0h_recursor_set_verify_on_device(r0h_recursor* rc, int on);
const char* r0h_recursor_control_root(const r0h_recursor* rc, uint32_t root_out[8]); /* of the recursion circuit at its po2 */
const char* r0h_lift(r0h_recursor* rc, const uint32_t* seal, size_t seal_words, const r0h_receipt_claim* claim, r0h_node** out);
const char* r0h_join(r0h_recursor* rc, const r0h_node* a, const r0h_node* b, r0h_node** out);
const char* r0h_node_new(const uint32_t* seal, size_t seal_words, const r0h_receipt_claim* claim, r0h_node** out); /* as received */
const char* r0h_node_free(r0h_node* node);
const char* r0h_node_seal(const r0h_node* node, const uint32_t** seal, size_t* seal_words);
const char* r0h_node_claim(const r0h_node* node, r0h_receipt_claim* claim_out);
const char* r0h_node_verify(const uint32_t* recursion_blob, size_t blob_words, const uint32_t* control_root, const r0h_node* node,
                            int* ok_out);
/* the leaves' session parts: *words points at n_leaves * R0H_NODE_SESSION_WORDS words owned by the node (n_leaves = 0: none) */
const char* r0h_node_session(const r0h_node* node, const uint32_t** words, size_t* n_leaves);
/* r0h_node_new for a node that arrives with its session parts */
const char* r0h_node_new_with_session(const uint32_t* seal, size_t seal_words, const r0h_receipt_claim* claim, const uint32_t* session,
                                      size_t n_leaves, r0h_node** out);
/* host only: the session part of one trace-circuit seal -- the extraction r0h_lift makes.  The seal is verified against the circuit
 * (it yields the DATA root); one that does not verify is an error. */
const char* r0h_trace_seal_session_part(const uint32_t* blob, size_t blob_words, const uint32_t* seal, size_t seal_words,
                                        uint32_t part_out[R0H_NODE_SESSION_WORDS]);
/* `prover.compress(opts, &receipt)`: every segment of a composite receipt lifted and the nodes joined into one root, neighbours per
 * level, an odd last node carried up -- the root r0h_lift / r0h_join give one after another, word for word.  lanes = 1..4 prover lanes
 * (0: 2): lane 0 is the recursor's context on the calling thread, the others helper contexts of the same device on threads of their
 * own; a lift is ready at once, a join when both its children are done.  Refused: what r0h_lift refuses, and, for a trace-circuit
 * receipt, before any proof is made, one that fails the session checks that need no image (numbers, closing rules, the common
 * challenge: R0H_RECEIPT_V_SESSION's reason and the segment are named).  The balance stays r0h_root_verify_session_*'s. */
const char* r0h_compress(r0h_recursor* rc, const r0h_receipt* receipt, uint32_t lanes, r0h_node** out);
/* A root held to its session (host only; see above).  blob: the trace circuit.  Returns an error string for a node that cannot be
 * read as a session at all -- no session part, 2^20 leaves or more, a word that is no field element -- and otherwise NULL with
 * *verdict_out an R0H_RECEIPT_V_* code and *leaf_out (optional) the leaf it is about.  The node's seal is not read: r0h_node_verify
 * does that. */
const char* r0h_root_verify_session_elf(const uint32_t* blob, size_t blob_words, const r0h_node* node, const uint8_t* journal,
                                        size_t journal_len, const uint8_t* elf, size_t elf_len, int* verdict_out, size_t* leaf_out);
/* ... the program image not in hand: the image proof (a receipt's `image_proof`) stands for it, checked as r0h_receipt_verify_image
 * checks it (image_control_root NULL: derived from the image blob) */
const char* r0h_root_verify_session_image(const uint32_t* blob, size_t blob_words, const r0h_node* node, const uint8_t* journal,
                                          size_t journal_len, const uint32_t* image_blob, size_t image_blob_words,
                                          const uint32_t* image_control_root, const uint32_t* image_seal, size_t image_seal_words,
                                          const uint8_t* image_id, int* verdict_out, size_t* leaf_out);

/* Optional per-kernel timing with HIP events on the context's stream (for bench.py's roofline object): enable, run,
 * then read {"kernel family": {"launches", "total_ms", "alg_bytes"}} as JSON.  Enabling resets the counters. */
const char* r0h_kernel_timing(r0h_ctx* ctx, int enable);
const char* r0h_kernel_stats(r0h_ctx* ctx, char* json_out, size_t capacity);

#ifdef __cplusplus
}
#endif
#endif
