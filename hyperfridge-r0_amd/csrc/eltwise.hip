// Streaming operations of the prover for gfx950: polynomial evaluation at extension points, FRI batching mix,
// FRI fold and the small element-wise helpers (the extension-field scans are scan.hip).
// Replaces risc0-zkp 3.0.4 hal `batch_evaluate_any`, `mix_poly_coeffs`, `eltwise_{add,copy}_elem`,
// `eltwise_sum_extelem`, `gather_sample`, `scatter`, `fri_fold` -- SURVEY.md 8(a) a12-a15.
// All of these are HBM-bound streams: one pass over the operand, coalesced column reads, 16-byte extension accesses.
#include <algorithm>
#include <array>
#include <map>

#include "internal.hpp"

namespace r0h {

__device__ __forceinline__ Fp4 ld4(const uint32_t* p) {
  uint4 v = *(const uint4*)p;
  return Fp4{{v.x, v.y, v.z, v.w}};
}
__device__ __forceinline__ void st4(uint32_t* p, const Fp4& v) { *(uint4*)p = make_uint4(v.e[0], v.e[1], v.e[2], v.e[3]); }

// ------------------------------------------------------------------ batch_evaluate_any
// sum_i c[i] x^i = sum_hi B[hi] * (sum_lo c[hi*RL + lo] * A[lo]),  A[lo] = x^lo, B[hi] = x^(hi*RL).
// A wave owns a row of RL coefficients: each lane keeps its 16 A-values in registers, multiplies base-field
// coefficients into them (4 products per coefficient), the wave reduces, lane 0 folds in B[hi].
constexpr uint32_t EVAL_BLOCKS = 64;  // partial sums per evaluation

// A[lo] and B[hi] with A[lo] * B[hi] = x^e(hi*rl + lo): e = identity for natural-order coefficients, e = brev_n for
// bit-reversed ones (brev_n(hi*rl + lo) = brev(lo) * rows + brev(hi))
__global__ void eval_tables_kernel(uint32_t* __restrict__ tabs, const uint32_t* __restrict__ points, uint32_t rl_log, uint32_t rows_log, uint32_t bitrev_coeffs) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, rl = 1u << rl_log, rows = 1u << rows_log;
  uint32_t* tab = tabs + 4 * (size_t)blockIdx.y * (rl + rows);  // one table pair per point
  const Fp4 x = ld4(points + 4 * (size_t)blockIdx.y);
  if (i < rl) st4(tab + 4 * (size_t)i, fp4_pow(x, bitrev_coeffs ? (uint64_t)bitrev(i, rl_log) << rows_log : (uint64_t)i));
  else if (i < rl + rows) st4(tab + 4 * (size_t)i, fp4_pow(x, bitrev_coeffs ? (uint64_t)bitrev(i - rl, rows_log) : (uint64_t)(i - rl) << rl_log));
}

// A column is read ONCE and evaluated at all NP points asked of it (a register's taps sit at 1-3 points z w^-back).
// sum_i c[i] x^i = sum_lo A[lo] * (sum_hi c[hi*RL + lo] * B[hi]): a lane owns KP fixed positions lo of every row and keeps, per
// point, one 64-bit running sum per (position, extension component).  A row costs one v_mad_u64_u32 per coefficient and component
// against the wave-uniform B[hi] (scalar loads) and a correction of the high words every second row -- no cross-lane step and no
// extension product inside the loop; the A[lo] products and the wave reduction happen once per wave at the end.  (Round 1, and the
// first form of this kernel, multiplied by A[lo] first and reduced every row across the wave: 1,150 instead of ~400 SIMD cycles per
// row and point.)
template <int NP>
__global__ __launch_bounds__(256) void eval_rows_kernel(uint32_t* __restrict__ partial, const uint32_t* __restrict__ coeffs,
                                                         const uint32_t* __restrict__ which, const uint32_t* __restrict__ tabs,
                                                         uint32_t po2, uint32_t rl_log) {
  constexpr int KP = 8;  // positions per lane: rows of up to 512 coefficients
  const uint32_t rl = 1u << rl_log, rows = 1u << (po2 - rl_log);
  const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t* poly = coeffs + ((size_t)which[blockIdx.y] << po2);
  const size_t tab_stride = 4 * (size_t)(rl + rows);
  uint64_t acc[NP][KP][4];
#pragma unroll
  for (int p = 0; p < NP; p++)
#pragma unroll
    for (int k = 0; k < KP; k++)
#pragma unroll
      for (int q = 0; q < 4; q++) acc[p][k][q] = 0;
  uint32_t n_rows = 0;
#pragma unroll 1
  for (uint32_t hi = blockIdx.x * 4 + wave; hi < rows; hi += gridDim.x * 4) {
    const uint32_t* row = poly + ((size_t)hi << rl_log);
    uint32_t cf[KP];
#pragma unroll
    for (int k = 0; k < KP; k++) {
      uint32_t lo = lane + 64 * k;
      cf[k] = lo < rl ? row[lo] : 0u;
    }
    // four terms fit a 64-bit sum as they are; from then on the high words are brought below p before every second term
    const bool fix = n_rows >= 4 && (n_rows & 1) == 0;
#pragma unroll
    for (int p = 0; p < NP; p++) {
      const uint32_t* bp = tabs + p * tab_stride + 4 * (size_t)(rl + hi);  // wave-uniform address
      const uint32_t b0 = bp[0], b1 = bp[1], b2 = bp[2], b3 = bp[3];
#pragma unroll
      for (int k = 0; k < KP; k++) {
        if (fix) {
#pragma unroll
          for (int q = 0; q < 4; q++) acc[p][k][q] = ((uint64_t)reduce1((uint32_t)(acc[p][k][q] >> 32)) << 32) | (uint32_t)acc[p][k][q];
        }
        acc[p][k][0] += (uint64_t)cf[k] * b0; acc[p][k][1] += (uint64_t)cf[k] * b1;
        acc[p][k][2] += (uint64_t)cf[k] * b2; acc[p][k][3] += (uint64_t)cf[k] * b3;
      }
    }
    n_rows++;
  }
  __shared__ uint32_t red[4][NP][4];
#pragma unroll
  for (int p = 0; p < NP; p++) {
    Fp4 tot = fp4_zero();
#pragma unroll
    for (int k = 0; k < KP; k++) {
      const uint32_t lo = lane + 64 * k;
      Fp4 v;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        uint64_t t = ((uint64_t)reduce1((uint32_t)(acc[p][k][q] >> 32)) << 32) | (uint32_t)acc[p][k][q];  // high word below 2p by the invariant
        v.e[q] = reduce64(t);
      }
      if (lo < rl) tot = tot + v * ld4(tabs + p * tab_stride + 4 * (size_t)lo);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      Fp4 o;
#pragma unroll
      for (int q = 0; q < 4; q++) o.e[q] = __shfl_xor(tot.e[q], off);
      tot = tot + o;
    }
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < 4; q++) red[wave][p][q] = tot.e[q];
    }
  }
  __syncthreads();
  if (threadIdx.x < NP) {
    const uint32_t p = threadIdx.x;
    Fp4 r = fp4_zero();
    for (int w = 0; w < 4; w++) r = r + Fp4{{red[w][p][0], red[w][p][1], red[w][p][2], red[w][p][3]}};
    st4(partial + 4 * (((size_t)blockIdx.y * NP + p) * gridDim.x + blockIdx.x), r);
  }
}

__global__ void eval_reduce_kernel(uint32_t* __restrict__ out, const uint32_t* __restrict__ partial,
                                   const uint32_t* __restrict__ dest, uint32_t n_partial, uint32_t n) {
  uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  Fp4 r = fp4_zero();
  for (uint32_t b = 0; b < n_partial; b++) r = r + ld4(partial + 4 * ((size_t)k * n_partial + b));
  st4(out + 4 * (size_t)dest[k], r);
}

// ------------------------------------------------------------------ mix_poly_coeffs
// combos[combo][i] += sum_{c in combo} mixpow[c] * input[c][i]; columns arrive sorted by combo.
__global__ __launch_bounds__(256) void mix_poly_kernel(uint32_t* __restrict__ combos, const uint32_t* __restrict__ input,
                                                        const uint32_t* __restrict__ params, uint32_t n_groups, uint32_t po2) {
  // params: [n_groups+1 group starts][per sorted column: col index][per group: combo id][per sorted column: 4 words mixpow]
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const uint32_t* start = params;
  const uint32_t total = start[n_groups];
  const uint32_t* cols = params + n_groups + 1;
  const uint32_t* combo_id = cols + total;
  const uint32_t* pw = combo_id + n_groups;
  for (uint32_t g = 0; g < n_groups; g++) {
    Fp4 acc = fp4_zero();
    for (uint32_t k = start[g]; k < start[g + 1]; k++) {
      Fp4 m = Fp4{{pw[4 * k], pw[4 * k + 1], pw[4 * k + 2], pw[4 * k + 3]}};
      acc = acc + scale(m, input[((size_t)cols[k] << po2) + i]);
    }
    uint32_t* dst = combos + 4 * (((size_t)combo_id[g] << po2) + i);
    st4(dst, ld4(dst) + acc);
  }
}

// out[k] = base^(exps ? exps[k] : k) for a base in device memory (a challenge the device's transcript drew): a lane per power by
// square-and-multiply, at most 32 squarings deep.  Fills the power tables the host otherwise computes and uploads -- eval_check's
// poly_mix powers, mix_poly_kernel's per-column powers, the DEEP head's.  (`out`, `base` need no alignment beyond a word.)
__global__ __launch_bounds__(256) void ext_powers_kernel(uint32_t* __restrict__ out, const uint32_t* __restrict__ base, const uint32_t* __restrict__ exps, uint32_t n) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const Fp4 r = fp4_pow(Fp4{{base[0], base[1], base[2], base[3]}}, exps ? exps[k] : k);
#pragma unroll
  for (int q = 0; q < 4; q++) out[4 * (size_t)k + q] = r.e[q];
}

// ------------------------------------------------------------------ small element-wise kernels
__global__ void add_elem_kernel(uint32_t* out, const uint32_t* a, const uint32_t* b, uint32_t n) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = add(a[i], b[i]);
}
__global__ void copy_elem_kernel(uint32_t* out, const uint32_t* in, uint32_t n) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = in[i];
}
// risc0 marks untouched witness cells with Elem::INVALID (0xffffffff); the prover zeroes them before committing
__global__ void zeroize_elem_kernel(uint32_t* io, uint32_t n) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && io[i] == 0xffffffffu) io[i] = 0u;
}
__global__ void sum_extelem_kernel(uint32_t* __restrict__ out, const uint32_t* __restrict__ in, uint32_t count, uint32_t n) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fp4 tot = fp4_zero();
  for (uint32_t c = 0; c < count; c++) tot = tot + ld4(in + 4 * ((size_t)c * n + i));
#pragma unroll
  for (int k = 0; k < 4; k++) out[(size_t)k * n + i] = tot.e[k];
}
__global__ void gather_sample_kernel(uint32_t* dst, const uint32_t* src, uint32_t idx, uint32_t size, uint32_t stride) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < size) dst[i] = src[(size_t)i * stride + idx];
}
__global__ void scatter_kernel(uint32_t* into, const uint32_t* offsets, const uint32_t* values, uint32_t begin, uint32_t end) {
  uint32_t k = begin + blockIdx.x * blockDim.x + threadIdx.x;
  if (k < end) into[offsets[k]] = values[k];
}

// ------------------------------------------------------------------ fri_fold
__device__ __forceinline__ void fri_fold_at(uint32_t* __restrict__ out, const uint32_t* __restrict__ in, const Fp4& mix, uint32_t n_out, uint32_t idx) {
  const size_t n_in = (size_t)n_out * R0H_FRI_FOLD;
  Fp4 tot = fp4_zero(), cur = fp4_one();
#pragma unroll
  for (uint32_t j = 0; j < R0H_FRI_FOLD; j++) {
    size_t src = (size_t)(__brev(j) >> 28) * n_out + idx;
    Fp4 v = Fp4{{in[src], in[n_in + src], in[2 * n_in + src], in[3 * n_in + src]}};
    tot = tot + cur * v;
    cur = cur * mix;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) out[(size_t)k * n_out + idx] = tot.e[k];
}
__global__ void fri_fold_kernel(uint32_t* __restrict__ out, const uint32_t* __restrict__ in, Fp4 mix, uint32_t n_out) {
  uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_out) return;
  fri_fold_at(out, in, mix, n_out, idx);
}
// the same with the mix read from device memory (four words a transcript on the device drew: r0h_iop_draw_ext)
__global__ void fri_fold_buf_kernel(uint32_t* __restrict__ out, const uint32_t* __restrict__ in, const uint32_t* __restrict__ mix, uint32_t n_out) {
  uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_out) return;
  fri_fold_at(out, in, Fp4{{mix[0], mix[1], mix[2], mix[3]}}, n_out, idx);
}

static Fp4 host_fp4(const uint32_t v[4]) { return Fp4{{v[0], v[1], v[2], v[3]}}; }
static bool canonical4(const uint32_t v[4]) { return v[0] < P && v[1] < P && v[2] < P && v[3] < P; }

}  // namespace r0h

using namespace r0h;

extern "C" {

const char* r0h_batch_evaluate_any(r0h_ctx* ctx, const r0h_buf* coeffs, uint32_t po2, const uint32_t* which,
                                   const uint32_t* xs, uint32_t n_eval, r0h_buf* out) {
  return r0h::evaluate_any(ctx, coeffs, po2, which, xs, n_eval, out, false);
}

}  // extern "C"

namespace r0h {
const char* ext_powers(r0h_ctx* ctx, uint32_t* d_out, const uint32_t* d_base, const uint32_t* d_exps, uint32_t n) {
  if (!n) return nullptr;
  KScope ks(ctx, "ext_powers_kernel", 16.0 * n);
  hipLaunchKernelGGL(ext_powers_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, d_out, d_base, d_exps, n);
  return launch_ok("ext_powers_kernel");
}

// Request k evaluates column which[k] at a point given by its four words xs[4k ..) (host words: evaluate_any), or, xs == nullptr, by
// its index pt_idx[k] in the device table d_points (evaluate_any_points).  Requests of one column are grouped by their list of points;
// the list's key is the words in one form and the indices in the other, so distinct points with distinct indices group alike.
static const char* evaluate_any_impl(r0h_ctx* ctx, const r0h_buf* coeffs, uint32_t po2, const uint32_t* which, const uint32_t* xs, const uint32_t* pt_idx,
                                     const uint32_t* d_points, uint32_t n_points, uint32_t n_eval, r0h_buf* out, bool bitrev_coeffs) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && coeffs && out && (n_eval == 0 || (which && (xs || (pt_idx && d_points)))), "r0h_batch_evaluate_any: NULL argument");
  R0H_REQUIRE(po2 <= MAX_DOMAIN_PO2, "r0h_batch_evaluate_any: po2 %u too large", po2);
  R0H_REQUIRE((size_t)n_eval * 16 <= out->bytes, "r0h_batch_evaluate_any: %u results exceed the output buffer", n_eval);
  if (!n_eval) return nullptr;
  const size_t n_polys = coeffs->bytes >> (po2 + 2);
  // evaluations of one column share a single read of it: group the requests by column, then the columns by the list of points
  // asked of them (in the prover: one list per tap combo), at most MAX_NP points per pass
  constexpr uint32_t MAX_NP = 2;  // 64 VGPRs of running sums per point: a third point takes a second pass over its column
  struct ColJob { uint32_t col; std::vector<uint32_t> dest; };
  std::map<uint32_t, std::vector<uint32_t>> by_col;  // column -> request indices
  for (uint32_t k = 0; k < n_eval; k++) {
    R0H_REQUIRE(which[k] < n_polys, "r0h_batch_evaluate_any: which[%u] = %u but the buffer holds %zu polynomials", k, which[k], n_polys);
    for (int q = 0; q < 4 && xs; q++) R0H_REQUIRE(xs[4 * k + q] < P, "r0h_batch_evaluate_any: xs[%u] not canonical", k);
    R0H_REQUIRE(xs || pt_idx[k] < n_points, "r0h_batch_evaluate_any: request %u names point %u of a table of %u", k, xs ? 0u : pt_idx[k], n_points);
    by_col[which[k]].push_back(k);
  }
  const size_t key_words = xs ? 4 : 1;
  std::map<std::vector<uint32_t>, std::vector<ColJob>> groups;  // point list (4 words per point, or its index in the table) -> columns
  for (auto& c : by_col)
    for (size_t at = 0; at < c.second.size(); at += MAX_NP) {
      std::vector<uint32_t> key;
      ColJob job{c.first, {}};
      for (size_t i = at; i < c.second.size() && i < at + MAX_NP; i++) {
        if (xs) key.insert(key.end(), xs + 4 * (size_t)c.second[i], xs + 4 * (size_t)c.second[i] + 4);
        else key.push_back(pt_idx[c.second[i]]);
        job.dest.push_back(c.second[i]);
      }
      groups[key].push_back(std::move(job));
    }
  const uint32_t rl_log = po2 < 9 ? po2 : 9, rl = 1u << rl_log, rows = 1u << (po2 - rl_log);
  uint32_t blocks = (rows + 3) / 4;
  if (blocks > EVAL_BLOCKS) blocks = EVAL_BLOCKS;
  size_t max_cols = 0;
  for (auto& g : groups) max_cols = std::max(max_cols, g.second.size());
  const size_t tab_words = 4 * (size_t)MAX_NP * (rl + rows), pt_words = 4 * MAX_NP, idx_words = (size_t)(1 + MAX_NP) * max_cols,
               part_words = 4 * (size_t)MAX_NP * max_cols * blocks;
  DevBuf tmp;  // [tables][points][indices][partial sums], sized for the largest group
  R0H_TRY(tmp.alloc(ctx, (tab_words + pt_words + idx_words + part_words) * 4));
  uint32_t* tab = u32(tmp.get());
  uint32_t* pts = tab + tab_words;
  uint32_t* idx = pts + pt_words;
  uint32_t* part = idx + idx_words;
  for (auto& g : groups) {
    const uint32_t np = (uint32_t)(g.first.size() / key_words), ng = (uint32_t)g.second.size();
    std::vector<uint32_t> host((size_t)(1 + np) * ng);  // [column per job][destination per (job, point)]
    for (uint32_t j = 0; j < ng; j++) {
      host[j] = g.second[j].col;
      for (uint32_t p = 0; p < np; p++) host[ng + (size_t)j * np + p] = g.second[j].dest[p];
    }
    R0H_TRY(stage_h2d(ctx, idx, host.data(), host.size() * 4));
    if (xs) R0H_TRY(stage_h2d(ctx, pts, g.first.data(), g.first.size() * 4));
    for (uint32_t p = 0; p < np && !xs; p++) R0H_TRY_HIP(hipMemcpyAsync(pts + 4 * p, d_points + 4 * (size_t)g.first[p], 16, hipMemcpyDeviceToDevice, ctx->stream));
    KScope ks(ctx, "batch_evaluate_any", 4.0 * ng * (double)(1u << po2));  // algorithmic bytes: every column once
    // blocks per polynomial: enough workgroups overall (~2048) to fill the chip, but no more -- every block re-loads the power tables
    uint32_t gb = 2048 / ng;
    gb = gb < 4 ? 4 : gb;
    gb = gb > blocks ? blocks : gb;
    hipLaunchKernelGGL(eval_tables_kernel, dim3((rl + rows + 255) / 256, np), dim3(256), 0, ctx->stream, tab, pts, rl_log, po2 - rl_log, bitrev_coeffs ? 1u : 0u);
    if (np == 1) hipLaunchKernelGGL(eval_rows_kernel<1>, dim3(gb, ng), dim3(256), 0, ctx->stream, part, u32(coeffs), idx, tab, po2, rl_log);
    else hipLaunchKernelGGL(eval_rows_kernel<2>, dim3(gb, ng), dim3(256), 0, ctx->stream, part, u32(coeffs), idx, tab, po2, rl_log);
    hipLaunchKernelGGL(eval_reduce_kernel, dim3((ng * np + 63) / 64), dim3(64), 0, ctx->stream, u32(out), part, idx + ng, gb, ng * np);
    R0H_TRY(launch_ok("batch_evaluate_any kernels"));  // reuse of the block by the next group is ordered by the stream
  }
  return nullptr;
  R0H_GUARD_END
}
const char* evaluate_any(r0h_ctx* ctx, const r0h_buf* coeffs, uint32_t po2, const uint32_t* which, const uint32_t* xs, uint32_t n_eval, r0h_buf* out, bool bitrev_coeffs) {
  R0H_REQUIRE(n_eval == 0 || xs, "r0h_batch_evaluate_any: NULL argument");
  return evaluate_any_impl(ctx, coeffs, po2, which, xs, nullptr, nullptr, 0, n_eval, out, bitrev_coeffs);
}
const char* evaluate_any_points(r0h_ctx* ctx, const r0h_buf* coeffs, uint32_t po2, const uint32_t* which, const uint32_t* pt_idx, uint32_t n_eval, const uint32_t* d_points,
                                uint32_t n_points, r0h_buf* out, bool bitrev_coeffs) {
  R0H_REQUIRE(n_eval == 0 || (pt_idx && d_points), "r0h_batch_evaluate_any: NULL argument");
  return evaluate_any_impl(ctx, coeffs, po2, which, nullptr, pt_idx, d_points, n_points, n_eval, out, bitrev_coeffs);
}

// The per-column powers are mix_start * mix^c from host words (r0h_mix_poly_coeffs), or, mix == nullptr, mix^(first_exp + c) of the four
// device words d_mix, filled into the parameter block by ext_powers (mix_poly_coeffs_dev)
static const char* mix_poly_coeffs_impl(r0h_ctx* ctx, r0h_buf* combos, const uint32_t* mix_start, const uint32_t* mix, uint32_t first_exp, const uint32_t* d_mix,
                                        const r0h_buf* input, const uint32_t* combo_of, uint32_t input_count, uint32_t po2) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && combos && input && ((mix_start && mix) || d_mix) && (combo_of || !input_count), "r0h_mix_poly_coeffs: NULL argument");
  R0H_REQUIRE(po2 <= MAX_DOMAIN_PO2, "r0h_mix_poly_coeffs: po2 %u too large", po2);
  R0H_REQUIRE(!mix || (canonical4(mix_start) && canonical4(mix)), "r0h_mix_poly_coeffs: mix words must be canonical (< p)");
  R0H_REQUIRE(((size_t)input_count << po2) * 4 <= input->bytes, "r0h_mix_poly_coeffs: %u columns exceed the input buffer", input_count);
  if (!input_count) return nullptr;
  std::vector<uint32_t> order(input_count);
  for (uint32_t c = 0; c < input_count; c++) {
    R0H_REQUIRE((((size_t)combo_of[c] + 1) << po2) * 16 <= combos->bytes, "r0h_mix_poly_coeffs: combo %u outside the combos buffer", combo_of[c]);
    order[c] = c;
  }
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return combo_of[a] < combo_of[b]; });
  std::vector<Fp4> pw(input_count);
  if (mix) {
    Fp4 cur = host_fp4(mix_start), m = host_fp4(mix);
    for (uint32_t c = 0; c < input_count; c++) { pw[c] = cur; cur = cur * m; }
  }
  std::vector<uint32_t> starts, ids;
  for (uint32_t k = 0; k < input_count; k++)
    if (k == 0 || combo_of[order[k]] != combo_of[order[k - 1]]) { starts.push_back(k); ids.push_back(combo_of[order[k]]); }
  const uint32_t n_groups = (uint32_t)ids.size();
  starts.push_back(input_count);
  std::vector<uint32_t> params;
  params.insert(params.end(), starts.begin(), starts.end());
  params.insert(params.end(), order.begin(), order.end());
  params.insert(params.end(), ids.begin(), ids.end());
  for (uint32_t k = 0; k < input_count; k++)
    for (int q = 0; q < 4; q++) params.push_back(mix ? pw[order[k]].e[q] : 0u);
  const size_t pw_at = params.size() - 4 * (size_t)input_count, exps_at = params.size();
  for (uint32_t k = 0; k < input_count && !mix; k++) params.push_back(first_exp + order[k]);  // behind everything the kernel reads: the exponent of each sorted column
  DevBuf d_params;
  R0H_TRY(d_params.alloc(ctx, params.size() * 4));
  R0H_TRY(stage_h2d(ctx, d_params->ptr, params.data(), params.size() * 4));
  if (!mix) R0H_TRY(ext_powers(ctx, u32(d_params.get()) + pw_at, d_mix, u32(d_params.get()) + exps_at, input_count));
  uint32_t n = 1u << po2, threads = n < 256 ? n : 256;
  KScope ks(ctx, "mix_poly_kernel", 4.0 * input_count * (double)n + 32.0 * n_groups * (double)n);
  hipLaunchKernelGGL(mix_poly_kernel, dim3(n / threads), dim3(threads), 0, ctx->stream, u32(combos), u32(input), u32(d_params.get()), n_groups, po2);
  return launch_ok("mix_poly_kernel");
  R0H_GUARD_END
}
const char* mix_poly_coeffs_dev(r0h_ctx* ctx, r0h_buf* combos, uint32_t first_exp, const uint32_t* d_mix, const r0h_buf* input, const uint32_t* combo_of, uint32_t input_count,
                                uint32_t po2) {
  R0H_REQUIRE(d_mix, "r0h_mix_poly_coeffs: NULL argument");
  return mix_poly_coeffs_impl(ctx, combos, nullptr, nullptr, first_exp, d_mix, input, combo_of, input_count, po2);
}
}  // namespace r0h

extern "C" {

const char* r0h_mix_poly_coeffs(r0h_ctx* ctx, r0h_buf* combos, const uint32_t mix_start[4], const uint32_t mix[4],
                                const r0h_buf* input, const uint32_t* combo_of, uint32_t input_count, uint32_t po2) {
  R0H_REQUIRE(mix_start && mix, "r0h_mix_poly_coeffs: NULL argument");
  return mix_poly_coeffs_impl(ctx, combos, mix_start, mix, 0, nullptr, input, combo_of, input_count, po2);
}

const char* r0h_eltwise_add_elem(r0h_ctx* ctx, r0h_buf* out, const r0h_buf* a, const r0h_buf* b, uint32_t n) {
  R0H_REQUIRE(ctx && out && a && b, "r0h_eltwise_add_elem: NULL argument");
  R0H_REQUIRE((size_t)n * 4 <= out->bytes && (size_t)n * 4 <= a->bytes && (size_t)n * 4 <= b->bytes, "r0h_eltwise_add_elem: n %u exceeds a buffer", n);
  if (!n) return nullptr;
  hipLaunchKernelGGL(add_elem_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, u32(out), u32(a), u32(b), n);
  return launch_ok("add_elem_kernel");
}
const char* r0h_eltwise_copy_elem(r0h_ctx* ctx, r0h_buf* out, const r0h_buf* in, uint32_t n) {
  R0H_REQUIRE(ctx && out && in, "r0h_eltwise_copy_elem: NULL argument");
  R0H_REQUIRE((size_t)n * 4 <= out->bytes && (size_t)n * 4 <= in->bytes, "r0h_eltwise_copy_elem: n %u exceeds a buffer", n);
  if (!n) return nullptr;
  hipLaunchKernelGGL(copy_elem_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, u32(out), u32(in), n);
  return launch_ok("copy_elem_kernel");
}
const char* r0h_eltwise_zeroize_elem(r0h_ctx* ctx, r0h_buf* io, uint32_t n) {
  R0H_REQUIRE(ctx && io, "r0h_eltwise_zeroize_elem: NULL argument");
  R0H_REQUIRE((size_t)n * 4 <= io->bytes, "r0h_eltwise_zeroize_elem: n %u exceeds the buffer", n);
  if (!n) return nullptr;
  hipLaunchKernelGGL(zeroize_elem_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, u32(io), n);
  return launch_ok("zeroize_elem_kernel");
}
const char* r0h_eltwise_sum_extelem(r0h_ctx* ctx, r0h_buf* out, const r0h_buf* in, uint32_t count, uint32_t n) {
  R0H_REQUIRE(ctx && out && in, "r0h_eltwise_sum_extelem: NULL argument");
  R0H_REQUIRE((size_t)n * 16 <= out->bytes && (size_t)n * count * 16 <= in->bytes, "r0h_eltwise_sum_extelem: sizes exceed a buffer");
  if (!n) return nullptr;
  hipLaunchKernelGGL(sum_extelem_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, u32(out), u32(in), count, n);
  return launch_ok("sum_extelem_kernel");
}
const char* r0h_gather_sample(r0h_ctx* ctx, r0h_buf* dst, const r0h_buf* src, uint32_t idx, uint32_t size, uint32_t stride) {
  R0H_REQUIRE(ctx && dst && src, "r0h_gather_sample: NULL argument");
  R0H_REQUIRE((size_t)size * 4 <= dst->bytes, "r0h_gather_sample: size %u exceeds dst", size);
  R0H_REQUIRE(size == 0 || ((size_t)(size - 1) * stride + idx + 1) * 4 <= src->bytes, "r0h_gather_sample: reads past src");
  if (!size) return nullptr;
  hipLaunchKernelGGL(gather_sample_kernel, dim3((size + 255) / 256), dim3(256), 0, ctx->stream, u32(dst), u32(src), idx, size, stride);
  return launch_ok("gather_sample_kernel");
}
const char* r0h_scatter(r0h_ctx* ctx, r0h_buf* into, const r0h_buf* index, const r0h_buf* offsets, const r0h_buf* values, uint32_t n_index) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && into && index && offsets && values, "r0h_scatter: NULL argument");
  if (n_index < 2) return nullptr;
  R0H_REQUIRE((size_t)n_index * 4 <= index->bytes, "r0h_scatter: n_index exceeds the index buffer");
  std::vector<uint32_t> idx(n_index);
  R0H_TRY(r0h_buf_d2h(ctx, index, 0, idx.data(), (size_t)n_index * 4));
  uint32_t begin = idx[0], end = idx[n_index - 1];
  R0H_REQUIRE(begin <= end && (size_t)end * 4 <= offsets->bytes && (size_t)end * 4 <= values->bytes, "r0h_scatter: index range [%u, %u) outside offsets/values", begin, end);
  std::vector<uint32_t> offs(end - begin);
  if (end > begin) {
    R0H_TRY(r0h_buf_d2h(ctx, offsets, (size_t)begin * 4, offs.data(), (size_t)(end - begin) * 4));
    for (uint32_t o : offs) R0H_REQUIRE((size_t)o * 4 < into->bytes, "r0h_scatter: offset %u outside the destination", o);
    hipLaunchKernelGGL(scatter_kernel, dim3((end - begin + 255) / 256), dim3(256), 0, ctx->stream, u32(into), u32(offsets), u32(values), begin, end);
  }
  return launch_ok("scatter_kernel");
  R0H_GUARD_END
}

// ---- the same operations with the operand placement of the risc0-zkp `Hal` trait (as recalled): `which`, `xs` and
// `combos` are device Buffers there, `scatter` takes host slices.  The grouping these kernels rely on is made on the host, so the
// Buffer forms read the small index buffers back (one copy of a few KB) -- a Rust `HipHal` calls these and never copies itself.
const char* r0h_batch_evaluate_any_buf(r0h_ctx* ctx, const r0h_buf* coeffs, uint32_t po2, const r0h_buf* which, const r0h_buf* xs, uint32_t n_eval, r0h_buf* out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && coeffs && out && which && xs, "r0h_batch_evaluate_any_buf: NULL argument");
  R0H_REQUIRE((size_t)n_eval * 4 <= which->bytes && (size_t)n_eval * 16 <= xs->bytes, "r0h_batch_evaluate_any_buf: %u evaluations exceed the which / xs buffers", n_eval);
  std::vector<uint32_t> w(n_eval), x(4 * (size_t)n_eval);
  if (n_eval) {
    R0H_TRY(r0h_buf_d2h(ctx, which, 0, w.data(), w.size() * 4));
    R0H_TRY(r0h_buf_d2h(ctx, xs, 0, x.data(), x.size() * 4));
  }
  return r0h::evaluate_any(ctx, coeffs, po2, w.data(), x.data(), n_eval, out, false);
  R0H_GUARD_END
}

const char* r0h_mix_poly_coeffs_buf(r0h_ctx* ctx, r0h_buf* combos, const uint32_t mix_start[4], const uint32_t mix[4], const r0h_buf* input, const r0h_buf* combo_of,
                                    uint32_t input_count, uint32_t po2) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && combo_of, "r0h_mix_poly_coeffs_buf: NULL argument");
  R0H_REQUIRE((size_t)input_count * 4 <= combo_of->bytes, "r0h_mix_poly_coeffs_buf: %u columns exceed the combo buffer", input_count);
  std::vector<uint32_t> c(input_count);
  if (input_count) R0H_TRY(r0h_buf_d2h(ctx, combo_of, 0, c.data(), c.size() * 4));
  return r0h_mix_poly_coeffs(ctx, combos, mix_start, mix, input, c.data(), input_count, po2);
  R0H_GUARD_END
}

// Hal::scatter(into, index: &[u32], offsets: &[u32], values: &[Elem]): values[k] goes to into[offsets[k]] for index[0] <= k < index[n_index - 1]
const char* r0h_scatter_slices(r0h_ctx* ctx, r0h_buf* into, const uint32_t* index, uint32_t n_index, const uint32_t* offsets, const uint32_t* values, uint32_t n_values) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && into && (index || !n_index) && ((offsets && values) || !n_values), "r0h_scatter_slices: NULL argument");
  if (n_index < 2) return nullptr;
  const uint32_t begin = index[0], end = index[n_index - 1];
  R0H_REQUIRE(begin <= end && end <= n_values, "r0h_scatter_slices: index range [%u, %u) outside %u offsets/values", begin, end, n_values);
  if (end == begin) return nullptr;
  for (uint32_t k = begin; k < end; k++) {
    R0H_REQUIRE((size_t)offsets[k] * 4 < into->bytes, "r0h_scatter_slices: offset %u outside the destination", offsets[k]);
    R0H_REQUIRE(values[k] < P, "r0h_scatter_slices: value %u is not a canonical field word", k);
  }
  const size_t bytes = (size_t)(end - begin) * 4;
  DevBuf tmp;  // [offsets][values]
  R0H_TRY(tmp.alloc(ctx, 2 * bytes));
  uint32_t* d_off = u32(tmp.get());
  uint32_t* d_val = d_off + (end - begin);
  R0H_TRY(stage_h2d(ctx, d_off, offsets + begin, bytes));
  R0H_TRY(stage_h2d(ctx, d_val, values + begin, bytes));
  hipLaunchKernelGGL(scatter_kernel, dim3((end - begin + 255) / 256), dim3(256), 0, ctx->stream, u32(into), d_off, d_val, 0u, end - begin);
  return launch_ok("scatter_kernel");
  R0H_GUARD_END
}

const char* r0h_fri_fold(r0h_ctx* ctx, r0h_buf* out, const r0h_buf* in, const uint32_t mix[4], uint32_t n_out) {
  R0H_REQUIRE(ctx && out && in && mix, "r0h_fri_fold: NULL argument");
  R0H_REQUIRE(canonical4(mix), "r0h_fri_fold: mix words must be canonical (< p)");
  R0H_REQUIRE((size_t)n_out * 16 <= out->bytes && (size_t)n_out * 16 * R0H_FRI_FOLD <= in->bytes, "r0h_fri_fold: n_out %u exceeds a buffer", n_out);
  if (!n_out) return nullptr;
  hipLaunchKernelGGL(fri_fold_kernel, dim3((n_out + 255) / 256), dim3(256), 0, ctx->stream, u32(out), u32(in), host_fp4(mix), n_out);
  return launch_ok("fri_fold_kernel");
}

const char* r0h_fri_fold_buf(r0h_ctx* ctx, r0h_buf* out, const r0h_buf* in, const r0h_buf* mix_buf, size_t mix_word_offset, uint32_t n_out) {
  R0H_REQUIRE(ctx && out && in && mix_buf, "r0h_fri_fold_buf: NULL argument");
  R0H_REQUIRE(mix_word_offset <= mix_buf->bytes / 4 && 4 <= mix_buf->bytes / 4 - mix_word_offset, "r0h_fri_fold_buf: the mix at words [%zu, +4) ends beyond a buffer of %zu words",
              mix_word_offset, mix_buf->bytes / 4);
  R0H_REQUIRE((size_t)n_out * 16 <= out->bytes && (size_t)n_out * 16 * R0H_FRI_FOLD <= in->bytes, "r0h_fri_fold_buf: n_out %u exceeds a buffer", n_out);
  if (!n_out) return nullptr;
  KScope ks(ctx, "fri_fold_buf_kernel", (double)n_out * 16 * (R0H_FRI_FOLD + 1));
  hipLaunchKernelGGL(fri_fold_buf_kernel, dim3((n_out + 255) / 256), dim3(256), 0, ctx->stream, u32(out), u32(in), u32(mix_buf) + mix_word_offset, n_out);
  return launch_ok("fri_fold_buf_kernel");
}

// ---- the device-challenge forms of steps 4-6 (internal.hpp) on their own: every challenge or table is (buffer, word offset)
const char* r0h_ext_powers_buf(r0h_ctx* ctx, r0h_buf* out, size_t out_word_offset, const r0h_buf* base_buf, size_t base_word_offset, const r0h_buf* exps_buf,
                               size_t exps_word_offset, uint32_t n) {
  R0H_REQUIRE(ctx && out && base_buf, "r0h_ext_powers_buf: NULL argument");
  R0H_TRY(require_words_in("r0h_ext_powers_buf", "output", out, out_word_offset, 4 * (size_t)n));
  R0H_TRY(require_words_in("r0h_ext_powers_buf", "base", base_buf, base_word_offset, 4));
  if (exps_buf) R0H_TRY(require_words_in("r0h_ext_powers_buf", "exponent table", exps_buf, exps_word_offset, n));
  return ext_powers(ctx, u32(out) + out_word_offset, u32(base_buf) + base_word_offset, exps_buf ? u32(exps_buf) + exps_word_offset : nullptr, n);
}

const char* r0h_batch_evaluate_any_points(r0h_ctx* ctx, const r0h_buf* coeffs, uint32_t po2, const uint32_t* which, const uint32_t* pt_idx, uint32_t n_eval,
                                          const r0h_buf* points_buf, size_t points_word_offset, uint32_t n_points, r0h_buf* out) {
  R0H_REQUIRE(ctx && coeffs && out && points_buf && (n_eval == 0 || (which && pt_idx)), "r0h_batch_evaluate_any_points: NULL argument");
  R0H_TRY(require_words_in("r0h_batch_evaluate_any_points", "point table", points_buf, points_word_offset, 4 * (size_t)n_points));
  return evaluate_any_points(ctx, coeffs, po2, which, pt_idx, n_eval, u32(points_buf) + points_word_offset, n_points, out, false);
}

const char* r0h_mix_poly_coeffs_mixbuf(r0h_ctx* ctx, r0h_buf* combos, uint32_t first_exp, const r0h_buf* mix_buf, size_t mix_word_offset, const r0h_buf* input,
                                       const uint32_t* combo_of, uint32_t input_count, uint32_t po2) {
  R0H_REQUIRE(ctx && combos && input && mix_buf, "r0h_mix_poly_coeffs_mixbuf: NULL argument");
  R0H_TRY(require_words_in("r0h_mix_poly_coeffs_mixbuf", "mix", mix_buf, mix_word_offset, 4));
  return mix_poly_coeffs_dev(ctx, combos, first_exp, u32(mix_buf) + mix_word_offset, input, combo_of, input_count, po2);
}

}  // extern "C"
