// Device side of a circuit: hipRTC compilation and module loading of the generated kernels, the launches of eval_check and of the
// witness checker, and the synthetic column program (witness generation, product accumulators).  Replaces the CircuitHal half of
// risc0-circuit-rv32im 4.0.4 / risc0-circuit-rv32im-sys 4.0.2 (`eval_check` + generated `poly_fp`, `generate_witness`, `step_accum`)
// -- SURVEY.md 8(a) a9-a11.  The blob is parsed by blob.cpp; the kernels' source text is written by evalcheck_emit.cpp.
#include <hip/hiprtc.h>

#include <memory>

#include "circuit.hpp"

namespace r0h {

static const char* compile_in_process(const std::string& src, std::vector<char>& code) {
  hiprtcProgram prog;
  hiprtcResult r = hiprtcCreateProgram(&prog, src.c_str(), "eval_check.hip", 0, nullptr, nullptr);
  R0H_REQUIRE(r == HIPRTC_SUCCESS, "hiprtcCreateProgram: %s", hiprtcGetErrorString(r));
  const char* opts[] = {"--offload-arch=gfx950", "-O3"};
  r = hiprtcCompileProgram(prog, 2, opts);
  if (r != HIPRTC_SUCCESS) {
    size_t n = 0;
    hiprtcGetProgramLogSize(prog, &n);
    std::string log(n, 0);
    if (n) hiprtcGetProgramLog(prog, &log[0]);
    hiprtcDestroyProgram(&prog);
    return make_error("hiprtcCompileProgram: %s\n%.2000s", hiprtcGetErrorString(r), log.c_str());
  }
  size_t n = 0;
  hiprtcGetCodeSize(prog, &n);
  code.resize(n);
  hiprtcGetCode(prog, code.data());
  hiprtcDestroyProgram(&prog);
  return nullptr;
}

// ------------------------------------------------------------------ synthetic witness + accumulation kernels
__global__ void witgen_fixed_kernel(uint32_t* __restrict__ buf, const uint32_t* __restrict__ kinds /* (kind, fixed_cell's arg) per col */,
                                    uint32_t po2, uint64_t seed_mixed, const uint32_t* __restrict__ periodic /* Montgomery */, uint32_t period) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x, col = blockIdx.y, kind = kinds[2 * col];
  if (kind > 6) return;  // derived column: filled later
  buf[((size_t)col << po2) + r] = fixed_cell(kind, kinds[2 * col + 1], r, 1u << po2, seed_mixed, periodic, period);
}
__global__ void witgen_derived_kernel(uint32_t* __restrict__ dst, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                      const uint32_t* __restrict__ c, const uint32_t* __restrict__ e, uint32_t ba, uint32_t bb,
                                      uint32_t bc, uint32_t be, uint32_t kind, uint32_t po2) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x, mask = (1u << po2) - 1;
  uint32_t prod = mul(a[(r - ba) & mask], b[(r - bb) & mask]);
  if (kind == 2) prod = mul(prod, c[(r - bc) & mask]);
  dst[r] = add(prod, e[(r - be) & mask]);
}
__device__ __forceinline__ void accum_term(uint32_t* __restrict__ term, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, const Fp4& m0, const Fp4& m1) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  Fp4 t = m0 + scale(m1, b[r]);
  t.e[0] = add(t.e[0], a[r]);
  *(uint4*)(term + 4 * (size_t)r) = make_uint4(t.e[0], t.e[1], t.e[2], t.e[3]);
}
__global__ void accum_term_kernel(uint32_t* __restrict__ term, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, Fp4 m0, Fp4 m1) {
  accum_term(term, a, b, m0, m1);
}
// the same term with the accumulator's two mix elements where a device transcript drew them: eight words at `mix` (r0h_accum_mixbuf)
__global__ void accum_term_mixbuf_kernel(uint32_t* __restrict__ term, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, const uint32_t* __restrict__ mix) {
  const Fp4 m0{{mix[0], mix[1], mix[2], mix[3]}}, m1{{mix[4], mix[5], mix[6], mix[7]}};
  accum_term(term, a, b, m0, m1);
}
// the checker's table before its kernels run: no row counted, no first row yet
__global__ void check_table_init_kernel(uint32_t* __restrict__ table, uint32_t n_terms) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n_terms) { table[2 * t] = 0u; table[2 * t + 1] = 0xffffffffu; }
}

}  // namespace r0h

using namespace r0h;

extern "C" {

static const char* read_code_object(const char* caller, const char* path, std::vector<char>& code) {
  FILE* f = fopen(path, "rb");
  R0H_REQUIRE(f, "%s: cannot open code object %s", caller, path);
  fseek(f, 0, SEEK_END);
  long sz = ftell(f);
  fseek(f, 0, SEEK_SET);
  code.resize(sz > 0 ? (size_t)sz : 0);
  size_t got = fread(code.data(), 1, code.size(), f);
  fclose(f);
  R0H_REQUIRE(got == code.size() && !code.empty(), "%s: short read of %s", caller, path);
  return nullptr;
}

// how a circuit goes, also on every early path out of r0h_circuit_load: its module (if one was loaded) is unloaded with it
struct CircuitUnload {
  void operator()(r0h_circuit* circuit) const {
    if (circuit->module) (void)hipModuleUnload(circuit->module);
    if (circuit->check_module) (void)hipModuleUnload(circuit->check_module);
    delete circuit;
  }
};

// One loader for both modules of a circuit: the code object at `code_object_path` -- or, without one, `emit`'s text compiled in
// process -- loaded, and its kernels <prefix>_0, <prefix>_1, ..: the first `required` of them must be there; with `open_ended` the
// code object decides how many more there are.  Nothing is handed out unless all of it worked.
static const char* load_module(const char* caller, const r0h_circuit* c, const char* code_object_path, std::string (*emit)(const r0h_circuit*), const char* prefix,
                               size_t required, bool open_ended, hipModule_t* module_out, std::vector<hipFunction_t>* kernels_out) {
  R0H_TRY_HIP(hipSetDevice(c->ctx->device));
  std::vector<char> code;
  if (code_object_path) R0H_TRY(read_code_object(caller, code_object_path, code));
  else R0H_TRY(compile_in_process(emit(c), code));
  hipModule_t module = nullptr;
  hipError_t e = hipModuleLoadData(&module, code.data());
  R0H_REQUIRE(e == hipSuccess, "%s: hipModuleLoadData: %s", caller, hipGetErrorString(e));
  std::vector<hipFunction_t> kernels;
  for (size_t k = 0; open_ended || k < required; k++) {
    char name[64];
    snprintf(name, sizeof name, "%s_%zu", prefix, k);
    hipFunction_t fn;
    if (hipModuleGetFunction(&fn, module, name) != hipSuccess) {
      (void)hipGetLastError();
      if (k >= required) break;
      (void)hipModuleUnload(module);
      return make_error("%s: the code object has no %s (built from another source?)", caller, name);
    }
    kernels.push_back(fn);
  }
  *module_out = module;
  kernels_out->swap(kernels);
  return nullptr;
}

const char* r0h_circuit_load(r0h_ctx* ctx, const uint32_t* blob, size_t n_words, const char* code_object_path, r0h_circuit** out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && blob && out, "r0h_circuit_load: NULL argument");
  std::unique_ptr<r0h_circuit, CircuitUnload> c(new r0h_circuit());
  c->ctx = ctx;
  R0H_TRY(parse_blob(c.get(), blob, n_words));
  make_plan(c.get());
  // the code object decides into how many kernels the program was cut: at least one, if there is a program at all
  R0H_TRY(load_module("r0h_circuit_load", c.get(), code_object_path, emit_source, "eval_check", c->plan.terms.empty() ? 0 : 1, true, &c->module, &c->kernels));
  ctx_retain(ctx);
  *out = c.release();
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_circuit_free(r0h_circuit* c) {
  if (!c) return nullptr;
  r0h_ctx* ctx = c->ctx;
  (void)hipSetDevice(ctx->device);
  (void)ctx_wait(ctx);
  ctx_code_commits_drop(ctx, c);  // the commitments of its CODE group go with the circuit
  CircuitUnload()(c);
  ctx_release(ctx);
  return nullptr;
}

uint32_t r0h_circuit_group_size(const r0h_circuit* c, uint32_t group) { return c && group < 3 ? c->group_size[group] : 0; }
uint32_t r0h_circuit_n_global(const r0h_circuit* c) { return c ? c->n_global : 0; }
uint32_t r0h_circuit_n_mix(const r0h_circuit* c) { return c ? c->n_mix : 0; }
uint32_t r0h_circuit_n_taps(const r0h_circuit* c) { return c ? (uint32_t)c->taps.size() : 0; }
uint32_t r0h_circuit_n_terms(const r0h_circuit* c) { return c ? (uint32_t)c->plan.terms.size() : 0; }

// the checker's module of `c`, under c->check_mu: its tallies are per term, so the cuts must be this plan's
static const char* check_module_load(const r0h_circuit* c, const char* caller, const char* code_object_path) {
  if (c->check_module) return nullptr;
  return load_module(caller, c, code_object_path, emit_check_source, "check_witness", c->plan.cut.size() - 1, false, &c->check_module, &c->check_kernels);
}

const char* r0h_circuit_load_check(r0h_circuit* c, const char* code_object_path) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(c, "r0h_circuit_load_check: NULL argument");
  std::lock_guard<std::mutex> lk(c->check_mu);
  R0H_REQUIRE(!c->check_module, "r0h_circuit_load_check: the circuit's checker is loaded already");
  return check_module_load(c, "r0h_circuit_load_check", code_object_path);
  R0H_GUARD_END
}

}  // extern "C"
namespace r0h {
// one launch of witgen_fixed_kernel over the columns `kinds` describes; the parameter block (kinds, then the PERIODIC section in
// Montgomery form) goes through a block from the pool, in stream order behind whatever read it last
static const char* witgen_fixed(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, std::vector<uint32_t>& kinds, uint64_t seed_mixed, r0h_buf* buf) {
  const uint32_t n = 1u << po2, threads = n < 256 ? n : 256, cols = (uint32_t)(kinds.size() / 2);
  const size_t table_at = kinds.size();
  for (uint32_t v : c->periodic) kinds.push_back(enc(v));
  DevBuf d_kinds;
  R0H_TRY(d_kinds.alloc(ctx, kinds.size() * 4));
  R0H_TRY(stage_h2d(ctx, d_kinds->ptr, kinds.data(), kinds.size() * 4));
  const uint32_t* dk = u32(d_kinds.get());
  hipLaunchKernelGGL(witgen_fixed_kernel, dim3(n / threads, cols), dim3(threads), 0, ctx->stream, u32(buf), dk, po2, seed_mixed, dk + table_at, c->period);
  return launch_ok("r0h_witgen");
}
const char* witgen_code(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, r0h_buf* code) {
  R0H_REQUIRE(ctx && c && code, "r0h_witgen: NULL argument");
  R0H_REQUIRE(c->has_column_program, "r0h_witgen: this circuit carries no synthetic column program (WITGEN/ACCUM sections); supply the witness");
  R0H_REQUIRE(po2 >= 4 && po2 <= R0H_MAX_PO2, "r0h_witgen: po2 %u outside [4, %u]", po2, R0H_MAX_PO2);
  const uint32_t nc = (uint32_t)c->code_cols.size();
  R0H_REQUIRE(((size_t)nc << po2) * 4 <= code->bytes, "r0h_witgen: buffers too small for 2^%u rows", po2);
  std::vector<uint32_t> kinds(2 * (size_t)nc);
  for (uint32_t k = 0; k < nc; k++) { kinds[2 * k] = c->code_cols[k].kind; kinds[2 * k + 1] = code_col_arg(c->code_cols[k], k); }
  return witgen_fixed(ctx, c, po2, kinds, splitmix64(CODE_SEED), code);
}
const char* code_commit_of(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, r0h_code_commit** out) {
  DevBuf code;
  R0H_TRY(code.alloc(ctx, ((size_t)c->group_size[R0H_GROUP_CODE] << po2) * 4));
  R0H_TRY(witgen_code(ctx, c, po2, code.get()));
  return r0h_code_commit_new(ctx, code.get(), c->group_size[R0H_GROUP_CODE], po2, out);
}
const char* ctx_code_commit(r0h_ctx* lane, const r0h_circuit* c, uint32_t po2, std::shared_ptr<r0h_code_commit>* out) {
  r0h_ctx* owner = c->ctx;
  std::lock_guard<std::mutex> lk(owner->code_commits_mu);
  const auto key = std::make_tuple(c, po2, lane->hashfn);  // (a helper lane follows its owner's suite: ctx_helper)
  auto it = owner->code_commits.find(key);
  if (it != owner->code_commits.end() && memcmp(&it->second.table, &lane->p2_host, sizeof(P2Consts)) != 0) {  // r0h_poseidon2_set_consts since
    owner->code_commits.erase(it);
    it = owner->code_commits.end();
  }
  if (it == owner->code_commits.end()) {
    r0h_code_commit* cc = nullptr;
    R0H_TRY(code_commit_of(lane, c, po2, &cc));
    std::shared_ptr<r0h_code_commit> held(cc, [](r0h_code_commit* p) { r0h_code_commit_free(p); });
    it = owner->code_commits.emplace(key, r0h_ctx::CodeCommitEntry{held, lane->p2_host}).first;
  }
  *out = it->second.cc;
  return nullptr;
}
void ctx_code_commits_drop(r0h_ctx* ctx, const r0h_circuit* c) {
  std::lock_guard<std::mutex> lk(ctx->code_commits_mu);
  for (auto it = ctx->code_commits.begin(); it != ctx->code_commits.end();) {
    if (c && std::get<0>(it->first) != c) { ++it; continue; }
    it = ctx->code_commits.erase(it);
  }
}
}  // namespace r0h
extern "C" {

static const char* witgen_impl(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, uint64_t seed, const uint32_t* global_in, r0h_buf* code,
                               r0h_buf* data, uint32_t* global_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && c && code && data, "r0h_witgen: NULL argument");
  R0H_REQUIRE(c->has_column_program, "r0h_witgen: this circuit carries no synthetic column program (WITGEN/ACCUM sections); supply the witness");
  R0H_REQUIRE(po2 >= 4 && po2 <= R0H_MAX_PO2, "r0h_witgen: po2 %u outside [4, %u]", po2, R0H_MAX_PO2);
  const uint32_t n = 1u << po2, threads = n < 256 ? n : 256, nc = (uint32_t)c->code_cols.size(), nd = (uint32_t)c->data_cols.size();
  R0H_REQUIRE(((size_t)nc << po2) * 4 <= code->bytes && ((size_t)nd << po2) * 4 <= data->bytes, "r0h_witgen: buffers too small for 2^%u rows", po2);
  R0H_TRY(witgen_code(ctx, c, po2, code));
  std::vector<uint32_t> kinds(2 * (size_t)nd);
  for (uint32_t k = 0; k < nd; k++) { kinds[2 * k] = c->data_cols[k].kind == 0 ? 3u : 99u; kinds[2 * k + 1] = (2u << 16) | k; }
  R0H_TRY(witgen_fixed(ctx, c, po2, kinds, splitmix64(seed), data));
  if (c->has_sponge) {
    // the sponge's columns hold the sponge over no words at all, and -- unless the caller names the public inputs -- the inputs its
    // digest is tied to are that digest (a caller who names them plants the rows of what it hashed instead: r0h_lift / r0h_join)
    R0H_TRY(sponge_plant(ctx, c, po2, nullptr, 0, data));
    if (!global_in) {
      uint32_t digest[8];
      p2_hash_elems_host(p2_default(), nullptr, 0, digest);
      for (uint32_t j = 0; j < 8; j++) R0H_TRY(stage_h2d(ctx, u32(data) + ((size_t)c->global_cols[c->sponge_global + j] << po2), digest + j, 4));
    }
  }
  if (global_in) {  // caller-chosen public inputs: row 0 of the (free) columns the globals are read from, before anything is derived from them
    for (uint32_t k = 0; k < c->n_global; k++) {
      R0H_REQUIRE(global_in[k] < P, "r0h_witgen_public: global %u is not a canonical field word", k);
      R0H_TRY(stage_h2d(ctx, u32(data) + ((size_t)c->global_cols[k] << po2), global_in + k, 4));
    }
  }
  for (uint32_t k = 0; k < nd; k++) {
    const DataCol& d = c->data_cols[k];
    if (d.kind == 0) continue;
    auto col = [&](uint32_t r) { return ((r >> 28) == R0H_GROUP_CODE ? u32(code) : u32(data)) + ((size_t)(r & 0xfffffu) << po2); };
    auto back = [](uint32_t r) { return (r >> 20) & 0xffu; };
    uint32_t rc = d.kind == 2 ? d.c : d.a;
    hipLaunchKernelGGL(witgen_derived_kernel, dim3(n / threads), dim3(threads), 0, ctx->stream, u32(data) + ((size_t)k << po2), col(d.a), col(d.b),
                       col(rc), col(d.e), back(d.a), back(d.b), back(rc), back(d.e), d.kind, po2);
  }
  R0H_TRY(launch_ok("r0h_witgen"));
  if (global_out) {
    for (uint32_t k = 0; k < c->n_global; k++)
      R0H_TRY_HIP(hipMemcpyAsync(global_out + k, u32(data) + ((size_t)c->global_cols[k] << po2), 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  R0H_TRY_HIP(ctx_wait(ctx));
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_witgen(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, uint64_t seed, r0h_buf* code, r0h_buf* data, uint32_t* global_out) {
  return witgen_impl(ctx, c, po2, seed, nullptr, code, data, global_out);
}

const char* r0h_witgen_public(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, uint64_t seed, const uint32_t* global_in, r0h_buf* code, r0h_buf* data) {
  R0H_REQUIRE(global_in || r0h_circuit_n_global(c) == 0, "r0h_witgen_public: global_in is NULL");
  return witgen_impl(ctx, c, po2, seed, global_in, code, data, nullptr);
}

// mix: the circuit's n_mix host words (r0h_accum), or nullptr with d_mix the same words on the device (r0h_accum_mixbuf)
static const char* accum_impl(const char* caller, r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* data, const uint32_t* mix, const uint32_t* d_mix, r0h_buf* accum) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && c && data && accum && (mix || d_mix || c->n_mix == 0), "%s: NULL argument", caller);
  R0H_REQUIRE(c->has_column_program, "%s: this circuit carries no synthetic column program (WITGEN/ACCUM sections)", caller);
  R0H_REQUIRE(po2 >= 4 && po2 <= R0H_MAX_PO2, "%s: po2 %u outside [4, %u]", caller, po2, R0H_MAX_PO2);
  const uint32_t n = 1u << po2, threads = n < 256 ? n : 256;
  R0H_REQUIRE(((size_t)c->data_cols.size() << po2) * 4 <= data->bytes && ((size_t)c->group_size[R0H_GROUP_ACCUM] << po2) * 4 <= accum->bytes,
              "%s: buffers too small for 2^%u rows", caller, po2);
  for (uint32_t i = 0; i < c->n_mix && mix; i++) R0H_REQUIRE(mix[i] < P, "%s: mix[%u] not canonical", caller, i);
  R0H_REQUIRE(c->logup.accs.empty(), "%s: this circuit accumulates a log-derivative argument that reads public inputs: use r0h_accum_public", caller);
  DevBuf term;
  R0H_TRY(term.alloc(ctx, (size_t)n * 16));
  for (uint32_t j = 0; j < c->acc_cols.size(); j++) {
    const uint32_t *a = u32(data) + ((size_t)c->acc_cols[j].a << po2), *b = u32(data) + ((size_t)c->acc_cols[j].b << po2);
    if (mix) {
      Fp4 m0{{mix[8 * j], mix[8 * j + 1], mix[8 * j + 2], mix[8 * j + 3]}}, m1{{mix[8 * j + 4], mix[8 * j + 5], mix[8 * j + 6], mix[8 * j + 7]}};
      hipLaunchKernelGGL(accum_term_kernel, dim3(n / threads), dim3(threads), 0, ctx->stream, u32(term.get()), a, b, m0, m1);
    } else {
      hipLaunchKernelGGL(accum_term_mixbuf_kernel, dim3(n / threads), dim3(threads), 0, ctx->stream, u32(term.get()), a, b, d_mix + 8 * (size_t)j);
    }
    R0H_TRY(r0h_prefix_products(ctx, term.get(), n));
    R0H_TRY(unpack_ext_columns(ctx, u32(accum) + ((size_t)(4 * j) << po2), u32(term.get()), po2));
  }
  return launch_ok(caller);
  R0H_GUARD_END
}
const char* r0h_accum(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, const uint32_t* mix, r0h_buf* accum) {
  (void)code;
  return accum_impl("r0h_accum", ctx, c, po2, data, mix, nullptr, accum);
}
// r0h_accum with the mix where a device transcript drew it: the circuit's n_mix words at word `mix_word_offset` of `mix_buf`.  Their
// canonicity is the producer's business, as for the other device-challenge forms.  Waits for nothing.
const char* r0h_accum_mixbuf(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, const r0h_buf* mix_buf, size_t mix_word_offset, r0h_buf* accum) {
  (void)code;
  R0H_REQUIRE(c && mix_buf, "r0h_accum_mixbuf: NULL argument");
  R0H_TRY(require_words_in("r0h_accum_mixbuf", "mix", mix_buf, mix_word_offset, c->n_mix));
  return accum_impl("r0h_accum_mixbuf", ctx, c, po2, data, nullptr, u32(mix_buf) + mix_word_offset, accum);
}

const char* r0h_accum_public(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* code, const r0h_buf* data, const uint32_t* global, const uint32_t* mix, r0h_buf* accum) {
  R0H_REQUIRE(ctx && c, "r0h_accum_public: NULL argument");
  if (c->logup.accs.empty()) return r0h_accum(ctx, c, po2, code, data, mix, accum);
  return logup_accum_kept(ctx, c, po2, code, data, global, mix, accum, nullptr);
}

// poly_mix: four host words (r0h_eval_check), or nullptr with d_poly_mix the four device words a transcript on the device drew (eval_check_dev)
static const char* eval_check_impl(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* eval_accum, const r0h_buf* eval_code, const r0h_buf* eval_data,
                                   const uint32_t* global, const uint32_t* mix, const uint32_t* poly_mix, const uint32_t* d_poly_mix, r0h_buf* check,
                                   const uint32_t* d_late = nullptr, const uint32_t* d_mix_words = nullptr) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && c && eval_accum && eval_code && eval_data && check && (poly_mix || d_poly_mix), "r0h_eval_check: NULL argument");
  R0H_REQUIRE((global || !c->n_global) && (mix || !c->n_mix), "r0h_eval_check: NULL globals");
  R0H_REQUIRE(po2 >= 6 && po2 <= R0H_MAX_PO2, "r0h_eval_check: po2 %u outside [6, %u]", po2, R0H_MAX_PO2);
  for (int q = 0; q < 4 && poly_mix; q++) R0H_REQUIRE(poly_mix[q] < P, "r0h_eval_check: poly_mix words must be canonical (< p)");
  const size_t domain = (size_t)4 << po2;
  const r0h_buf* g[3] = {eval_accum, eval_code, eval_data};
  for (int k = 0; k < 3; k++) R0H_REQUIRE(domain * c->group_size[k] * 4 <= g[k]->bytes, "r0h_eval_check: group %d buffer too small", k);
  R0H_REQUIRE(domain * 16 <= check->bytes, "r0h_eval_check: check buffer too small");
  // parameters: globals, mix, powers of poly_mix, inverse vanishing values
  std::vector<uint32_t> params(c->n_global + c->n_mix + 4 * (size_t)c->plan.n_pow + 4);
  uint32_t* p = params.data();
  for (uint32_t i = 0; i < c->n_global; i++) { R0H_REQUIRE(global[i] < P, "r0h_eval_check: global[%u] not canonical", i); *p++ = global[i]; }
  for (uint32_t i = 0; i < c->n_mix; i++) { R0H_REQUIRE(mix[i] < P, "r0h_eval_check: mix[%u] not canonical", i); *p++ = mix[i]; }
  if (poly_mix) {
    Fp4 pm{{poly_mix[0], poly_mix[1], poly_mix[2], poly_mix[3]}}, cur = fp4_one();
    for (uint32_t k = 0; k < c->plan.n_pow; k++) { memcpy(p, cur.e, 16); p += 4; cur = cur * pm; }
  } else {
    p += 4 * (size_t)c->plan.n_pow;  // filled on the device, below
  }
  {
    uint32_t three_n = fpow(enc(3), (uint64_t)1 << po2), w4 = rou_fwd(2), w = ONE;
    for (int k = 0; k < 4; k++) { *p++ = inv(sub(mul(three_n, w), ONE)); w = mul(w, w4); }
  }
  // the parameter block comes from the calling context's pool (stream-ordered reuse), not from the circuit: one loaded circuit
  // then serves every context of its device at once (r0h_prove_elf's prover lanes share it)
  DevBuf pbuf;
  R0H_TRY(pbuf.alloc(ctx, params.size() * 4));
  R0H_TRY(stage_h2d(ctx, pbuf->ptr, params.data(), params.size() * 4));
  uint32_t* d_check = u32(check);
  const uint32_t *g0 = u32(g[0]), *g1 = u32(g[1]), *g2 = u32(g[2]);
  const uint32_t *d_glob = u32(pbuf.get()), *d_mix = d_glob + c->n_global, *d_pow = d_mix + c->n_mix, *d_van = d_pow + 4 * (size_t)c->plan.n_pow;
  if (!poly_mix) R0H_TRY(ext_powers(ctx, const_cast<uint32_t*>(d_pow), d_poly_mix, nullptr, c->plan.n_pow));
  // the late public inputs and the mix where a device transcript left them: over the host's words, behind their upload in stream order
  if (d_late && c->n_late) R0H_TRY_HIP(hipMemcpyAsync(const_cast<uint32_t*>(d_glob) + (c->n_global - c->n_late), d_late, (size_t)c->n_late * 4, hipMemcpyDeviceToDevice, ctx->stream));
  if (d_mix_words && c->n_mix) R0H_TRY_HIP(hipMemcpyAsync(const_cast<uint32_t*>(d_mix), d_mix_words, (size_t)c->n_mix * 4, hipMemcpyDeviceToDevice, ctx->stream));
  double alg = (double)domain * 16;
  for (int k = 0; k < 3; k++) alg += (double)domain * c->group_size[k] * 4;
  KScope ks(ctx, "eval_check", alg);
  for (size_t k = 0; k < c->kernels.size(); k++) {
    uint32_t accumulate = k ? 1u : 0u;
    void* args[] = {&d_check, &g0, &g1, &g2, &d_glob, &d_mix, &d_pow, &d_van, &po2, &accumulate};
    R0H_TRY_HIP(hipModuleLaunchKernel(c->kernels[k], (uint32_t)(domain / 256), 1, 1, 256, 1, 1, 0, ctx->stream, args, nullptr));
  }
  if (c->kernels.empty()) R0H_TRY_HIP(hipMemsetAsync(check->ptr, 0, domain * 16, ctx->stream));
  return nullptr;
  R0H_GUARD_END
}
const char* r0h_eval_check(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* eval_accum, const r0h_buf* eval_code,
                           const r0h_buf* eval_data, const uint32_t* global, const uint32_t* mix, const uint32_t poly_mix[4], r0h_buf* check) {
  R0H_REQUIRE(poly_mix, "r0h_eval_check: NULL argument");
  return eval_check_impl(ctx, c, po2, eval_accum, eval_code, eval_data, global, mix, poly_mix, nullptr, check);
}
}  // extern "C"
namespace r0h {
const char* eval_check_dev(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* eval_accum, const r0h_buf* eval_code, const r0h_buf* eval_data,
                           const uint32_t* global, const uint32_t* mix, const uint32_t* d_poly_mix, r0h_buf* check, const uint32_t* d_late, const uint32_t* d_mix) {
  R0H_REQUIRE(d_poly_mix, "r0h_eval_check: NULL argument");
  return eval_check_impl(ctx, c, po2, eval_accum, eval_code, eval_data, global, mix, nullptr, d_poly_mix, check, d_late, d_mix);
}
}  // namespace r0h
extern "C" {

const char* r0h_eval_check_mixbuf(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* eval_accum, const r0h_buf* eval_code, const r0h_buf* eval_data,
                                  const uint32_t* global, const uint32_t* mix, const r0h_buf* poly_mix_buf, size_t poly_mix_word_offset, r0h_buf* check) {
  R0H_REQUIRE(poly_mix_buf, "r0h_eval_check_mixbuf: NULL argument");
  R0H_TRY(require_words_in("r0h_eval_check_mixbuf", "poly_mix", poly_mix_buf, poly_mix_word_offset, 4));
  return r0h::eval_check_dev(ctx, c, po2, eval_accum, eval_code, eval_data, global, mix, u32(poly_mix_buf) + poly_mix_word_offset, check);
}

const char* r0h_check_witness(r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* accum, const r0h_buf* code, const r0h_buf* data,
                              const uint32_t* global, const uint32_t* mix, r0h_violation* out, size_t capacity, size_t* n_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && c && code && data && n_out && (out || !capacity), "r0h_check_witness: NULL argument");
  R0H_REQUIRE((global || !c->n_global) && (mix || !c->n_mix || !accum), "r0h_check_witness: NULL globals");
  R0H_REQUIRE(po2 >= 6 && po2 <= R0H_MAX_PO2, "r0h_check_witness: po2 %u outside [6, %u]", po2, R0H_MAX_PO2);
  R0H_REQUIRE(c->ctx->device == ctx->device, "r0h_check_witness: the circuit lives on device %d, this context on device %d", c->ctx->device, ctx->device);
  const size_t n = (size_t)1 << po2;
  const r0h_buf* g[3] = {accum, code, data};
  for (int k = 0; k < 3; k++) R0H_REQUIRE(!g[k] || n * c->group_size[k] * 4 <= g[k]->bytes, "r0h_check_witness: group %d buffer too small", k);
  const uint32_t n_terms = (uint32_t)c->plan.terms.size();
  *n_out = 0;
  if (!n_terms) return nullptr;
  {
    std::lock_guard<std::mutex> lk(c->check_mu);
    R0H_TRY(check_module_load(c, "r0h_check_witness", nullptr));
  }
  // parameters: globals and mix, then the table
  const size_t n_params = (size_t)c->n_global + c->n_mix;
  std::vector<uint32_t> params(n_params + 1, 0);
  for (uint32_t i = 0; i < c->n_global; i++) { R0H_REQUIRE(global[i] < P, "r0h_check_witness: global[%u] not canonical", i); params[i] = global[i]; }
  for (uint32_t i = 0; i < c->n_mix && accum; i++) { R0H_REQUIRE(mix[i] < P, "r0h_check_witness: mix[%u] not canonical", i); params[c->n_global + i] = mix[i]; }
  DevBuf pbuf;
  R0H_TRY(pbuf.alloc(ctx, (n_params + 1 + 2 * (size_t)n_terms) * 4));
  R0H_TRY(stage_h2d(ctx, pbuf->ptr, params.data(), params.size() * 4));
  const uint32_t *d_glob = u32(pbuf.get()), *d_mix = d_glob + c->n_global;
  uint32_t* d_table = u32(pbuf.get()) + n_params + 1;
  const uint32_t *g0 = accum ? u32(accum) : nullptr, *g1 = u32(code), *g2 = u32(data);
  std::vector<uint32_t> table(2 * (size_t)n_terms);
  {
    double alg = 0;
    for (int k = 0; k < 3; k++) alg += g[k] ? (double)n * c->group_size[k] * 4 : 0.0;
    KScope ks(ctx, "check_witness", alg);
    hipLaunchKernelGGL(check_table_init_kernel, dim3((n_terms + 255) / 256), dim3(256), 0, ctx->stream, d_table, n_terms);
    R0H_TRY(launch_ok("r0h_check_witness"));
    const uint32_t threads = n < 256 ? (uint32_t)n : 256u;  // whole waves: a lane per row, 2^po2 >= 64 rows
    uint32_t with_accum = accum ? 1u : 0u;
    for (hipFunction_t fn : c->check_kernels) {
      void* args[] = {&d_table, &g0, &g1, &g2, &d_glob, &d_mix, &po2, &with_accum};
      R0H_TRY_HIP(hipModuleLaunchKernel(fn, (uint32_t)(n / threads), 1, 1, threads, 1, 1, 0, ctx->stream, args, nullptr));
    }
  }
  R0H_TRY_HIP(hipMemcpyAsync(table.data(), d_table, table.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
  R0H_TRY_HIP(ctx_wait(ctx));
  size_t found = 0;
  for (uint32_t t = 0; t < n_terms; t++) {
    if (!table[2 * t]) continue;
    if (found < capacity) out[found] = r0h_violation{t, table[2 * t], table[2 * t + 1], 0};
    found++;
  }
  *n_out = found;
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_ctx_set_check_witness(r0h_ctx* ctx, int on) {
  R0H_REQUIRE(ctx, "r0h_ctx_set_check_witness: ctx is NULL");
  ctx->check_witness = on != 0;
  for (r0h_ctx* h : ctx->helpers) h->check_witness = ctx->check_witness;
  return nullptr;
}

}  // extern "C"

namespace r0h {
const char* require_witness(const char* caller, r0h_ctx* ctx, const r0h_circuit* c, uint32_t po2, const r0h_buf* accum, const r0h_buf* code, const r0h_buf* data,
                            const uint32_t* global, const uint32_t* mix) {
  r0h_violation first = {0, 0, 0, 0};
  size_t n_bad = 0;
  R0H_TRY(r0h_check_witness(ctx, c, po2, accum, code, data, global, mix, &first, 1, &n_bad));
  R0H_REQUIRE(!n_bad, "%s: the witness violates %zu of the circuit's %zu constraint terms: term %u does not vanish on %u of 2^%u rows, first at row %u",
              caller, n_bad, c->plan.terms.size(), first.term, first.rows, po2, first.first_row);
  return nullptr;
}
}  // namespace r0h
