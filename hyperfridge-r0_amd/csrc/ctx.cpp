// Context, device buffers, error strings, constant tables.
// Replaces the host-side glue of risc0-zkp 3.0.4 hal/{cuda,metal}.rs (`alloc_elem`, `copy_from_*`, buffer slicing) and
// risc0-sys 1.5.0's C-string error convention.
#include <stdarg.h>

#include <exception>
#include <stdexcept>

#include "internal.hpp"
#include "poseidon2_dot_schedule.hpp"

namespace r0h {

const char* make_error(const char* fmt, ...) {
  char tmp[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(tmp, sizeof tmp, fmt, ap);
  va_end(ap);
  char* out = (char*)malloc(strlen(tmp) + 1);
  if (!out) return "r0hip: out of memory while formatting an error";
  strcpy(out, tmp);
  return out;
}

const char* stage_h2d(r0h_ctx* ctx, void* dst, const void* src, size_t bytes) {
  if (!bytes) return nullptr;
  if (bytes > ctx->pinned_bytes / 2) {  // too large for the ring: plain blocking copy
    R0H_TRY_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    R0H_TRY_HIP(ctx_wait(ctx));
    return nullptr;
  }
  size_t need = (bytes + 255) & ~(size_t)255;
  if (ctx->pinned_off + need > ctx->pinned_bytes) {
    R0H_TRY_HIP(ctx_wait(ctx));  // every earlier ring slot has been consumed
    ctx->ring_waits++;
    ctx->pinned_off = 0;
  }
  char* slot = (char*)ctx->pinned + ctx->pinned_off;
  memcpy(slot, src, bytes);
  ctx->pinned_off += need;
  R0H_TRY_HIP(hipMemcpyAsync(dst, slot, bytes, hipMemcpyHostToDevice, ctx->stream));
  return nullptr;
}

const char* buf_alloc_pooled(r0h_ctx* ctx, size_t bytes, r0h_buf** out) {
  size_t sz = bytes ? (bytes + 255) & ~(size_t)255 : 256;
  r0h_buf* b = new r0h_buf();
  b->ctx = ctx; b->bytes = bytes; b->pooled = true;
  auto it = ctx->pool.find(sz);
  if (it != ctx->pool.end()) {
    b->ptr = it->second;
    ctx->pool.erase(it);
    ctx->pool_bytes -= sz;
  } else {
    hipError_t e = hipMalloc(&b->ptr, sz);
    if (e != hipSuccess && !ctx->pool.empty()) {
      // out of memory with blocks of other sizes parked: give them back and try once more
      (void)hipGetLastError();
      (void)ctx_wait(ctx);
      for (auto& kv : ctx->pool) (void)hipFree(kv.second);
      ctx->pool.clear();
      ctx->pool_bytes = 0;
      e = hipMalloc(&b->ptr, sz);
    }
    if (e != hipSuccess) {
      (void)hipGetLastError();
      delete b;
      return make_error("device allocation of %zu bytes failed: %s", sz, hipGetErrorString(e));
    }
  }
  ctx_retain(ctx);
  *out = b;
  return nullptr;
}

r0h_buf buf_view(const r0h_buf* b, size_t offset_bytes, size_t bytes) {
  if (offset_bytes > b->bytes || bytes > b->bytes - offset_bytes) throw std::out_of_range("buf_view: window outside its buffer");
  r0h_buf v;
  v.ctx = b->ctx; v.ptr = (char*)b->ptr + offset_bytes; v.bytes = bytes; v.owned = false;
  return v;
}

const char* launch_ok(const char* what) {
  hipError_t e = hipGetLastError();
  R0H_REQUIRE(e == hipSuccess, "%s: launch failed: %s", what, hipGetErrorString(e));
  return nullptr;
}

void profile_phase(r0h_ctx* ctx, const char* name) {
  Profile& p = ctx->prof;
  size_t i = p.names.size();
  if (p.events.size() <= i) {
    hipEvent_t e;
    (void)hipEventCreate(&e);
    p.events.push_back(e);
  }
  (void)hipEventRecord(p.events[i], ctx->stream);
  p.names.push_back(name);
}
void profile_end(r0h_ctx* ctx) { profile_phase(ctx, "end"); }
const char* profile_close(r0h_ctx* ctx) {
  profile_end(ctx);
  return profile_collect(ctx);
}
const char* profile_collect(r0h_ctx* ctx) {
  R0H_TRY_HIP(ctx_wait(ctx));
  Profile& p = ctx->prof;
  std::vector<float> ms(p.names.size() - 1, 0.f);
  for (size_t i = 0; i < ms.size(); i++) (void)hipEventElapsedTime(&ms[i], p.events[i], p.events[i + 1]);
  p.closed_names.assign(p.names.begin(), p.names.end() - 1);  // ("end" names no phase)
  p.closed_ms.swap(ms);
  return nullptr;
}

void ctx_retain(r0h_ctx* ctx) { ctx->refs++; }
const char* ctx_helper(r0h_ctx* ctx, size_t k, r0h_ctx** out) {
  while (ctx->helpers.size() <= k) {
    r0h_ctx* h = nullptr;
    R0H_TRY(r0h_ctx_create(ctx->device, &h));
    ctx->helpers.push_back(h);
  }
  r0h_ctx* h = ctx->helpers[k];
  h->check_witness = ctx->check_witness;
  h->check_balance = ctx->check_balance;
  h->check_session = ctx->check_session;
  h->device_transcript = ctx->device_transcript;
  h->device_finish = ctx->device_finish;
  h->hashfn = ctx->hashfn;
  h->merkle_fused_tops = ctx->merkle_fused_tops;
  h->p2_tight = ctx->p2_tight;  // goes with the table below
  if (memcmp(&h->p2_host, &ctx->p2_host, sizeof(P2Consts)) != 0) {  // r0h_poseidon2_set_consts on the owner since the helper was made
    h->p2_host = ctx->p2_host;
    R0H_TRY_HIP(hipSetDevice(h->device));
    R0H_TRY_HIP(ctx_wait(h));
    R0H_TRY_HIP(hipMemcpy(h->p2, &h->p2_host, sizeof(P2Consts), hipMemcpyHostToDevice));
  }
  *out = h;
  return nullptr;
}
void ctx_release(r0h_ctx* ctx) {
  if (--ctx->refs > 0) return;
  session_rows_free(ctx);
  for (r0h_ctx* h : ctx->helpers) r0h_ctx_destroy(h);
  ctx->helpers.clear();
  (void)hipSetDevice(ctx->device);
  (void)ctx_wait(ctx);
  for (int d = 0; d < 2; d++) { (void)hipFree(ctx->tw_lo[d]); (void)hipFree(ctx->tw_hi[d]); (void)hipFree(ctx->tw12[d]); }
  for (int d = 0; d < 2; d++) { (void)hipFree(ctx->twb_lo[d]); (void)hipFree(ctx->twb_hi[d]); }
  (void)hipFree(ctx->pow3_lo); (void)hipFree(ctx->pow3_hi); (void)hipFree(ctx->pow3_top); (void)hipFree(ctx->p2);
  (void)hipHostFree(ctx->pinned);
  for (auto& kv : ctx->pool) (void)hipFree(kv.second);
  for (hipEvent_t e : ctx->prof.events) (void)hipEventDestroy(e);
  for (auto& kv : ctx->ktimers)
    for (hipEvent_t e : kv.second.ev) (void)hipEventDestroy(e);
  (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

static const char* upload_pow_table(uint32_t** dst, uint32_t base, uint32_t n) {
  std::vector<uint32_t> t(n);
  uint32_t cur = ONE;
  for (uint32_t i = 0; i < n; i++) { t[i] = cur; cur = mul(cur, base); }
  R0H_TRY_HIP(hipMalloc((void**)dst, n * 4));
  R0H_TRY_HIP(hipMemcpy(*dst, t.data(), n * 4, hipMemcpyHostToDevice));
  return nullptr;
}

}  // namespace r0h

using namespace r0h;

extern "C" {

void r0h_free_error(const char* msg) { free((void*)msg); }
const char* r0h_version(void) { return "r0hip 0.1 (gfx950)"; }

const char* r0h_ctx_create(int device, r0h_ctx** out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(out, "r0h_ctx_create: out is NULL");
  int n = 0;
  R0H_TRY_HIP(hipGetDeviceCount(&n));
  R0H_REQUIRE(device >= 0 && device < n, "r0h_ctx_create: device %d not present (%d visible); no CPU fallback exists", device, n);
  R0H_TRY_HIP(hipSetDevice(device));
  R0H_TRY(ntt_init_device());
  r0h_ctx* ctx = new r0h_ctx();
  ctx->device = device;
  R0H_TRY_HIP(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
  for (int d = 0; d < 2; d++) {
    uint32_t w22 = d == 0 ? rou_fwd(TW_TOP) : rou_rev(TW_TOP), w26 = d == 0 ? rou_fwd(MAX_DOMAIN_PO2) : rou_rev(MAX_DOMAIN_PO2);
    R0H_TRY(upload_pow_table(&ctx->twb_lo[d], w26, TWB_SIZE));
    R0H_TRY(upload_pow_table(&ctx->twb_hi[d], fpow(w26, TWB_SIZE), TWB_SIZE));
    R0H_TRY(upload_pow_table(&ctx->tw_lo[d], w22, TW_SIZE));
    R0H_TRY(upload_pow_table(&ctx->tw_hi[d], fpow(w22, TW_SIZE), TW_SIZE));
    R0H_TRY(upload_pow_table(&ctx->tw12[d], d == 0 ? rou_fwd(TWL_BITS) : rou_rev(TWL_BITS), 1u << (TWL_BITS - 1)));
  }
  R0H_TRY(upload_pow_table(&ctx->pow3_lo, enc(3), TW_SIZE));
  R0H_TRY(upload_pow_table(&ctx->pow3_hi, fpow(enc(3), TW_SIZE), TW_SIZE));
  R0H_TRY(upload_pow_table(&ctx->pow3_top, fpow(enc(3), (uint64_t)1 << TW_TOP), 1u << (MAX_DOMAIN_PO2 - TW_TOP)));
  R0H_TRY_HIP(hipMalloc((void**)&ctx->p2, sizeof(P2Consts)));
  ctx->p2_host = p2_default();
  ctx->p2_tight = p2_dot_schedule_covers(P2_DOT_TIGHT, ctx->p2_host.part_sigma, ctx->p2_host.part_final);
  R0H_TRY_HIP(hipMemcpy(ctx->p2, &ctx->p2_host, sizeof(P2Consts), hipMemcpyHostToDevice));
  ctx->pinned_bytes = 8u << 20;
  R0H_TRY_HIP(hipHostMalloc(&ctx->pinned, ctx->pinned_bytes, hipHostMallocDefault));
  *out = ctx;
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_ctx_destroy(r0h_ctx* ctx) {
  if (!ctx) return nullptr;
  (void)hipSetDevice(ctx->device);
  (void)ctx_wait(ctx);
  ctx_code_commits_drop(ctx, nullptr);  // cached CODE commitments hold references of their own: they go first, their buffers while the device state is whole
  ctx_release(ctx);  // buffers and circuits still alive keep the device state until they are freed
  return nullptr;
}

const char* r0h_sync(r0h_ctx* ctx) {
  R0H_REQUIRE(ctx, "r0h_sync: ctx is NULL");
  R0H_TRY_HIP(ctx_wait(ctx));
  return nullptr;
}

const char* r0h_ctx_set_device_transcript(r0h_ctx* ctx, int on) {
  R0H_REQUIRE(ctx, "r0h_ctx_set_device_transcript: ctx is NULL");
  ctx->device_transcript = on != 0;
  for (r0h_ctx* h : ctx->helpers) h->device_transcript = ctx->device_transcript;
  return nullptr;
}
const char* r0h_ctx_set_device_finish(r0h_ctx* ctx, int on) {
  R0H_REQUIRE(ctx, "r0h_ctx_set_device_finish: ctx is NULL");
  ctx->device_finish = on != 0;
  for (r0h_ctx* h : ctx->helpers) h->device_finish = ctx->device_finish;
  return nullptr;
}
const char* r0h_ctx_set_session_enqueue(r0h_ctx* ctx, int on) {
  R0H_REQUIRE(ctx, "r0h_ctx_set_session_enqueue: ctx is NULL");
  ctx->session_enqueue = on != 0 ? 1 : 0;
  return nullptr;
}
const char* r0h_ctx_set_session_enqueue_begin(r0h_ctx* ctx, int on) {
  R0H_REQUIRE(ctx, "r0h_ctx_set_session_enqueue_begin: ctx is NULL");
  ctx->session_enqueue_begin = on != 0 ? 1 : 0;
  return nullptr;
}
const char* r0h_ctx_set_merkle_fused_tops(r0h_ctx* ctx, int on) {
  R0H_REQUIRE(ctx, "r0h_ctx_set_merkle_fused_tops: ctx is NULL");
  ctx->merkle_fused_tops = on != 0 ? 1 : 0;
  for (r0h_ctx* h : ctx->helpers) h->merkle_fused_tops = ctx->merkle_fused_tops;
  return nullptr;
}
const char* r0h_ctx_blocking_waits(const r0h_ctx* ctx, uint64_t* count_out) {
  R0H_REQUIRE(ctx && count_out, "r0h_ctx_blocking_waits: NULL argument");
  *count_out = ctx->blocking_waits.load();
  return nullptr;
}

const char* r0h_poseidon2_set_consts(r0h_ctx* ctx, const uint32_t* rc, const uint32_t* diag_m1) {
  R0H_REQUIRE(ctx && rc && diag_m1, "r0h_poseidon2_set_consts: NULL argument");
  for (int i = 0; i < P2_CELLS * P2_ROUNDS; i++) R0H_REQUIRE(rc[i] < P, "round constant %d not canonical", i);
  for (int i = 0; i < P2_CELLS; i++) R0H_REQUIRE(diag_m1[i] < P, "diagonal word %d not canonical", i);
  ctx->p2_tight = fill_p2(ctx->p2_host, rc, diag_m1);
  R0H_TRY_HIP(ctx_wait(ctx));
  R0H_TRY_HIP(hipMemcpy(ctx->p2, &ctx->p2_host, sizeof(P2Consts), hipMemcpyHostToDevice));
  return nullptr;
}

const char* r0h_poseidon2_dot_schedule(const r0h_ctx* ctx, int* tight) {
  R0H_REQUIRE(ctx && tight, "r0h_poseidon2_dot_schedule: NULL argument");
  *tight = ctx->p2_tight ? 1 : 0;
  return nullptr;
}

const char* r0h_buf_alloc(r0h_ctx* ctx, size_t bytes, r0h_buf** out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && out, "r0h_buf_alloc: NULL argument");
  R0H_TRY_HIP(hipSetDevice(ctx->device));
  r0h_buf* b = new r0h_buf();
  b->ctx = ctx;
  b->bytes = bytes;
  hipError_t e = hipMalloc(&b->ptr, bytes ? bytes : 4);
  if (e != hipSuccess) {
    delete b;
    return make_error("r0h_buf_alloc(%zu bytes): %s", bytes, hipGetErrorString(e));
  }
  ctx_retain(ctx);
  *out = b;
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_buf_wrap(r0h_ctx* ctx, void* device_ptr, size_t bytes, r0h_buf** out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && out && device_ptr, "r0h_buf_wrap: NULL argument");
  r0h_buf* b = new r0h_buf();
  b->ctx = ctx; b->ptr = device_ptr; b->bytes = bytes; b->owned = false;
  ctx_retain(ctx);
  *out = b;
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_buf_slice(r0h_buf* parent, size_t off, size_t bytes, r0h_buf** out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(parent && out, "r0h_buf_slice: NULL argument");
  R0H_REQUIRE(off % 4 == 0 && off + bytes <= parent->bytes, "r0h_buf_slice: [%zu, +%zu) outside a %zu-byte buffer", off, bytes, parent->bytes);
  r0h_buf* b = new r0h_buf();
  b->ctx = parent->ctx; b->ptr = (char*)parent->ptr + off; b->bytes = bytes; b->parent = parent; b->owned = false;
  parent->refs++;
  ctx_retain(parent->ctx);
  *out = b;
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_buf_free(r0h_buf* b) {
  while (b) {
    if (--b->refs > 0) break;
    r0h_buf* parent = b->parent;
    if (b->pooled && b->ptr) {
      // stream-ordered reuse: whoever takes this block next enqueues behind everything that used it
      const size_t sz = b->bytes ? (b->bytes + 255) & ~(size_t)255 : 256;
      if (b->ctx->pool_bytes + sz > POOL_LIMIT) {
        (void)ctx_wait(b->ctx);
        (void)hipFree(b->ptr);
      } else {
        b->ctx->pool.emplace(sz, b->ptr);
        b->ctx->pool_bytes += sz;
      }
    } else if (b->owned && b->ptr) {
      (void)hipSetDevice(b->ctx->device);  // best effort before the free: a failure here shows up as the free's error
      (void)ctx_wait(b->ctx);
      hipError_t e = hipFree(b->ptr);
      if (e != hipSuccess) return make_error("r0h_buf_free: %s", hipGetErrorString(e));
    }
    r0h_ctx* ctx = b->ctx;
    delete b;
    ctx_release(ctx);
    b = parent;
  }
  return nullptr;
}

const char* r0h_buf_h2d(r0h_ctx* ctx, r0h_buf* dst, size_t off, const void* src, size_t bytes) {
  R0H_REQUIRE(ctx && dst && (src || !bytes), "r0h_buf_h2d: NULL argument");
  R0H_REQUIRE(off + bytes <= dst->bytes, "r0h_buf_h2d: [%zu, +%zu) outside a %zu-byte buffer", off, bytes, dst->bytes);
  if (!bytes) return nullptr;
  R0H_TRY_HIP(hipMemcpyAsync((char*)dst->ptr + off, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  R0H_TRY_HIP(ctx_wait(ctx));  // src is pageable caller memory: do not outlive the call
  return nullptr;
}

const char* r0h_buf_d2h(r0h_ctx* ctx, const r0h_buf* src, size_t off, void* dst, size_t bytes) {
  R0H_REQUIRE(ctx && src && (dst || !bytes), "r0h_buf_d2h: NULL argument");
  R0H_REQUIRE(off + bytes <= src->bytes, "r0h_buf_d2h: [%zu, +%zu) outside a %zu-byte buffer", off, bytes, src->bytes);
  if (!bytes) return nullptr;
  R0H_TRY_HIP(hipMemcpyAsync(dst, (const char*)src->ptr + off, bytes, hipMemcpyDeviceToHost, ctx->stream));
  R0H_TRY_HIP(ctx_wait(ctx));
  return nullptr;
}

const char* r0h_buf_zero(r0h_ctx* ctx, r0h_buf* buf) {
  R0H_REQUIRE(ctx && buf, "r0h_buf_zero: NULL argument");
  R0H_TRY_HIP(hipMemsetAsync(buf->ptr, 0, buf->bytes, ctx->stream));
  return nullptr;
}

const char* r0h_ctx_set_session_resident_limit(r0h_ctx* ctx, uint64_t bytes) {
  R0H_REQUIRE(ctx, "r0h_ctx_set_session_resident_limit: ctx is NULL");
  ctx->session_resident_limit = bytes;
  return nullptr;
}
const char* r0h_ctx_set_session_device_limit(r0h_ctx* ctx, uint64_t bytes) {
  R0H_REQUIRE(ctx, "r0h_ctx_set_session_device_limit: ctx is NULL");
  ctx->session_device_limit = bytes;
  return nullptr;
}
const char* r0h_last_session_device(r0h_ctx* ctx, uint64_t out[4]) {
  R0H_REQUIRE(ctx && out, "r0h_last_session_device: NULL argument");
  memcpy(out, ctx->session_device, sizeof ctx->session_device);
  return nullptr;
}
uint64_t r0h_ctx_session_held_bytes(const r0h_ctx* ctx) { return ctx ? ctx->session_held.load() : 0; }
const char* r0h_ctx_set_session_tree_tops(r0h_ctx* ctx, uint32_t levels) {
  R0H_REQUIRE(ctx, "r0h_ctx_set_session_tree_tops: ctx is NULL");
  R0H_REQUIRE(levels <= R0H_MERKLE_TOP_MAX_LEVELS, "r0h_ctx_set_session_tree_tops: levels %u outside [0, %u] (0: off)", levels, (unsigned)R0H_MERKLE_TOP_MAX_LEVELS);
  ctx->session_tree_tops = levels;
  return nullptr;
}
const char* r0h_last_session_tree_tops(r0h_ctx* ctx, uint64_t out[3]) {
  R0H_REQUIRE(ctx && out, "r0h_last_session_tree_tops: NULL argument");
  memcpy(out, ctx->session_tops, sizeof ctx->session_tops);
  return nullptr;
}
const char* r0h_kernel_timing(r0h_ctx* ctx, int enable) {
  R0H_REQUIRE(ctx, "r0h_kernel_timing: ctx is NULL");
  R0H_TRY_HIP(ctx_wait(ctx));
  ctx->ktime_on = enable != 0;
  for (auto& kv : ctx->ktimers) { kv.second.used = 0; kv.second.alg_bytes = 0; }
  return nullptr;
}

const char* r0h_kernel_stats(r0h_ctx* ctx, char* json_out, size_t capacity) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && json_out && capacity, "r0h_kernel_stats: NULL argument");
  R0H_TRY_HIP(ctx_wait(ctx));
  std::string js = "{";
  bool first = true;
  for (auto& kv : ctx->ktimers) {
    double total = 0;
    for (size_t i = 0; i + 1 < kv.second.used; i += 2) {
      float ms = 0;
      R0H_TRY_HIP(hipEventElapsedTime(&ms, kv.second.ev[i], kv.second.ev[i + 1]));
      total += ms;
    }
    char item[256];
    snprintf(item, sizeof item, "%s\"%s\": {\"launches\": %zu, \"total_ms\": %.6f, \"alg_bytes\": %.0f}", first ? "" : ", ",
             kv.first.c_str(), kv.second.used / 2, total, kv.second.alg_bytes);
    js += item;
    first = false;
  }
  js += "}";
  R0H_REQUIRE(js.size() + 1 <= capacity, "r0h_kernel_stats: need %zu bytes", js.size() + 1);
  memcpy(json_out, js.c_str(), js.size() + 1);
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_last_profile(r0h_ctx* ctx, const char*** names_out, const float** ms_out, uint32_t* n_out) {
  R0H_REQUIRE(ctx && names_out && ms_out && n_out, "r0h_last_profile: NULL argument");
  const Profile& p = ctx->prof;  // the closed one: a proof in flight, aborted or failed since has not touched it
  *names_out = const_cast<const char**>(p.closed_names.data());
  *ms_out = p.closed_ms.data();
  *n_out = (uint32_t)p.closed_names.size();
  return nullptr;
}

void* r0h_buf_device_ptr(const r0h_buf* buf) { return buf ? buf->ptr : nullptr; }
size_t r0h_buf_bytes(const r0h_buf* buf) { return buf ? buf->bytes : 0; }

}  // extern "C"
