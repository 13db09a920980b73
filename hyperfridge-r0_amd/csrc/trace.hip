// Witness generation of the trace circuit on the device: the executor's compact preflight rows (72 bytes per cycle, 16 per boundary
// row) are uploaded and one thread per trace row expands them into the column-major Montgomery DATA group -- risc0-circuit-rv32im
// 4.0.4's `generate_witness` step (SURVEY.md 3.4 step 2, 8(a) a9, 8(e) "do witgen on device from the compact preflight trace").
// A 2^20-row segment uploads 72 MiB instead of the 576 MiB the expanded group occupies, and the expansion is an HBM-bound stream:
// 72 B read + 138 x 4 B written per row, consecutive lanes own consecutive rows, so every column store is one contiguous 256-byte
// line per wave.  The expansion itself is csrc/trace.hpp, the same code the host reference (r0h_vm_trace_witness) compiles.  The two
// multiplicity columns stay zero here: r0h_logup_multiplicities counts the lookups afterwards (csrc/logup.hip).
#include "trace.hpp"

namespace r0h {

__global__ __launch_bounds__(256) void trace_witgen_kernel(uint32_t* __restrict__ data, const r0h_preflight_row* __restrict__ rows, uint32_t n_rows,
                                                           const r0h_preflight_bound* __restrict__ bounds, uint32_t n_bounds,
                                                           const trace::Tables* __restrict__ tables, uint32_t po2, uint32_t seg_number, uint32_t closing) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x, n = 1u << po2;
  if (r >= n) return;
  uint32_t* cell = data + r;
  // every column of the row is written exactly once: the buffer needs no clearing beforehand.  `put` and `raw` only remember what
  // the expansion sets; the sweep below stores the row, zeros included.
  uint32_t vals[trace::N_COLS];
#pragma unroll
  for (uint32_t c = 0; c < trace::N_COLS; c++) vals[c] = 0;
  auto put = [&](uint32_t col, uint32_t v) { vals[col] = enc(v); };
  auto raw = [&](uint32_t col, uint32_t w) { vals[col] = w; };
  if (r < n_rows) trace::live_row(rows[r], *tables, put, raw);
  else if (r < n_rows + n_bounds) {
    const uint32_t j = r - n_rows;
    trace::bound_row(bounds[j], j ? bounds[j - 1].addr : 0xffffffffu, seg_number, closing != 0, *tables, put, raw);
  } else trace::blank_row(*tables, put, raw);
#pragma unroll
  for (uint32_t c = 0; c < trace::N_COLS; c++) cell[(size_t)c << po2] = vals[c];
}

}  // namespace r0h

using namespace r0h;

// The compact rows of one segment on the device, ready to be expanded: cycles, boundary rows and the expansion's tables in one block
// from the context's pool.  What a session keeps of a segment it evicts (csrc/session.cpp).
struct r0h_trace_rows {
  r0h_ctx* ctx = nullptr;  // retained
  DevBuf block;            // [rows][bounds] padded to 16 bytes, then trace::Tables
  size_t n_rows = 0, n_bounds = 0, row_bytes = 0, tab_off = 0;
  uint32_t po2 = 0, number = 0, closing = 0;
  ~r0h_trace_rows() {
    block.reset();  // (its own reference on the context goes first)
    if (ctx) ctx_release(ctx);
  }
};

namespace {
const char* check_data(const char* who, uint32_t po2, const r0h_buf* data) {
  R0H_REQUIRE(((size_t)R0H_TRACE_COLUMNS << po2) * 4 <= data->bytes, "%s: the DATA buffer holds fewer than %u columns of 2^%u rows", who, (unsigned)R0H_TRACE_COLUMNS, po2);
  return nullptr;
}

// Argument checks, the staging block and the copies into it, the early public inputs.  wait: return only once the copies have landed
// (the caller's arrays may be page-locked, and then nothing else keeps them until the copy has read them).
const char* rows_upload(const char* who, r0h_ctx* ctx, const r0h_preflight_row* rows, size_t n_rows, const r0h_preflight_bound* bounds, size_t n_bounds, uint32_t po2,
                        const r0h_trace_segment* segment, bool wait, std::unique_ptr<r0h_trace_rows>* out, uint32_t* globals_out) {
  R0H_REQUIRE(n_rows + n_bounds >= 1, "%s: a segment has at least one cycle or one boundary row", who);
  R0H_REQUIRE(segment->number >= 1 && segment->number <= 65536, "%s: segment number %u outside [1, 65536]", who, segment->number);
  R0H_REQUIRE(po2 >= R0H_TRACE_MIN_PO2 && po2 <= R0H_TRACE_MAX_PO2, "%s: po2 %u outside [%u, %u] (the lookup tables have 2^16 rows)", who, po2, (unsigned)R0H_TRACE_MIN_PO2,
              (unsigned)R0H_TRACE_MAX_PO2);
  R0H_REQUIRE(n_rows + n_bounds <= ((size_t)1 << po2), "%s: %zu cycles and %zu boundary rows do not fit 2^%u", who, n_rows, n_bounds, po2);
  for (size_t j = 0; j < n_bounds; j += (n_bounds > 4096 ? n_bounds / 4096 : 1))
    R0H_REQUIRE(bounds[j].prev_seg < segment->number && bounds[j].addr < R0H_REG_BASE + 32, "%s: boundary row %zu names segment %u (own: %u) or an address outside memory and registers", who, j,
                bounds[j].prev_seg, segment->number);
  // what the kernel's indexing relies on, checked on the host: cycle numbers are the row numbers, timestamps are in order, a pc is
  // one field element
  for (size_t r = 0; r < n_rows; r += (n_rows > 4096 ? n_rows / 4096 : 1)) {
    R0H_REQUIRE(rows[r].cycle == r, "%s: row %zu carries cycle %u", who, r, rows[r].cycle);
    R0H_REQUIRE(rows[r].pc < P && rows[r].next_pc < P, "%s: pc %#x is not below p: the trace circuit carries a pc as one field element", who, rows[r].pc);
  }
  std::unique_ptr<r0h_trace_rows> h(new r0h_trace_rows());
  h->ctx = ctx;
  ctx_retain(ctx);
  h->n_rows = n_rows;
  h->n_bounds = n_bounds;
  h->row_bytes = n_rows * sizeof(r0h_preflight_row);
  const size_t bound_bytes = n_bounds * sizeof(r0h_preflight_bound);
  h->tab_off = (h->row_bytes + bound_bytes + 15) & ~(size_t)15;
  h->po2 = po2;
  h->number = segment->number;
  h->closing = segment->closing;
  R0H_TRY(h->block.alloc(ctx, h->tab_off + sizeof(trace::Tables)));
  char* base = (char*)h->block->ptr;
  // the caller's arrays are pageable: the copies are stream-ordered but return only once the source has been read
  if (n_rows) R0H_TRY_HIP(hipMemcpyAsync(base, rows, h->row_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (n_bounds) R0H_TRY_HIP(hipMemcpyAsync(base + h->row_bytes, bounds, bound_bytes, hipMemcpyHostToDevice, ctx->stream));
  R0H_TRY(stage_h2d(ctx, base + h->tab_off, &trace::trace_tables(), sizeof(trace::Tables)));
  trace::trace_globals(rows, n_rows, bounds, n_bounds, segment->number, segment->closing != 0, segment->idle_pc, globals_out);
  if (wait) R0H_TRY_HIP(ctx_wait(ctx));
  *out = std::move(h);
  return nullptr;
}

// the launch: one thread per trace row, from the staged block into `data` (checked by the caller)
const char* rows_expand(const r0h_trace_rows* h, r0h_buf* data) {
  const size_t n = (size_t)1 << h->po2;
  const char* base = (const char*)h->block->ptr;
  hipLaunchKernelGGL(trace_witgen_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, h->ctx->stream, u32(data), (const r0h_preflight_row*)base, (uint32_t)h->n_rows,
                     (const r0h_preflight_bound*)(base + h->row_bytes), (uint32_t)h->n_bounds, (const trace::Tables*)(base + h->tab_off), h->po2, h->number, h->closing);
  return launch_ok("trace_witgen_kernel");
}
double expand_bytes(size_t n_rows, size_t n_bounds, uint32_t po2) {
  return (double)n_rows * sizeof(r0h_preflight_row) + (double)n_bounds * sizeof(r0h_preflight_bound) + (double)R0H_TRACE_COLUMNS * ((size_t)1 << po2) * 4;
}
}  // namespace

extern "C" {

const char* r0h_trace_rows_upload(r0h_ctx* ctx, const r0h_preflight_row* rows, size_t n_rows, const r0h_preflight_bound* bounds, size_t n_bounds, uint32_t po2,
                                  const r0h_trace_segment* segment, r0h_trace_rows** rows_out, uint32_t globals_out[R0H_TRACE_GLOBALS]) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && (rows || !n_rows) && (bounds || !n_bounds) && globals_out && segment && rows_out, "r0h_trace_rows_upload: NULL argument");
  KScope ks(ctx, "trace_rows_upload", (double)n_rows * sizeof(r0h_preflight_row) + (double)n_bounds * sizeof(r0h_preflight_bound) + (double)sizeof(trace::Tables));
  std::unique_ptr<r0h_trace_rows> h;
  R0H_TRY(rows_upload("r0h_trace_rows_upload", ctx, rows, n_rows, bounds, n_bounds, po2, segment, true, &h, globals_out));
  *rows_out = h.release();
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_trace_rows_expand(const r0h_trace_rows* h, r0h_buf* data) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(h && data, "r0h_trace_rows_expand: NULL argument");
  R0H_REQUIRE(data->ctx->device == h->ctx->device, "r0h_trace_rows_expand: the DATA buffer is on another device than the rows");
  R0H_TRY(check_data("r0h_trace_rows_expand", h->po2, data));
  KScope ks(h->ctx, "trace_witgen", expand_bytes(h->n_rows, h->n_bounds, h->po2));
  return rows_expand(h, data);
  R0H_GUARD_END
}

}  // extern "C"
const char* r0h::trace_rows_upload_enqueue(r0h_ctx* ctx, const r0h_preflight_row* rows, size_t n_rows, const r0h_preflight_bound* bounds, size_t n_bounds, uint32_t po2,
                                           const r0h_trace_segment* segment, r0h_trace_rows** rows_out, uint32_t* globals_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && (rows || !n_rows) && (bounds || !n_bounds) && globals_out && segment && rows_out, "r0h_trace_rows_upload: NULL argument");
  KScope ks(ctx, "trace_rows_upload", (double)n_rows * sizeof(r0h_preflight_row) + (double)n_bounds * sizeof(r0h_preflight_bound) + (double)sizeof(trace::Tables));
  std::unique_ptr<r0h_trace_rows> h;
  R0H_TRY(rows_upload("r0h_trace_rows_upload", ctx, rows, n_rows, bounds, n_bounds, po2, segment, false, &h, globals_out));
  *rows_out = h.release();
  return nullptr;
  R0H_GUARD_END
}
extern "C" {
size_t r0h_trace_rows_bytes(const r0h_trace_rows* h) { return h ? h->block->bytes : 0; }

const char* r0h_trace_rows_free(r0h_trace_rows* h) {
  delete h;
  return nullptr;
}

// upload + expand + free: one wait, after the launch
const char* r0h_trace_witgen(r0h_ctx* ctx, const r0h_preflight_row* rows, size_t n_rows, const r0h_preflight_bound* bounds, size_t n_bounds,
                             uint32_t po2, const r0h_trace_segment* segment, r0h_buf* data, uint32_t globals_out[R0H_TRACE_GLOBALS]) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && (rows || !n_rows) && data && (bounds || !n_bounds) && globals_out && segment, "r0h_trace_witgen: NULL argument");
  if (po2 <= R0H_TRACE_MAX_PO2) R0H_TRY(check_data("r0h_trace_witgen", po2, data));  // (a po2 out of range is rows_upload's to name)
  KScope ks(ctx, "trace_witgen", expand_bytes(n_rows, n_bounds, po2 <= R0H_TRACE_MAX_PO2 ? po2 : 0));
  std::unique_ptr<r0h_trace_rows> h;
  R0H_TRY(rows_upload("r0h_trace_witgen", ctx, rows, n_rows, bounds, n_bounds, po2, segment, false, &h, globals_out));
  R0H_TRY(rows_expand(h.get(), data));
  R0H_TRY_HIP(ctx_wait(ctx));  // the staging block goes back to the pool and the caller may free its rows
  return nullptr;
  R0H_GUARD_END
}

}  // extern "C"
