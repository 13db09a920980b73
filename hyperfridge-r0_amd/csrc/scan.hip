// Extension-field scans of the prover for gfx950: running sums, running products and synthetic division, one chunked scan under
// three operations.  Replaces risc0-zkp 3.0.4 hal `prefix_products` and core/poly.rs `poly_divide` (which upstream runs on the
// host) -- SURVEY.md 8(a) a10; the running sums are the additive counterpart a log-derivative argument needs.
// A scan of n = 2^k packed elements is cut into chunks of `threads * E` (ScanGeom) and takes three launches:
//   scan_summary_kernel  per chunk: a thread joins its E elements, the block reduces, one summary per (job, chunk);
//   scan_link_kernel     one block per job: exclusive scan of the job's chunk summaries in place, the total into slot n_chunks;
//   scan_apply_kernel    per chunk: a scan across the block's threads, the carry in from the linked summary, serial write-back.
// A job is one scan; the kernels take a batch of jobs on blockIdx.y (link: blockIdx.x).
#include <map>

#include "internal.hpp"

namespace r0h {

__device__ __forceinline__ Fp4 ld4(const uint32_t* p) {
  uint4 v = *(const uint4*)p;
  return Fp4{{v.x, v.y, v.z, v.w}};
}
__device__ __forceinline__ void st4(uint32_t* p, const Fp4& v) { *(uint4*)p = make_uint4(v.e[0], v.e[1], v.e[2], v.e[3]); }

struct ScanGeom {
  uint32_t threads, E, chunk, n_chunks;
};
static ScanGeom scan_geom(uint32_t n) {
  ScanGeom g;
  g.threads = n < 256 ? n : 256;
  g.chunk = n < 4096 ? n : 4096;
  g.E = g.chunk / g.threads;
  g.n_chunks = n / g.chunk;
  return g;
}

// ------------------------------------------------------------------ the operations
// An operation joins the summary of a run of elements with the summary of the run that follows it: join(earlier, later, weight of
// the later run's length).  It names its identity, whether scan position i is element i or element n - 1 - i, whether element
// i receives the scan up to and including itself or up to the element before, and whether join(a, b) = join(b, a).  Job: the weights of one element, of one thread's
// E elements and of one chunk, the polynomial scanned (index into a buffer of n-element polynomials) and the slot of its summaries.
struct NoWeight {};  // sums and products weigh nothing: the powers the kernels take of it compile away
R0H_HD NoWeight operator*(NoWeight, NoWeight) { return {}; }
R0H_HD NoWeight fp4_pow(NoWeight, uint64_t) { return {}; }
struct Unweighted {  // io[i] = io[0] (+ or *) ... (+ or *) io[i]; one job per launch and nothing to upload: poly = slot = the job's index
  struct Job {
    NoWeight w, wE, wChunk;
    uint32_t poly, slot;
  };
  static constexpr bool REVERSED = false, INCLUSIVE = true, COMMUTES = true;
  static __device__ Job job(const Job*, uint32_t j) { return Job{{}, {}, {}, j, j}; }
};
struct SumOp : Unweighted {
  static __device__ Fp4 id() { return fp4_zero(); }
  static __device__ Fp4 join(const Fp4& a, const Fp4& b, NoWeight) { return a + b; }
};
struct ProductOp : Unweighted {
  static __device__ Fp4 id() { return fp4_one(); }
  static __device__ Fp4 join(const Fp4& a, const Fp4& b, NoWeight) { return a * b; }
};
// Synthetic division by (x - z): q[i] = sum_{j>i} p[j] z^(j-i-1), remainder = sum_j p[j] z^j.  Horner's rule from the top
// coefficient down is a scan in reversed order whose summary of a run is its value at z: q[i] is the scan before p[i], the
// remainder is the total.  w = z, wE = z^E, wChunk = z^chunk, computed on the host.
struct DivJob {
  Fp4 w, wE, wChunk;
  uint32_t poly, slot, pad0, pad1;
};
struct HornerOp {
  typedef DivJob Job;
  static constexpr bool REVERSED = true, INCLUSIVE = false, COMMUTES = false;
  static __device__ Job job(const Job* __restrict__ jobs, uint32_t j) { return jobs[j]; }
  static __device__ Fp4 id() { return fp4_zero(); }
  static __device__ Fp4 join(const Fp4& a, const Fp4& b, const Fp4& w) { return a * w + b; }
};

// ------------------------------------------------------------------ the three kernels
// scan position i of thread t in chunk blockIdx.x is at first + i * stride words
template <class Op>
__device__ __forceinline__ uint32_t* scan_first(uint32_t* polys, uint32_t poly, uint32_t E, uint32_t n) {
  const size_t at = (size_t)blockIdx.x * blockDim.x * E + (size_t)threadIdx.x * E;
  return polys + 4 * ((size_t)poly * n + (Op::REVERSED ? n - 1 - at : at));
}
template <class Op> constexpr int scan_stride() { return Op::REVERSED ? -4 : 4; }

template <class Op>
__global__ void scan_summary_kernel(uint32_t* __restrict__ sums, const uint32_t* __restrict__ polys, const typename Op::Job* __restrict__ jobs, uint32_t E,
                                    uint32_t n, uint32_t n_chunks) {
  extern __shared__ uint32_t sh[];
  const uint32_t t = threadIdx.x, nt = blockDim.x;
  const typename Op::Job job = Op::job(jobs, blockIdx.y);
  const uint32_t* p = scan_first<Op>((uint32_t*)polys, job.poly, E, n);
  Fp4 v = Op::id();
  for (uint32_t k = 0; k < E; k++) v = Op::join(v, ld4(p + (int)k * scan_stride<Op>()), job.w);
  st4(sh + 4 * t, v);
  __syncthreads();
  // Pairs of neighbouring runs in scan order, s threads each.  An operation that commutes takes the thread `far` above instead: the
  // active threads stay together (idle waves retire, LDS accesses stay dense) -- 0.5-1 us per launch of the sums' kernel at 2^20.
  auto step = job.wE;  // weight of the run on the right of a pair
  for (uint32_t s = 1, far = nt / 2; s < nt; s <<= 1, far >>= 1) {
    const uint32_t d = Op::COMMUTES ? far : s;
    if (Op::COMMUTES ? t < far : (t & (2 * s - 1)) == 0) st4(sh + 4 * t, Op::join(ld4(sh + 4 * t), ld4(sh + 4 * (t + d)), step));
    step = step * step;
    __syncthreads();
  }
  if (t == 0) st4(sums + 4 * ((size_t)job.slot * (n_chunks + 1) + blockIdx.x), ld4(sh));
}
// One block: each thread owns `per` consecutive chunks (none, past the last chunk: those threads hold the identity and come last in
// scan order, so nothing joins them from the left of a thread that counts), Hillis-Steele across the threads.
template <class Op>
__global__ __launch_bounds__(256) void scan_link_kernel(uint32_t* sums, const typename Op::Job* __restrict__ jobs, uint32_t n_chunks) {
  __shared__ uint32_t sh[256 * 4];
  const typename Op::Job job = Op::job(jobs, blockIdx.x);
  uint32_t* sum = sums + 4 * (size_t)job.slot * (n_chunks + 1);
  const uint32_t t = threadIdx.x, per = (n_chunks + 255) / 256, b0 = t * per;
  Fp4 v = Op::id();
  for (uint32_t k = 0; k < per && b0 + k < n_chunks; k++) v = Op::join(v, ld4(sum + 4 * (size_t)(b0 + k)), job.wChunk);
  st4(sh + 4 * t, v);
  __syncthreads();
  auto step = fp4_pow(job.wChunk, per);
  for (uint32_t s = 1; s < 256; s <<= 1) {  // inclusive scan over threads
    Fp4 o = t >= s ? ld4(sh + 4 * (t - s)) : Op::id();
    __syncthreads();
    if (t >= s) st4(sh + 4 * t, Op::join(o, ld4(sh + 4 * t), step));
    step = step * step;
    __syncthreads();
  }
  if (t == (n_chunks < 256 ? n_chunks : 256) - 1) st4(sum + 4 * (size_t)n_chunks, ld4(sh + 4 * t));  // the total, at the last thread with chunks
  Fp4 cur = t ? ld4(sh + 4 * (t - 1)) : Op::id();
  for (uint32_t k = 0; k < per && b0 + k < n_chunks; k++) {
    Fp4 x = ld4(sum + 4 * (size_t)(b0 + k));
    st4(sum + 4 * (size_t)(b0 + k), cur);
    cur = Op::join(cur, x, job.wChunk);
  }
}
template <class Op>
__global__ void scan_apply_kernel(uint32_t* __restrict__ polys, const uint32_t* __restrict__ sums, const typename Op::Job* __restrict__ jobs, uint32_t E, uint32_t n,
                                  uint32_t n_chunks) {
  extern __shared__ uint32_t sh[];
  const uint32_t t = threadIdx.x, nt = blockDim.x;
  const typename Op::Job job = Op::job(jobs, blockIdx.y);
  uint32_t* p = scan_first<Op>(polys, job.poly, E, n);
  Fp4 v = Op::id();
  for (uint32_t k = 0; k < E; k++) v = Op::join(v, ld4(p + (int)k * scan_stride<Op>()), job.w);
  st4(sh + 4 * t, v);
  __syncthreads();
  auto step = job.wE;
  for (uint32_t s = 1; s < nt; s <<= 1) {  // inclusive scan over threads
    Fp4 o = t >= s ? ld4(sh + 4 * (t - s)) : Op::id();
    __syncthreads();
    if (t >= s) st4(sh + 4 * t, Op::join(o, ld4(sh + 4 * t), step));
    step = step * step;
    __syncthreads();
  }
  // what precedes this thread's elements: the chunks before the block, then the threads before it (t * E elements)
  Fp4 cur = ld4(sums + 4 * ((size_t)job.slot * (n_chunks + 1) + blockIdx.x));
  if (t > 0) cur = Op::join(cur, ld4(sh + 4 * (t - 1)), fp4_pow(job.wE, t));
  for (uint32_t k = 0; k < E; k++) {
    uint32_t* q = p + (int)k * scan_stride<Op>();
    const Fp4 next = Op::join(cur, ld4(q), job.w);
    st4(q, Op::INCLUSIVE ? next : cur);
    cur = next;
  }
}

// what a scan leaves, n = 2^po2 packed extension elements, as the four columns of 2^po2 words an ACCUM accumulator is stored in
__global__ void ext_unpack_kernel(uint32_t* __restrict__ cols, const uint32_t* __restrict__ packed, uint32_t po2) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= (1u << po2)) return;
  const uint4 v = *(const uint4*)(packed + 4 * (size_t)r);
  cols[r] = v.x; cols[((size_t)1 << po2) + r] = v.y; cols[((size_t)2 << po2) + r] = v.z; cols[((size_t)3 << po2) + r] = v.w;
}

// remainders of a batch, packed: out[job] = sums[slot(job)][n_chunks]
__global__ void divide_remainders_kernel(uint32_t* __restrict__ out, const uint32_t* __restrict__ sums, uint32_t n_jobs, uint32_t n_chunks) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n_jobs) st4(out + 4 * (size_t)j, ld4(sums + 4 * ((size_t)j * (n_chunks + 1) + n_chunks)));
}

// The job table's weights filled on the device: job j divides by (x - points[pad0 of job j]), a point the device's transcript made
// (poly_divide_batch_points).  A lane per job: w, w^E, w^chunk by square-and-multiply.
__global__ __launch_bounds__(64) void divide_jobs_kernel(DivJob* __restrict__ jobs, const uint32_t* __restrict__ points, uint32_t E, uint32_t chunk, uint32_t n_jobs) {
  const uint32_t j = blockIdx.x * 64 + threadIdx.x;
  if (j >= n_jobs) return;
  const uint32_t* pt = points + 4 * (size_t)jobs[j].pad0;
  const Fp4 w{{pt[0], pt[1], pt[2], pt[3]}};
  jobs[j].w = w;
  jobs[j].wE = fp4_pow(w, E);
  jobs[j].wChunk = fp4_pow(w, chunk);
}
// report[0] = 0, or 1 + the lowest job whose remainder (divide_remainders_kernel's packed output) is not zero.  One wave.
__global__ __launch_bounds__(64) void divide_report_kernel(uint32_t* __restrict__ report, const uint32_t* __restrict__ rem, uint32_t n_jobs) {
  uint32_t first = 0xffffffffu;
  for (uint32_t j = threadIdx.x; j < n_jobs; j += 64) {
    const Fp4 r = ld4(rem + 4 * (size_t)j);
    if ((r.e[0] | r.e[1] | r.e[2] | r.e[3]) && j < first) first = j;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint32_t o = __shfl_xor(first, off);
    first = o < first ? o : first;
  }
  if (threadIdx.x == 0) report[0] = first == 0xffffffffu ? 0u : first + 1;
}

}  // namespace r0h

using namespace r0h;

// One job and no job table.  (r0h_accum and the log-derivative accumulators scan one accumulator per call; the job axis would take
// them side by side.)
template <class Op>
static const char* prefix_scan(r0h_ctx* ctx, r0h_buf* io, uint32_t n, const char* what) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && io, "%s: NULL argument", what);
  R0H_REQUIRE(n && (n & (n - 1)) == 0, "%s: n %u is not a power of two", what, n);
  R0H_REQUIRE((size_t)n * 16 <= io->bytes, "%s: n %u exceeds the buffer", what, n);
  const ScanGeom g = scan_geom(n);
  DevBuf sums;
  R0H_TRY(sums.alloc(ctx, (size_t)(g.n_chunks + 1) * 16));
  hipLaunchKernelGGL(scan_summary_kernel<Op>, dim3(g.n_chunks), dim3(g.threads), g.threads * 16, ctx->stream, u32(sums.get()), u32(io), nullptr, g.E, n, g.n_chunks);
  hipLaunchKernelGGL(scan_link_kernel<Op>, dim3(1), dim3(256), 0, ctx->stream, u32(sums.get()), nullptr, g.n_chunks);
  hipLaunchKernelGGL(scan_apply_kernel<Op>, dim3(g.n_chunks), dim3(g.threads), g.threads * 16, ctx->stream, u32(io), u32(sums.get()), nullptr, g.E, n, g.n_chunks);
  return launch_ok(what);
  R0H_GUARD_END
}

extern "C" {

const char* r0h_prefix_products(r0h_ctx* ctx, r0h_buf* io, uint32_t n) { return prefix_scan<ProductOp>(ctx, io, n, "r0h_prefix_products"); }
// the additive counterpart (the running sums of a log-derivative argument): io[i] = sum_{j <= i} io[j] over extension elements
const char* r0h_prefix_sums(r0h_ctx* ctx, r0h_buf* io, uint32_t n) { return prefix_scan<SumOp>(ctx, io, n, "r0h_prefix_sums"); }

const char* r0h_poly_divide(r0h_ctx* ctx, r0h_buf* poly, uint32_t n, const uint32_t z[4], uint32_t remainder[4]) {
  R0H_REQUIRE(ctx && poly && z, "r0h_poly_divide: NULL argument");
  R0H_REQUIRE(z[0] < P && z[1] < P && z[2] < P && z[3] < P, "r0h_poly_divide: z words must be canonical (< p)");
  R0H_REQUIRE(n && (n & (n - 1)) == 0, "r0h_poly_divide: n %u is not a power of two", n);
  R0H_REQUIRE((size_t)n * 16 <= poly->bytes, "r0h_poly_divide: n %u exceeds the buffer", n);
  const uint32_t idx = 0;
  return r0h::poly_divide_batch(ctx, poly, n, &idx, z, 1, remainder);
}

}  // extern "C"

namespace r0h {
const char* unpack_ext_columns(r0h_ctx* ctx, uint32_t* cols, const uint32_t* packed, uint32_t po2) {
  const uint32_t n = 1u << po2, threads = n < 256 ? n : 256;
  hipLaunchKernelGGL(ext_unpack_kernel, dim3(n / threads), dim3(threads), 0, ctx->stream, cols, packed, po2);
  return launch_ok("ext_unpack_kernel");
}

// polys: a buffer of n-coefficient extension polynomials (AoS, natural order); job j divides polynomial poly_idx[j] in place by
// (x - points[4j..4j+4)).  Jobs on the same polynomial are applied in the order given.  remainders_host (4 words per job, may be
// NULL) is filled by ONE blocking copy after everything has been enqueued.  The DEEP step divides ~10 combos by one to three points
// each: one launch set per "k-th point of every combo" instead of one per (combo, point).
// points: four host words per job (poly_divide_batch), or nullptr with the job's point named by pt_idx[j] in the device table d_points and
// the verdict left in the device word d_report instead of a read-back (poly_divide_batch_points)
static const char* poly_divide_batch_impl(r0h_ctx* ctx, r0h_buf* polys, uint32_t n, const uint32_t* poly_idx, const uint32_t* points, const uint32_t* pt_idx,
                                          const uint32_t* d_points, uint32_t n_points, uint32_t n_jobs, uint32_t* remainders_host, uint32_t* d_report) {
  R0H_GUARD_BEGIN
  if (!n_jobs) {
    if (d_report) R0H_TRY_HIP(hipMemsetAsync(d_report, 0, 4, ctx->stream));
    return nullptr;
  }
  const ScanGeom g = scan_geom(n);
  const size_t n_polys = polys->bytes / ((size_t)n * 16);
  // pass k holds the k-th job of every polynomial: within a pass the jobs touch different polynomials and run side by side
  std::vector<std::vector<uint32_t>> passes;
  {
    std::map<uint32_t, uint32_t> seen;
    for (uint32_t j = 0; j < n_jobs; j++) {
      R0H_REQUIRE(poly_idx[j] < n_polys, "poly_divide: polynomial %u outside a buffer of %zu", poly_idx[j], n_polys);
      const uint32_t k = seen[poly_idx[j]]++;
      if (passes.size() <= k) passes.emplace_back();
      passes[k].push_back(j);
    }
  }
  std::vector<DivJob> jobs;  // in launch order; slot = the job's index as given (remainders come back in the caller's order)
  for (const auto& pass : passes)
    for (uint32_t j : pass) {
      DivJob d;
      d.poly = poly_idx[j]; d.slot = j; d.pad0 = d.pad1 = 0;
      if (points) {
        d.w = Fp4{{points[4 * (size_t)j], points[4 * (size_t)j + 1], points[4 * (size_t)j + 2], points[4 * (size_t)j + 3]}};
        d.wE = fp4_pow(d.w, g.E);
        d.wChunk = fp4_pow(d.w, g.chunk);
      } else {
        R0H_REQUIRE(pt_idx[j] < n_points, "poly_divide: job %u names point %u of a table of %u", j, pt_idx[j], n_points);
        d.w = d.wE = d.wChunk = fp4_zero();  // divide_jobs_kernel's
        d.pad0 = pt_idx[j];
      }
      jobs.push_back(d);
    }
  const size_t sum_bytes = (size_t)n_jobs * (g.n_chunks + 1) * 16, job_bytes = jobs.size() * sizeof(DivJob), rem_bytes = (size_t)n_jobs * 16;
  DevBuf tmp;  // [summaries][jobs][remainders]
  R0H_TRY(tmp.alloc(ctx, sum_bytes + job_bytes + rem_bytes));
  uint32_t* sums = u32(tmp.get());
  DivJob* d_jobs = (DivJob*)((char*)tmp->ptr + sum_bytes);
  uint32_t* d_rem = (uint32_t*)((char*)tmp->ptr + sum_bytes + job_bytes);
  R0H_TRY(stage_h2d(ctx, d_jobs, jobs.data(), job_bytes));
  if (!points) {
    KScope kj(ctx, "divide_jobs_kernel", (double)job_bytes);
    hipLaunchKernelGGL(divide_jobs_kernel, dim3((n_jobs + 63) / 64), dim3(64), 0, ctx->stream, d_jobs, d_points, g.E, g.chunk, n_jobs);
    R0H_TRY(launch_ok("divide_jobs_kernel"));
  }
  KScope ks(ctx, "poly_divide", 48.0 * n * n_jobs);
  size_t first = 0;
  for (const auto& pass : passes) {
    const uint32_t nj = (uint32_t)pass.size();
    hipLaunchKernelGGL(scan_summary_kernel<HornerOp>, dim3(g.n_chunks, nj), dim3(g.threads), g.threads * 16, ctx->stream, sums, u32(polys), d_jobs + first, g.E, n, g.n_chunks);
    hipLaunchKernelGGL(scan_link_kernel<HornerOp>, dim3(nj), dim3(256), 0, ctx->stream, sums, d_jobs + first, g.n_chunks);
    hipLaunchKernelGGL(scan_apply_kernel<HornerOp>, dim3(g.n_chunks, nj), dim3(g.threads), g.threads * 16, ctx->stream, u32(polys), sums, d_jobs + first, g.E, n, g.n_chunks);
    first += nj;
  }
  R0H_TRY(launch_ok("poly_divide kernels"));
  if (remainders_host || d_report) {
    hipLaunchKernelGGL(divide_remainders_kernel, dim3((n_jobs + 63) / 64), dim3(64), 0, ctx->stream, d_rem, sums, n_jobs, g.n_chunks);
    R0H_TRY(launch_ok("divide_remainders_kernel"));
  }
  if (remainders_host) {
    R0H_TRY_HIP(hipMemcpyAsync(remainders_host, d_rem, rem_bytes, hipMemcpyDeviceToHost, ctx->stream));
    R0H_TRY_HIP(ctx_wait(ctx));
  }
  if (d_report) {  // the remainders stay on the device: reduced to one word the caller reads back when it likes
    KScope kr(ctx, "divide_report_kernel", (double)rem_bytes);
    hipLaunchKernelGGL(divide_report_kernel, dim3(1), dim3(64), 0, ctx->stream, d_report, d_rem, n_jobs);
    R0H_TRY(launch_ok("divide_report_kernel"));
  }
  return nullptr;
  R0H_GUARD_END
}
const char* poly_divide_batch(r0h_ctx* ctx, r0h_buf* polys, uint32_t n, const uint32_t* poly_idx, const uint32_t* points, uint32_t n_jobs, uint32_t* remainders_host) {
  return poly_divide_batch_impl(ctx, polys, n, poly_idx, points, nullptr, nullptr, 0, n_jobs, remainders_host, nullptr);
}
const char* poly_divide_batch_points(r0h_ctx* ctx, r0h_buf* polys, uint32_t n, const uint32_t* poly_idx, const uint32_t* pt_idx, uint32_t n_jobs, const uint32_t* d_points,
                                     uint32_t n_points, uint32_t* d_report) {
  R0H_REQUIRE(ctx && polys && d_report && (!n_jobs || (poly_idx && pt_idx && d_points)), "poly_divide: NULL argument");
  return poly_divide_batch_impl(ctx, polys, n, poly_idx, nullptr, pt_idx, d_points, n_points, n_jobs, nullptr, d_report);
}
}  // namespace r0h

extern "C" {

const char* r0h_poly_divide_batch(r0h_ctx* ctx, r0h_buf* polys, uint32_t n, const uint32_t* poly_idx, const uint32_t* points, uint32_t n_jobs, uint32_t* remainders_out) {
  R0H_REQUIRE(ctx && polys && (!n_jobs || (poly_idx && points)), "r0h_poly_divide_batch: NULL argument");
  R0H_REQUIRE(n && (n & (n - 1)) == 0, "r0h_poly_divide_batch: n %u is not a power of two", n);
  for (size_t k = 0; k < 4 * (size_t)n_jobs; k++) R0H_REQUIRE(points[k] < P, "r0h_poly_divide_batch: the point of job %zu is not canonical (< p)", k / 4);
  return r0h::poly_divide_batch(ctx, polys, n, poly_idx, points, n_jobs, remainders_out);
}

const char* r0h_poly_divide_batch_points(r0h_ctx* ctx, r0h_buf* polys, uint32_t n, const uint32_t* poly_idx, const uint32_t* pt_idx, uint32_t n_jobs, const r0h_buf* points_buf,
                                         size_t points_word_offset, uint32_t n_points, r0h_buf* report_buf, size_t report_word_offset) {
  R0H_REQUIRE(ctx && polys && points_buf && report_buf && (!n_jobs || (poly_idx && pt_idx)), "r0h_poly_divide_batch_points: NULL argument");
  R0H_REQUIRE(n && (n & (n - 1)) == 0, "r0h_poly_divide_batch_points: n %u is not a power of two", n);
  R0H_TRY(require_words_in("r0h_poly_divide_batch_points", "point table", points_buf, points_word_offset, 4 * (size_t)n_points));
  R0H_TRY(require_words_in("r0h_poly_divide_batch_points", "report word", report_buf, report_word_offset, 1));
  return r0h::poly_divide_batch_points(ctx, polys, n, poly_idx, pt_idx, n_jobs, u32(points_buf) + points_word_offset, n_points, u32(report_buf) + report_word_offset);
}

}  // extern "C"
