// Batched BabyBear NTTs for gfx950: register-blocked radix-16 butterflies, one to three HBM passes.
// Replaces risc0-zkp 3.0.4 hal `batch_interpolate_ntt` / `batch_expand_into_evaluate_ntt` / `batch_bit_reverse` /
// `zk_shift` (core/ntt.rs; CUDA side in risc0-sys 1.5.0) -- SURVEY.md 8(a) a2-a5.
//
// Decomposition (N = 2^n = N0 * N1 * N2; N2 = 2^L contiguous, N1 = 2^H strided, N0 = 2^outer = 16 or 1: split16_for):
//   forward  (bit-reversed coeffs -> natural evals, DIT):  local size-2^L DITs on contiguous chunks (ntt_local16_kernel), then for
//            every residue lo a size-2^H DIT over the chunk index with the inter-pass twiddle w^(brev_H(hi) * lo) on load
//            (ntt_strided16_kernel), then one radix-16 butterfly over the top four index bits (ntt_outer16_kernel);
//   inverse  (natural evals -> bit-reversed coeffs, DIF):  the transpose: outer, strided (twiddle on store), then local DIFs with
//            the 1/N normalisation -- and on request the coset shift f(x) -> f(3x) -- folded into the final store.
// Every thread keeps sixteen words in VGPRs and runs four butterfly layers on them per round; the rounds of a pass exchange through
// LDS.  Column-major batches map to blockIdx.y.  Transforms below 2^8 points, and the contiguous pass of an expansion other than
// x1 or x4, go through one small radix-2 kernel (ntt_local_kernel).
#include <algorithm>

#include "internal.hpp"

namespace r0h {

struct TwTables {
  const uint32_t* lo;    // w22^i            (w26^i for the BIG kernels)
  const uint32_t* hi;    // w22^(i << 11)    (w26^(i << 13))
  const uint32_t* tw12;  // ROU[TWL_BITS]^i, i < 2^(TWL_BITS - 1): the twiddles of every layer inside a contiguous chunk
};

// w_n^e from a two-level table: powers of ROU[22] (2 x 2^11 words) for n <= 22; BIG: powers of ROU[26] (2 x 2^13 words) for
// the outer pass of larger transforms (the host hands over the matching table pair)
template <int BIG = 0>
__device__ __forceinline__ uint32_t omega_n(const TwTables& t, uint32_t e, uint32_t n) {
  if (BIG) {
    const uint32_t E = e << (MAX_DOMAIN_PO2 - n);
    return mul(t.lo[E & (TWB_SIZE - 1)], t.hi[E >> TWB_BITS]);
  }
  const uint32_t E = e << (TW_TOP - n);
  return mul(t.lo[E & (TW_SIZE - 1)], t.hi[E >> TW_BITS]);
}

// One contiguous chunk of 2^L words per block, radix-2 in LDS: whole transforms below 2^8 points, and the contiguous pass of a forward
// transform whose expand_bits the radix-16 kernel has no instantiation for.  DIR 0: DIT layers (expand_bits, L]; DIR 1: DIF layers L..1.
template <int DIR>
__global__ __launch_bounds__(256) void ntt_local_kernel(uint32_t* out, const uint32_t* in /* may alias out */,
                                                         uint32_t L, uint32_t n_out, uint32_t expand_bits,
                                                         const uint32_t* __restrict__ tw12, uint32_t scale) {
  extern __shared__ uint32_t s[];
  const uint32_t size = 1u << L, tid = threadIdx.x;
  const size_t col = blockIdx.y;
  const uint32_t* src = in + (col << (n_out - expand_bits));
  uint32_t* dst = out + (col << n_out);
  const uint32_t base = blockIdx.x << L;
  for (uint32_t i = tid; i < size; i += 256) s[i] = src[(base + i) >> expand_bits];
  __syncthreads();
  if (DIR == 0) {
    for (uint32_t l = expand_bits + 1; l <= L; l++) {
      const uint32_t half = 1u << (l - 1);
      for (uint32_t b = tid; b < size / 2; b += 256) {
        uint32_t j = b & (half - 1), i0 = ((b >> (l - 1)) << l) + j;
        uint32_t a = s[i0], t = mul(s[i0 + half], tw12[j << (TWL_BITS - l)]);
        s[i0] = add(a, t);
        s[i0 + half] = sub(a, t);
      }
      __syncthreads();
    }
  } else {
    for (uint32_t l = L; l >= 1; l--) {
      const uint32_t half = 1u << (l - 1);
      for (uint32_t b = tid; b < size / 2; b += 256) {
        uint32_t j = b & (half - 1), i0 = ((b >> (l - 1)) << l) + j;
        uint32_t a = s[i0], t = s[i0 + half];
        s[i0] = add(a, t);
        s[i0 + half] = mul(sub(a, t), tw12[j << (TWL_BITS - l)]);
      }
      __syncthreads();
    }
  }
  if (DIR == 1) {
    for (uint32_t i = tid; i < size; i += 256) dst[base + i] = mul(s[i], scale);
  } else {
    for (uint32_t i = tid; i < size; i += 256) dst[base + i] = s[i];
  }
}

// ------------------------------------------------------------------ radix-16 register-blocked kernels
// Sub-transforms of size 2^m (8 <= m <= 13) are done in rounds of four butterfly layers: every thread keeps 16 words
// in VGPRs, runs the layers of one 4-bit index field on them, and the block exchanges through LDS between rounds
// (2 LDS writes + 2 LDS reads per word per pass instead of 2 per layer).  Twiddles of a round are
// ROU[l]^(low bits) -- one table word per layer and thread -- times a constant 16th root of unity.
struct W16 {
  uint32_t w[8];  // ROU[4]^k, k < 8 (forward or inverse)
};

// Layers of the field at bit B (width W) on 16 >> W independent sets; DIT when DIR == 0 (skipping layers below
// LO_LAYER), DIF when DIR == 1.  rest0 = index of the thread's first set among the 2^(m-W) sets of the sub-transform.
template <int W, int B, int DIR, int LO_LAYER>
__device__ __forceinline__ void field_layers(uint32_t (&x)[16], uint32_t rest0, const uint32_t* __restrict__ tw12, const W16& c) {
  constexpr int SETS = 16 >> W;
#pragma unroll
  for (int s = 0; s < SETS; s++) {
    const uint32_t low = (rest0 + s) & ((1u << B) - 1u);
#pragma unroll
    for (int step = 0; step < W; step++) {
      const int l = DIR == 0 ? step : W - 1 - step;
      if (DIR == 0 && l < LO_LAYER) continue;
      uint32_t a_tw = ONE;
      if (B != 0) a_tw = tw12[low << (TWL_BITS - (B + l + 1))];
#pragma unroll
      for (int j0 = 0; j0 < (1 << W); j0++) {
        if (j0 & (1 << l)) continue;
        const int j1 = j0 | (1 << l), cidx = (j0 & ((1 << l) - 1)) << (3 - l);
        uint32_t& u = x[s * (1 << W) + j0];
        uint32_t& v = x[s * (1 << W) + j1];
        const bool trivial = B == 0 && cidx == 0;
        uint32_t twd = cidx == 0 ? a_tw : (B == 0 ? c.w[cidx] : mul_lazy(a_tw, c.w[cidx]));  // < 2p is fine as a multiplier
        if (DIR == 0) {
          uint32_t a = u, t = trivial ? v : mul(v, twd);
          u = add(a, t);
          v = sub(a, t);
        } else {
          uint32_t a = u, t = v;
          u = add(a, t);
          v = trivial ? sub(a, t) : mul(sub(a, t), twd);
        }
      }
    }
  }
}

// element index of word (set s, digit j) for the field at bit B of width W, thread's first set rest0
template <int W, int B>
__device__ __forceinline__ uint32_t field_index(uint32_t rest0, int s, int j) {
  uint32_t r = rest0 + s;
  return ((r >> B) << (B + W)) | ((uint32_t)j << B) | (r & ((1u << B) - 1u));
}

// The sixteen words of thread q in the layout of the field <W, B> -- the thread's first set is q * (16 >> W), as for field_layers:
// f(element index, register slot) for each of them
template <int W, int B, class F>
__device__ __forceinline__ void field_walk(uint32_t q, F&& f) {
  constexpr int SETS = 16 >> W;
#pragma unroll
  for (int s = 0; s < SETS; s++)
#pragma unroll
    for (int j = 0; j < (1 << W); j++) f(field_index<W, B>(q * SETS, s, j), s * (1 << W) + j);
}

// Inter-pass twiddles of one thread: element e = q*16 + j needs w_n^(brev_H(e) * lo) with
// brev_H(e) = brev_4(j) << (H-4) | brev_{H-4}(q), i.e. base * g^brev_4(j) with base = w_n^(brev(q) * lo), g = w_n^(lo << (H-4)):
// four table words and 29 products per 16 elements instead of 32 table words and 16 products.
template <uint32_t H, int BIG>
__device__ __forceinline__ void interpass_twiddles(uint32_t (&t)[16], const TwTables& tw, uint32_t q, uint32_t lo, uint32_t n) {
  const uint32_t base = omega_n<BIG>(tw, bitrev(q, H - 4) * lo, n), g = omega_n<BIG>(tw, lo << (H - 4), n);
  uint32_t gp[16];  // base * g^k
  gp[0] = base;
#pragma unroll
  for (int k = 1; k < 16; k++) gp[k] = mul_lazy(gp[k - 1], g);  // multipliers may stay below 2p (g < p keeps the bound)
#pragma unroll
  for (int j = 0; j < 16; j++) t[j] = gp[((j & 1) << 3) | ((j & 2) << 1) | ((j & 4) >> 1) | ((j & 8) >> 3)];
}

// [2^H][32] tile, H = 8 + WL, 32 consecutive residues: forward = DIT over the chunk index with the inter-pass twiddle on load,
// inverse = DIF with the twiddle on store.  Block = 16 << (H - 4) threads; a thread owns two adjacent residues (one radix-16
// column each), so every global access is a 128-byte row: 4.8 TB/s against 3.2 TB/s for 64-byte rows in a plain copy of the same
// shape (tools/microbench/tile_copy_bench.hip) -- the rows always hold that much, since a strided pass runs over chunks of at least
// 2^8 words (split16_for).  The tile has to stay small enough for two blocks per CU (load, butterflies and store of different
// blocks overlap): H <= 9, i.e. the contiguous pass takes up to 2^13 words.  LDS rows are padded by two words so that the four row
// groups of a wave fall into different banks.
// BIG: the rows are 2^L <= 2^18 words apart and the transform has more than 2^22 points (third level, see the host side).
template <int WL, int DIR, int BIG = 0>
__global__ __launch_bounds__(16 << (4 + WL)) void ntt_strided16_kernel(uint32_t* io, const uint32_t* in, uint32_t n, uint32_t L, TwTables tw, W16 c) {
  extern __shared__ uint32_t s[];
  constexpr uint32_t H = 8 + WL;
  constexpr int WORDS = 2;
  constexpr uint32_t S = 16 * WORDS + 2;  // LDS row stride in words
  const uint32_t t = threadIdx.x & 15, q = threadIdx.x >> 4, lo = ((blockIdx.x << 4) + t) * WORDS;
  uint32_t* col = io + ((size_t)blockIdx.y << n) + lo;
  const uint32_t* src = in + ((size_t)blockIdx.y << n) + lo;  // may alias col (in-place): every word is read before its tile is written
  uint32_t x[WORDS][16];
  auto take = [&](const uint32_t* p, int k) { const uint2 v = *(const uint2*)p; x[0][k] = v.x; x[1][k] = v.y; };
  auto give = [&](uint32_t* p, int k) { *(uint2*)p = make_uint2(x[0][k], x[1][k]); };
  auto gload = [&](uint32_t row, int k) { take(src + ((size_t)row << L), k); };
  auto gstore = [&](uint32_t row, int k) { give(col + ((size_t)row << L), k); };
  auto sput = [&](uint32_t row, int k) { give(s + row * S + t * WORDS, k); };
  auto sget = [&](uint32_t row, int k) { take(s + row * S + t * WORDS, k); };
  // rounds: rows' bits 0-3, 4-7, then WLs more bits at 8
  constexpr int WLs = WL == 0 ? 1 : WL, SETS = 16 >> WLs;
  if (DIR == 0) {
    field_walk<4, 0>(q, gload);
#pragma unroll
    for (int w = 0; w < WORDS; w++) {
      uint32_t tws[16];
      interpass_twiddles<H, BIG>(tws, tw, q, lo + w, n);
#pragma unroll
      for (int j = 0; j < 16; j++) x[w][j] = mul(x[w][j], tws[j]);
      field_layers<4, 0, 0, 0>(x[w], q, tw.tw12, c);
    }
    field_walk<4, 0>(q, sput);
    __syncthreads();
    field_walk<4, 4>(q, sget);
#pragma unroll
    for (int w = 0; w < WORDS; w++) field_layers<4, 4, 0, 0>(x[w], q, tw.tw12, c);
    if (WL == 0) {
      field_walk<4, 4>(q, gstore);
      return;
    }
    field_walk<4, 4>(q, sput);
    __syncthreads();
    field_walk<WLs, 8>(q, sget);
#pragma unroll
    for (int w = 0; w < WORDS; w++) field_layers<WLs, 8, 0, 0>(x[w], q * SETS, tw.tw12, c);
    field_walk<WLs, 8>(q, gstore);
  } else {
    if (WL != 0) {
      field_walk<WLs, 8>(q, gload);
#pragma unroll
      for (int w = 0; w < WORDS; w++) field_layers<WLs, 8, 1, 0>(x[w], q * SETS, tw.tw12, c);
      field_walk<WLs, 8>(q, sput);
      __syncthreads();
      field_walk<4, 4>(q, sget);
    } else {
      field_walk<4, 4>(q, gload);
    }
#pragma unroll
    for (int w = 0; w < WORDS; w++) field_layers<4, 4, 1, 0>(x[w], q, tw.tw12, c);
    field_walk<4, 4>(q, sput);
    __syncthreads();
    field_walk<4, 0>(q, sget);
#pragma unroll
    for (int w = 0; w < WORDS; w++) {
      field_layers<4, 0, 1, 0>(x[w], q, tw.tw12, c);
      uint32_t tws[16];
      interpass_twiddles<H, BIG>(tws, tw, q, lo + w, n);
#pragma unroll
      for (int j = 0; j < 16; j++) x[w][j] = mul(x[w][j], tws[j]);
    }
    field_walk<4, 0>(q, gstore);
  }
}

// Third level (transforms of 2^14, 2^15 and above 2^23 points): the top four bits of the index -- 16 rows, 2^(n-4) words apart.  A thread owns one
// residue: sixteen words, the inter-pass twiddles w_n^(brev_4(j) * lo) as powers of one table product, one radix-16 butterfly in
// registers.  No LDS; every access of a wave is a 256-byte run per row, sixteen of them in flight per lane.
template <int DIR>
__global__ __launch_bounds__(256) void ntt_outer16_kernel(uint32_t* io, const uint32_t* in /* may alias io */, uint32_t n, TwTables twb, W16 c) {
  const uint32_t L = n - 4, lo = blockIdx.x * 256 + threadIdx.x;
  uint32_t* col = io + ((size_t)blockIdx.y << n) + lo;
  const uint32_t* src = in + ((size_t)blockIdx.y << n) + lo;
  uint32_t x[16], gp[16];
#pragma unroll
  for (int j = 0; j < 16; j++) x[j] = src[(size_t)j << L];
  gp[0] = ONE;
  gp[1] = omega_n<1>(twb, lo, n);
#pragma unroll
  for (int k = 2; k < 16; k++) gp[k] = mul_lazy(gp[k - 1], gp[1]);  // multipliers may stay below 2p
  if (DIR == 1) field_layers<4, 0, 1, 0>(x, 0, twb.tw12, c);
#pragma unroll
  for (int j = 1; j < 16; j++) x[j] = mul(x[j], gp[((j & 1) << 3) | ((j & 2) << 1) | ((j & 4) >> 1) | ((j & 8) >> 3)]);
  if (DIR == 0) field_layers<4, 0, 0, 0>(x, 0, twb.tw12, c);
#pragma unroll
  for (int j = 0; j < 16; j++) col[(size_t)j << L] = x[j];
}

__device__ __forceinline__ uint32_t lds_pad(uint32_t e) { return e + (e >> 4); }

struct ZkShift {        // optional fused f(x) -> f(3x) on the inverse transform's output
  const uint32_t* lo;   // 3^i, i < 2^11
  const uint32_t* hi;   // 3^(i << 11)
  const uint32_t* top;  // 3^(i << 22), i < 16
  uint32_t outer;       // the columns are the 2^outer blocks of a larger transform (third level): block b of a column holds the
                        // coefficients whose index ends in brev(b)
  uint32_t g[16];       // 3^(k << (n - 4)), k < 16, n = log2 of the whole transform
};

// One contiguous chunk of 2^L words (L = 8 + WL) per block of 2^(L-4) threads.
// Forward (DIR 0): DIT, optionally fed by an input 2^EXP_BITS (EXP_BITS 0 or 2) times shorter (each word replicated 2^EXP_BITS times,
// the first EXP_BITS layers skipped).  Inverse (DIR 1): DIF, result scaled by `scale`.
template <int WL, int DIR, int EXP_BITS, int ZK>
__global__ __launch_bounds__(1 << (4 + (WL < 4 ? 4 : WL))) void ntt_local16_kernel(uint32_t* out, const uint32_t* in /* may alias out */, uint32_t n_out,
                                                           const uint32_t* __restrict__ tw12, W16 c, uint32_t scale, ZkShift zk) {
  extern __shared__ uint32_t s[];
  constexpr uint32_t L = 8 + WL;
  // rounds: bits 0-3, 4-7, then WLs more bits at 8; L = 13 (WL = 5) adds a one-layer round at bit 12
  constexpr int WLs = WL == 0 ? 1 : (WL > 4 ? 4 : WL), SETS = 16 >> WLs;
  const uint32_t q = threadIdx.x;
  const size_t colid = blockIdx.y;
  const uint32_t base = blockIdx.x << L;
  uint32_t* dst = out + (colid << n_out) + base;
  uint32_t x[16];
  auto put = [&](uint32_t e, int k) { s[lds_pad(e)] = x[k]; };
  auto get = [&](uint32_t e, int k) { x[k] = s[lds_pad(e)]; };
  if (DIR == 0) {
    const uint32_t* src = in + (colid << (n_out - EXP_BITS)) + (base >> EXP_BITS);
    auto store = [&](uint32_t e, int k) { dst[e] = x[k]; };
    if (EXP_BITS == 2) {
      uint4 v = *(const uint4*)(src + q * 4);
      const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 16; j++) x[j] = w4[j >> 2];
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) {
        uint4 v = *(const uint4*)(src + q * 16 + 4 * k);
        x[4 * k] = v.x; x[4 * k + 1] = v.y; x[4 * k + 2] = v.z; x[4 * k + 3] = v.w;
      }
    }
    field_layers<4, 0, 0, EXP_BITS>(x, q, tw12, c);
    field_walk<4, 0>(q, put);
    __syncthreads();
    field_walk<4, 4>(q, get);
    field_layers<4, 4, 0, 0>(x, q, tw12, c);
    if (WL == 0) {
      field_walk<4, 4>(q, store);
      return;
    }
    field_walk<4, 4>(q, put);
    __syncthreads();
    field_walk<WLs, 8>(q, get);
    field_layers<WLs, 8, 0, 0>(x, q * SETS, tw12, c);
    if (WL != 5) {
      field_walk<WLs, 8>(q, store);
      return;
    }
    field_walk<4, 8>(q, put);
    __syncthreads();
    field_walk<1, 12>(q, get);
    field_layers<1, 12, 0, 0>(x, q * 8, tw12, c);
    field_walk<1, 12>(q, store);
  } else {
    const uint32_t* src = in + (colid << n_out) + base;
    auto load = [&](uint32_t e, int k) { x[k] = src[e]; };
    if (WL == 0) {
      field_walk<4, 4>(q, load);
    } else {
      if (WL == 5) {  // the one-layer round at bit 12 first, then through LDS into the bit-8 layout
        field_walk<1, 12>(q, load);
        field_layers<1, 12, 1, 0>(x, q * 8, tw12, c);
        field_walk<1, 12>(q, put);
        __syncthreads();
        field_walk<4, 8>(q, get);
        __syncthreads();  // the next exchange reuses the buffer
      } else {
        field_walk<WLs, 8>(q, load);
      }
      field_layers<WLs, 8, 1, 0>(x, q * SETS, tw12, c);
      field_walk<WLs, 8>(q, put);
      __syncthreads();
      field_walk<4, 4>(q, get);
    }
    field_layers<4, 4, 1, 0>(x, q, tw12, c);
    field_walk<4, 4>(q, put);
    __syncthreads();
    field_walk<4, 0>(q, get);
    field_layers<4, 0, 1, 0>(x, q, tw12, c);
    if (ZK) {
      // position p = base + 16 q + j holds the coefficient of x^brev_n(p), brev_n(p) = brev_n(base + 16 q) + (brev_4(j) << (n - 4));
      // as block b of a transform 2^outer times larger: x^(brev_n(p) << outer | brev_outer(b))
      const uint32_t e0 = (bitrev(base + q * 16, n_out) << zk.outer) | bitrev((uint32_t)colid & ((1u << zk.outer) - 1u), zk.outer);
      const uint32_t s0 = mul(scale, mul(mul(zk.lo[e0 & (TW_SIZE - 1)], zk.hi[(e0 >> TW_BITS) & (TW_SIZE - 1)]), zk.top[e0 >> TW_TOP]));
#pragma unroll
      for (int j = 0; j < 16; j++) x[j] = mul(x[j], mul(s0, zk.g[((j & 1) << 3) | ((j & 2) << 1) | ((j & 4) >> 1) | ((j & 8) >> 3)]));
#pragma unroll
      for (int k = 0; k < 4; k++) *(uint4*)(dst + q * 16 + 4 * k) = make_uint4(x[4 * k], x[4 * k + 1], x[4 * k + 2], x[4 * k + 3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++)
        *(uint4*)(dst + q * 16 + 4 * k) = make_uint4(mul(x[4 * k], scale), mul(x[4 * k + 1], scale), mul(x[4 * k + 2], scale), mul(x[4 * k + 3], scale));
    }
  }
}

template <class T>  // uint32_t, or uint4 for extension elements
__global__ void bit_reverse_kernel(T* io, uint32_t po2) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  T* col = io + ((size_t)blockIdx.y << po2);
  uint32_t j = bitrev(i, po2);
  if (i < j) {
    T a = col[i], b = col[j];
    col[i] = b;
    col[j] = a;
  }
}

// Tiled in-place bit reversal for po2 >= 2 EB, tiles of E x E elements, E = 2^EB: i = (a:EB | m:po2-2EB | b:EB) maps to
// (brev b | brev m | brev a), so the tile of middle index m lands, transposed and index-reversed, in the tile of brev(m).  A block
// swaps the pair (m, brev m) through LDS.  32 x 32 words: every global access is a 128-byte row; 16 x 16 uint4: 256-byte rows.
template <class T, int EB>
__global__ __launch_bounds__(256) void bit_reverse_tiled_kernel(T* io, uint32_t po2) {
  constexpr uint32_t E = 1u << EB, ROWS = 256 / E;  // rows of a tile that the block moves at a time
  __shared__ T ta[E][E + 1], tb[E][E + 1];
  const uint32_t mbits = po2 - 2 * EB, m = blockIdx.x, mr = bitrev(m, mbits);
  if (m > mr) return;
  T* col = io + ((size_t)blockIdx.y << po2);
  const uint32_t b = threadIdx.x & (E - 1), a0 = threadIdx.x >> EB;
#pragma unroll
  for (uint32_t k = 0; k < E / ROWS; k++) {
    const uint32_t a = a0 + ROWS * k;
    ta[a][b] = col[((size_t)a << (po2 - EB)) + (m << EB) + b];
    if (m != mr) tb[a][b] = col[((size_t)a << (po2 - EB)) + (mr << EB) + b];
  }
  __syncthreads();
  const uint32_t rb = __brev(b) >> (32 - EB);
#pragma unroll
  for (uint32_t k = 0; k < E / ROWS; k++) {
    const uint32_t a = a0 + ROWS * k, ra = __brev(a) >> (32 - EB);
    // new tile(mr)[a][b] = old tile(m)[brev b][brev a]; and symmetrically
    col[((size_t)a << (po2 - EB)) + (mr << EB) + b] = ta[rb][ra];
    if (m != mr) col[((size_t)a << (po2 - EB)) + (m << EB) + b] = tb[rb][ra];
  }
}

__global__ void zk_shift_kernel(uint32_t* io, uint32_t po2, const uint32_t* pow3_lo, const uint32_t* pow3_hi, const uint32_t* pow3_top) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t* col = io + ((size_t)blockIdx.y << po2);
  uint32_t e = bitrev(i, po2);
  uint32_t s = mul(pow3_lo[e & (TW_SIZE - 1)], pow3_hi[(e >> TW_BITS) & (TW_SIZE - 1)]);
  if (po2 > TW_TOP) s = mul(s, pow3_top[e >> TW_TOP]);
  col[i] = mul(col[i], s);
}

constexpr uint32_t LOCAL16_MIN = 8;  // the radix-16 contiguous pass takes chunks of 2^8 .. 2^13 words; smaller transforms are radix-2
struct Split16 {
  uint32_t L, H;   // contiguous chunk 2^L, strided 2^H (0 = no strided pass)
  uint32_t outer;  // third level: a column is 2^outer blocks of 2^(L + H) words (0 = none)
};
// Up to 2^13: one contiguous pass.  2^14, 2^15: sixteen contiguous blocks of 2^10, 2^11 and the pass over the top four bits.
// 2^16 .. 2^22: two passes (H = 8 or 9: two strided tiles per CU).  2^23: two passes with 2^10-row tiles (139 KB of LDS, one block
// per CU) and the ROU[26] tables.  2^24 .. 2^26 (segments of 2^22 .. 2^24 rows -- what 288 GB of HBM has room for): three levels.
// With a third level a column's 16 blocks are transformed like 16 columns by the passes below it, and one register-only radix-16
// pass runs across the blocks (ntt_outer16_kernel).
static Split16 split16_for(uint32_t n) {
  Split16 sp{n, 0, 0};
  if (n <= 13) return sp;
  if (n <= 15 || n > 23) { sp.outer = 4; n -= 4; }
  if (n >= 16) sp.H = n <= 20 ? 8 : (n <= 22 ? 9 : 10);  // the contiguous pass takes up to 2^13 words
  sp.L = n - sp.H;
  return sp;
}
static W16 make_w16(bool inverse) {
  W16 c;
  uint32_t w = inverse ? rou_rev(4) : rou_fwd(4), cur = ONE;
  for (int k = 0; k < 8; k++) {
    c.w[k] = cur;
    cur = mul(cur, w);
  }
  return c;
}

constexpr size_t GRID_Y_MAX = 32768;  // columns per launch (blockIdx.y): the blocks of large transforms count as columns

// `count` columns, 2^n_out words apart at `out`, as chunks of 2^L words through the radix-2 kernel
template <int DIR>
static void launch_local(r0h_ctx* ctx, uint32_t L, size_t count, uint32_t* out, const uint32_t* in, uint32_t n_out, uint32_t expand_bits, const uint32_t* tw12,
                         uint32_t scale) {
  for (size_t c0 = 0; c0 < count; c0 += GRID_Y_MAX) {
    const dim3 grid(1u << (n_out - L), (uint32_t)std::min(count - c0, GRID_Y_MAX));
    hipLaunchKernelGGL(ntt_local_kernel<DIR>, grid, dim3(256), (size_t)4 << L, ctx->stream, out + (c0 << n_out), in + (c0 << (n_out - expand_bits)), L, n_out,
                       expand_bits, tw12, scale);
  }
}

// The instantiations that exist: chunks of 2^8 .. 2^13 words; strided tiles of 2^8 .. 2^10 rows
using Local16Kernel = void (*)(uint32_t*, const uint32_t*, uint32_t, const uint32_t*, W16, uint32_t, ZkShift);
template <int DIR, int EXP_BITS, int ZK>
static Local16Kernel local16_kernel(uint32_t L) {
  static const Local16Kernel k[6] = {ntt_local16_kernel<0, DIR, EXP_BITS, ZK>, ntt_local16_kernel<1, DIR, EXP_BITS, ZK>, ntt_local16_kernel<2, DIR, EXP_BITS, ZK>,
                                     ntt_local16_kernel<3, DIR, EXP_BITS, ZK>, ntt_local16_kernel<4, DIR, EXP_BITS, ZK>, ntt_local16_kernel<5, DIR, EXP_BITS, ZK>};
  return k[L - 8];
}
using Strided16Kernel = void (*)(uint32_t*, const uint32_t*, uint32_t, uint32_t, TwTables, W16);
template <int DIR, int BIG>
static Strided16Kernel strided16_kernel(uint32_t H) {
  static const Strided16Kernel k[3] = {ntt_strided16_kernel<0, DIR, BIG>, ntt_strided16_kernel<1, DIR, BIG>, ntt_strided16_kernel<2, DIR, BIG>};
  return k[H - 8];
}
static size_t local16_lds_bytes(uint32_t L) { return (((size_t)1 << L) + ((size_t)1 << (L - 4))) * 4; }
constexpr size_t strided16_lds_bytes(uint32_t H) { return ((size_t)1 << H) * (16 * 2 + 2) * 4; }

template <int DIR, int EXP_BITS, int ZK = 0>
static void launch_local16(r0h_ctx* ctx, uint32_t L, uint32_t blocks_x, size_t count, uint32_t* out, const uint32_t* in, uint32_t n_out, const uint32_t* tw12,
                           const W16& c, uint32_t scale, const ZkShift& zk = ZkShift{}) {
  const Local16Kernel kernel = local16_kernel<DIR, EXP_BITS, ZK>(L);
  for (size_t c0 = 0; c0 < count; c0 += GRID_Y_MAX) {
    const dim3 grid(blocks_x, (uint32_t)std::min(count - c0, GRID_Y_MAX));
    hipLaunchKernelGGL(kernel, grid, dim3(1u << (L - 4)), local16_lds_bytes(L), ctx->stream, out + (c0 << n_out),
                       in + (c0 << (DIR == 0 ? n_out - EXP_BITS : n_out)), n_out, tw12, c, scale, zk);
  }
}
template <int DIR, int BIG>
static void launch_strided16(r0h_ctx* ctx, uint32_t H, size_t count, uint32_t* io, const uint32_t* in, uint32_t n, uint32_t L,
                             const TwTables& tw, const W16& c) {
  const Strided16Kernel kernel = strided16_kernel<DIR, BIG>(H);
  for (size_t c0 = 0; c0 < count; c0 += GRID_Y_MAX) {
    const dim3 grid(1u << (L - 5), (uint32_t)std::min(count - c0, GRID_Y_MAX));  // 32 residues per block
    // tiles above 64 KB of LDS: the limit was raised for this device when its first context was created (ntt_init_device)
    hipLaunchKernelGGL(kernel, grid, dim3(16u << (H - 4)), strided16_lds_bytes(H), ctx->stream, io + (c0 << n), in + (c0 << n), n, L, tw, c);
  }
}

template <int DIR>
static void launch_outer16(r0h_ctx* ctx, size_t count, uint32_t* io, const uint32_t* in, uint32_t n, const TwTables& twb, const W16& c) {
  for (size_t c0 = 0; c0 < count; c0 += GRID_Y_MAX) {
    const dim3 grid((1u << (n - 4)) / 256, (uint32_t)std::min(count - c0, GRID_Y_MAX));
    hipLaunchKernelGGL(ntt_outer16_kernel<DIR>, grid, dim3(256), 0, ctx->stream, io + (c0 << n), in + (c0 << n), n, twb, c);
  }
}

// Dynamic LDS above the 64 KB default has to be asked for per kernel instantiation and device.  Done for every instantiation
// that needs it when a context is created (r0h_ctx_create, after hipSetDevice), so no launch can race the request and a
// refusal is reported instead of surfacing later as "launch failed".
template <int DIR, int BIG>
static const char* raise_lds_limits() {
  for (uint32_t H = 8; H <= 10; H++) {
    const size_t lds = strided16_lds_bytes(H);
    if (lds > 65536) R0H_TRY_HIP(hipFuncSetAttribute((const void*)(strided16_kernel<DIR, BIG>(H)), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  return nullptr;
}
const char* ntt_init_device() {
  R0H_TRY((raise_lds_limits<0, 0>()));
  R0H_TRY((raise_lds_limits<1, 0>()));
  R0H_TRY((raise_lds_limits<0, 1>()));
  R0H_TRY((raise_lds_limits<1, 1>()));
  return nullptr;
}

static const char* zk_shift_cols(r0h_ctx* ctx, uint32_t* io, size_t count, uint32_t po2) {
  const uint32_t threads = po2 >= 8 ? 256 : (1u << po2);
  KScope ks(ctx, "zk_shift_kernel", 8.0 * count * (double)((size_t)1 << po2));
  for (size_t c0 = 0; c0 < count; c0 += GRID_Y_MAX) {
    const dim3 grid((1u << po2) / threads, (uint32_t)std::min(count - c0, GRID_Y_MAX));
    hipLaunchKernelGGL(zk_shift_kernel, grid, dim3(threads), 0, ctx->stream, io + (c0 << po2), po2, ctx->pow3_lo, ctx->pow3_hi, ctx->pow3_top);
  }
  return launch_ok("zk_shift_kernel");
}

// Forward transform of `count` columns: bit-reversed coefficients, 2^(n - expand_bits) words apart at `in`; natural evaluations,
// 2^n words apart at `out`; expand_bits < split16_for(n).L
static const char* forward16(r0h_ctx* ctx, uint32_t* out, const uint32_t* in, size_t count, uint32_t n, uint32_t expand_bits) {
  const Split16 sp = split16_for(n);
  const W16 c = make_w16(false);
  const TwTables tw{ctx->tw_lo[0], ctx->tw_hi[0], ctx->tw12[0]}, twb{ctx->twb_lo[0], ctx->twb_hi[0], ctx->tw12[0]};
  const uint32_t n_in = n - sp.outer;       // what the first two levels transform
  const size_t blocks = count << sp.outer;  // a column's blocks are contiguous on both sides: they are columns of the inner transform
  const double words = (double)((size_t)1 << n);
  {
    KScope ks(ctx, "ntt_local_kernel", 4.0 * count * (words + (double)((size_t)1 << (n - expand_bits))));
    if (sp.L < LOCAL16_MIN || (expand_bits != 0 && expand_bits != 2)) launch_local<0>(ctx, sp.L, blocks, out, in, n_in, expand_bits, tw.tw12, 0u);
    else if (expand_bits == 2) launch_local16<0, 2>(ctx, sp.L, 1u << (n_in - sp.L), blocks, out, in, n_in, tw.tw12, c, 0u);
    else launch_local16<0, 0>(ctx, sp.L, 1u << (n_in - sp.L), blocks, out, in, n_in, tw.tw12, c, 0u);
  }
  R0H_TRY(launch_ok("ntt_local_kernel<fwd>"));
  if (sp.H) {
    KScope ks(ctx, "ntt_strided_kernel", 8.0 * count * words);
    if (n_in > TW_TOP) launch_strided16<0, 1>(ctx, sp.H, blocks, out, out, n_in, sp.L, twb, c);
    else launch_strided16<0, 0>(ctx, sp.H, blocks, out, out, n_in, sp.L, tw, c);
    R0H_TRY(launch_ok("ntt_strided16_kernel<fwd>"));
  }
  if (sp.outer) {
    KScope ks(ctx, "ntt_outer_kernel", 8.0 * count * words);
    launch_outer16<0>(ctx, count, out, out, n, twb, c);
    R0H_TRY(launch_ok("ntt_outer16_kernel<fwd>"));
  }
  return nullptr;
}

// The transpose: natural evaluations at `src` (may be `io`) -> bit-reversed coefficients at `io`, scaled by 1/2^n, f(x) -> f(3x) on request
static const char* inverse16(r0h_ctx* ctx, uint32_t* io, const uint32_t* src, size_t count, uint32_t n, bool zk_shift) {
  const Split16 sp = split16_for(n);
  const W16 c = make_w16(true);
  const TwTables tw{ctx->tw_lo[1], ctx->tw_hi[1], ctx->tw12[1]}, twb{ctx->twb_lo[1], ctx->twb_hi[1], ctx->tw12[1]};
  const uint32_t n_in = n - sp.outer, norm = inv(enc(1u << n));
  const size_t blocks = count << sp.outer;
  const double words = (double)((size_t)1 << n);
  const uint32_t* cur = src;
  if (sp.outer) {
    KScope ks(ctx, "ntt_outer_kernel", 8.0 * count * words);
    launch_outer16<1>(ctx, count, io, cur, n, twb, c);
    R0H_TRY(launch_ok("ntt_outer16_kernel<inv>"));
    cur = io;
  }
  if (sp.H) {
    KScope ks(ctx, "ntt_strided_kernel", 8.0 * count * words);
    if (n_in > TW_TOP) launch_strided16<1, 1>(ctx, sp.H, blocks, io, cur, n_in, sp.L, twb, c);
    else launch_strided16<1, 0>(ctx, sp.H, blocks, io, cur, n_in, sp.L, tw, c);
    R0H_TRY(launch_ok("ntt_strided16_kernel<inv>"));
    cur = io;
  }
  {
    KScope ks(ctx, "ntt_local_kernel", 8.0 * count * words);
    if (sp.L < LOCAL16_MIN) {
      launch_local<1>(ctx, sp.L, blocks, io, cur, n_in, 0u, tw.tw12, norm);
    } else if (zk_shift) {  // fused into the last pass: no separate sweep over the coefficients
      ZkShift zk{ctx->pow3_lo, ctx->pow3_hi, ctx->pow3_top, sp.outer, {0}};
      const uint32_t g = fpow(enc(3), (uint64_t)1 << (n - 4));
      uint32_t pw = ONE;
      for (int k = 0; k < 16; k++) { zk.g[k] = pw; pw = mul(pw, g); }
      launch_local16<1, 0, 1>(ctx, sp.L, 1u << (n_in - sp.L), blocks, io, cur, n_in, tw.tw12, c, norm, zk);
    } else {
      launch_local16<1, 0>(ctx, sp.L, 1u << (n_in - sp.L), blocks, io, cur, n_in, tw.tw12, c, norm);
    }
  }
  R0H_TRY(launch_ok("ntt_local_kernel<inv>"));
  if (sp.L < LOCAL16_MIN && zk_shift) return zk_shift_cols(ctx, io, count, n);  // the radix-2 kernel carries no shift: a sweep of its own
  return nullptr;
}

const char* interpolate_ntt(r0h_ctx* ctx, r0h_buf* io, const r0h_buf* src, uint32_t count, uint32_t po2, bool zk_shift) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && io && src, "r0h_batch_interpolate_ntt: NULL argument");
  R0H_REQUIRE(((size_t)count << po2) * 4 <= src->bytes, "r0h_batch_interpolate_ntt: %u columns of 2^%u exceed the source buffer", count, po2);
  R0H_REQUIRE(po2 >= 1 && po2 <= MAX_DOMAIN_PO2, "r0h_batch_interpolate_ntt: po2 %u outside [1, %u]", po2, MAX_DOMAIN_PO2);
  R0H_REQUIRE(((size_t)count << po2) * 4 <= io->bytes, "r0h_batch_interpolate_ntt: %u columns of 2^%u exceed the buffer", count, po2);
  if (!count) return nullptr;
  return inverse16(ctx, u32(io), u32(src), count, po2, zk_shift);
  R0H_GUARD_END
}

const char* bit_reverse_ext(r0h_ctx* ctx, r0h_buf* io, uint32_t count, uint32_t po2) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && io && po2 <= MAX_DOMAIN_PO2, "bit_reverse_ext: bad argument");
  R0H_REQUIRE(((size_t)count << po2) * 16 <= io->bytes, "bit_reverse_ext: %u columns of 2^%u exceed the buffer", count, po2);
  if (!count || po2 == 0) return nullptr;
  KScope ks(ctx, "bit_reverse_kernel", 32.0 * count * (double)(1u << po2));
  if (po2 >= 8) {
    hipLaunchKernelGGL((bit_reverse_tiled_kernel<uint4, 4>), dim3(1u << (po2 - 8), count), dim3(256), 0, ctx->stream, (uint4*)io->ptr, po2);
  } else {
    hipLaunchKernelGGL(bit_reverse_kernel<uint4>, dim3(1, count), dim3(1u << po2), 0, ctx->stream, (uint4*)io->ptr, po2);
  }
  return launch_ok("bit_reverse_ext kernel");
  R0H_GUARD_END
}

}  // namespace r0h

using namespace r0h;

extern "C" {

const char* r0h_batch_interpolate_ntt(r0h_ctx* ctx, r0h_buf* io, uint32_t count, uint32_t po2) { return interpolate_ntt(ctx, io, io, count, po2, false); }
const char* r0h_batch_interpolate_ntt_zk_shift(r0h_ctx* ctx, r0h_buf* io, uint32_t count, uint32_t po2) { return interpolate_ntt(ctx, io, io, count, po2, true); }

const char* r0h_batch_expand_into_evaluate_ntt(r0h_ctx* ctx, r0h_buf* out, const r0h_buf* in, uint32_t count,
                                               uint32_t in_po2, uint32_t expand_bits) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && out && in, "r0h_batch_expand_into_evaluate_ntt: NULL argument");
  const uint32_t n = in_po2 + expand_bits;
  R0H_REQUIRE(n >= 1 && n <= MAX_DOMAIN_PO2, "r0h_batch_expand_into_evaluate_ntt: output po2 %u outside [1, %u]", n, MAX_DOMAIN_PO2);
  R0H_REQUIRE(((size_t)count << in_po2) * 4 <= in->bytes && ((size_t)count << n) * 4 <= out->bytes,
              "r0h_batch_expand_into_evaluate_ntt: %u columns exceed the buffers", count);
  R0H_REQUIRE(out->ptr != in->ptr || expand_bits == 0, "r0h_batch_expand_into_evaluate_ntt: in-place expansion is not supported");
  if (!count) return nullptr;
  R0H_REQUIRE(expand_bits < split16_for(n).L, "r0h_batch_expand_into_evaluate_ntt: expand_bits %u too large for size 2^%u", expand_bits, n);
  return forward16(ctx, u32(out), u32(in), count, n, expand_bits);
  R0H_GUARD_END
}

const char* r0h_batch_bit_reverse(r0h_ctx* ctx, r0h_buf* io, uint32_t count, uint32_t po2) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && io, "r0h_batch_bit_reverse: NULL argument");
  R0H_REQUIRE(po2 <= MAX_DOMAIN_PO2 + 2, "r0h_batch_bit_reverse: po2 %u too large", po2);
  R0H_REQUIRE(((size_t)count << po2) * 4 <= io->bytes, "r0h_batch_bit_reverse: %u columns of 2^%u exceed the buffer", count, po2);
  if (!count || po2 == 0) return nullptr;
  KScope ks(ctx, "bit_reverse_kernel", 8.0 * count * (double)(1u << po2));
  if (po2 >= 10) {
    hipLaunchKernelGGL((bit_reverse_tiled_kernel<uint32_t, 5>), dim3(1u << (po2 - 10), count), dim3(256), 0, ctx->stream, u32(io), po2);
    return launch_ok("bit_reverse_tiled_kernel");
  }
  uint32_t threads = po2 >= 8 ? 256 : (1u << po2);
  dim3 grid((1u << po2) / threads, count);
  hipLaunchKernelGGL(bit_reverse_kernel<uint32_t>, grid, dim3(threads), 0, ctx->stream, u32(io), po2);
  return launch_ok("bit_reverse_kernel");
  R0H_GUARD_END
}

const char* r0h_zk_shift(r0h_ctx* ctx, r0h_buf* io, uint32_t count, uint32_t po2) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && io, "r0h_zk_shift: NULL argument");
  R0H_REQUIRE(po2 <= MAX_DOMAIN_PO2, "r0h_zk_shift: po2 %u too large", po2);
  R0H_REQUIRE(((size_t)count << po2) * 4 <= io->bytes, "r0h_zk_shift: %u columns of 2^%u exceed the buffer", count, po2);
  if (!count) return nullptr;
  return zk_shift_cols(ctx, u32(io), count, po2);
  R0H_GUARD_END
}

}  // extern "C"
