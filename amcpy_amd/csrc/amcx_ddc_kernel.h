// The digital down-converter (include/amcx.h, amcx_tune_decimate; ABI 11): mixer, real FIR low-pass, integer decimation, from
// one contiguous stream of complex64 / sc16 / ci8 / cu8 samples to packed complex64, D times fewer.
//
//   phi(n) = phase0 + n * phase_step   (uint64, exact; n counts the call's input samples)
//   v[n]   = x[n] * exp(+2 pi j phi(n) / 2^64)
//   y[m]   = sum_{k = 0 .. T-1} h[k] * v[m D + T - 1 - k]
//
// A SAMPLE'S BITS DEPEND ON NOTHING BUT THE SAMPLE.  x[n] is what ABI 9 / 10 say -- (float)integer * scale, ONE float32
// multiplication per component -- whichever load brought it in.  The mixer's angle is formed from the top 32 bits of phi(n)
// by integer range reduction (ddc_mixer): the same integer gives the same (cos, sin), and phi < 2^32 gives exactly 1 + 0j, for
// which the product is skipped (v = x, signed zeros included).  y[m] is h[0] v[.] and then one FMA per component and tap in the
// order k = 1 ... T - 1, whichever thread of whichever tile sums it: a stream cut into calls at any multiple of D, with phase0
// advanced, gives the one-call result bit for bit.
//
// THE LAUNCH.  256 threads, a persistent grid over TILES of `tile` consecutive outputs (ddc_tile_outputs: chosen by the host so
// that a tile's input span, (tile - 1) D + T samples, fits kDdcStage).  A workgroup puts the taps into LDS once; per tile it
// stages the span's MIXED samples in LDS -- every input is mixed once per tile that reads it -- barrier, then thread t sums the
// outputs t, t + 256, ... of the tile and stores them (8-byte vector stores, consecutive lanes consecutive outputs), barrier.
// D > T is legal; the samples between two windows are then staged with the rest and never read (a tile of few outputs, down
// to one at D = 4096, stages few of them).  No atomics, nothing shared between workgroups.
//
// ONE STAGING ROUTINE, THREE LOADS, THE SAME BITS.  ddc_stage_span is the only code that decides which bytes of the source are
// read, here, in the filter bank (amcx_bank_kernel.h) and in the resampler (amcx_resample_kernel.h).  A span is read in items of
// 16 bytes (2 complex64 / 4 sc16 / 8 eight-bit samples) from its first 16-byte boundary on, and one sample per step in front of
// that boundary and behind the last whole item: any sample-aligned address, any span.  Every sample is mixed as it is stored.
//
// LDS IMAGE.  Sample i of the span lives at float2 index i + (i >> 5).  Lanes that sum neighbouring outputs read D samples
// apart, 2 D dwords: without the pad a power of two D >= 32 puts a whole half-wave onto one bank pair; with it the 32 lanes of
// a half-wave are on 32 different pairs for every power of two D <= 32 (and every odd D), 2-way at 64.
//
// KERNEL ORDER (amcx_launch.h): plain kernels in the header amcx.hip includes FIRST, in front of the 8-bit widening kernels --
// every kernel that was there before keeps its bytes: tools/codeobj_gate.py --kernels, profiles/r15_ddc_codeobj_kernels.txt.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace amcx {

constexpr int kDdcThreads = 256;           // of all three stream kernels: ddc_stage_span strides by it
constexpr int kDdcMaxTaps = 2048;
constexpr int kDdcMaxDecim = 4096;
constexpr int kDdcStage = 6144;            // most samples of one tile's span: 6336 float2 with the pad, 49.5 KiB

__host__ __device__ __forceinline__ int ddc_pad(int i) { return i + (i >> 5); }

// outputs per tile for (T, D): as many as kDdcStage holds the span of, at least one (T <= 2048 always fits)
inline int ddc_tile_outputs(int T, int D) { return (kDdcStage - T) / D + 1; }
// bytes of the padded image of a span of `span` samples, rounded up to 16: where the taps begin
__host__ __device__ __forceinline__ int ddc_stage_bytes(int span) { return (8 * (ddc_pad(span - 1) + 1) + 15) / 16 * 16; }
// dynamic LDS of a launch: the padded span of a full tile, then the taps (58 880 bytes at most: no attribute needed)
inline size_t ddc_lds_bytes(int T, int D) {
  return (size_t)ddc_stage_bytes((ddc_tile_outputs(T, D) - 1) * D + T) + (size_t)4 * (size_t)T;
}

// exp(2 pi j p / 2^32): the nearest quarter turn q and a remainder r in [-2^29, 2^29) are integers, so the reduction is exact;
// sine and cosine of r's angle (at most pi / 4) by polynomials of the Cephes single-precision kernels, evaluated with FMAs;
// the quarter turns are swaps and sign changes.  p == 0 gives exactly (1, 0).
__device__ __forceinline__ float2 ddc_mixer(unsigned p) {
  const unsigned q = (p + 0x20000000u) >> 30;
  const int r = (int)(p - (q << 30));
  const float t = (float)r * 1.4629180792671596e-9f;          // 2 pi / 2^32
  const float z = t * t;
  float s = __builtin_fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f);
  s = __builtin_fmaf(z, s, -1.6666654611e-1f);
  s = __builtin_fmaf(t * z, s, t);
  float c = __builtin_fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f);
  c = __builtin_fmaf(z, c, 4.166664568298827e-2f);
  c = __builtin_fmaf(z * z, c, __builtin_fmaf(z, -0.5f, 1.0f));
  // q = 0: (c, s); 1: (-s, c); 2: (-c, -s); 3: (s, -c)
  const float a = (q & 1u) ? s : c, b = (q & 1u) ? c : s;
  return make_float2(((q + 1u) & 2u) ? -a : a, (q & 2u) ? -b : b);
}

// v = x * w(phi), phi's top 32 bits the angle
__device__ __forceinline__ float2 ddc_mix(float2 x, unsigned long long phi) {
  const unsigned p = (unsigned)(phi >> 32);
  const float2 w = ddc_mixer(p);
  const float2 v = make_float2(__builtin_fmaf(x.x, w.x, -(x.y * w.y)), __builtin_fmaf(x.x, w.y, x.y * w.x));
  return p == 0u ? x : v;              // (a select, not a branch: the lanes of a wave differ)
}

// ---- the three sample formats: bytes per sample, samples per 16-byte item, one sample, one item ------------------------------
struct DdcC64 {
  static constexpr int kBytes = 8, kItem = 2;
  static __device__ __forceinline__ float2 one(const char* p, float, unsigned) { return *reinterpret_cast<const float2*>(p); }
  static __device__ __forceinline__ void item(const char* p, float, unsigned, float2* x) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    x[0] = make_float2(v.x, v.y);
    x[1] = make_float2(v.z, v.w);
  }
};
// the two int16 halves of a word as one sample
__device__ __forceinline__ float2 ddc_sc16_word(unsigned w, float scale) {
  return make_float2((float)((int)(w << 16) >> 16) * scale, (float)((int)w >> 16) * scale);
}
struct DdcSc16 {
  static constexpr int kBytes = 4, kItem = 4;
  static __device__ __forceinline__ float2 one(const char* p, float scale, unsigned) {
    return ddc_sc16_word(*reinterpret_cast<const unsigned*>(p), scale);
  }
  static __device__ __forceinline__ void item(const char* p, float scale, unsigned, float2* x) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    x[0] = ddc_sc16_word(v.x, scale);
    x[1] = ddc_sc16_word(v.y, scale);
    x[2] = ddc_sc16_word(v.z, scale);
    x[3] = ddc_sc16_word(v.w, scale);
  }
};
// bytes 2 k, 2 k + 1 (k = 0, 1) of a word, flipped already (0x80 per byte for cu8: byte - 128), as one sample
__device__ __forceinline__ float2 ddc_iq8_half(unsigned w, int k, float scale) {
  return make_float2((float)((int)(w << (24 - 16 * k)) >> 24) * scale, (float)((int)(w << (16 - 16 * k)) >> 24) * scale);
}
struct DdcIq8 {
  static constexpr int kBytes = 2, kItem = 8;
  static __device__ __forceinline__ float2 one(const char* p, float scale, unsigned flip4) {
    return ddc_iq8_half(*reinterpret_cast<const unsigned short*>(p) ^ (flip4 & 0xffffu), 0, scale);
  }
  static __device__ __forceinline__ void item(const char* p, float scale, unsigned flip4, float2* x) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    const unsigned w[4] = {v.x ^ flip4, v.y ^ flip4, v.z ^ flip4, v.w ^ flip4};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[2 * j] = ddc_iq8_half(w[j], 0, scale);
      x[2 * j + 1] = ddc_iq8_half(w[j], 1, scale);
    }
  }
};

// ---- staging (ONE STAGING ROUTINE above) -------------------------------------------------------------------------------------
// the float2 index of a span's sample i in the LDS image: padded (LDS IMAGE above), or plain (the bank's, amcx_bank_kernel.h)
struct DdcPadded {
  static __device__ __forceinline__ int at(int i) { return ddc_pad(i); }
};
struct DdcPlain {
  static __device__ __forceinline__ int at(int i) { return i; }
};

// The workgroup's kDdcThreads threads (tid) read the `span` samples from `base` on -- the stream's samples s0 ... s0 + span - 1
// -- and nothing else, and store sample i, mixed, at stage[Image::at(i)].  The caller's barrier follows.  kUnroll: the item
// loop's unroll count, 4 in the bank's kernels and 1 in the others (what the compiler does with that loop unhinted).
template <class L, class Image, int kUnroll>
__device__ __forceinline__ void ddc_stage_span(float2* stage, const char* __restrict__ base, long long s0, int span,
                                               float scale, unsigned flip4, unsigned long long phase0,
                                               unsigned long long phase_step, int tid) {
  // in front of the first 16-byte boundary, whole items, behind the last whole item
  int head = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(base) & 15u)) & 15u) / L::kBytes;
  if (head > span) head = span;
  const int items = (span - head) / L::kItem;
  const int tail0 = head + items * L::kItem;
  for (int i = tid; i < head; i += kDdcThreads)
    stage[Image::at(i)] = ddc_mix(L::one(base + (size_t)i * L::kBytes, scale, flip4), phase0 + (unsigned long long)(s0 + i) * phase_step);
#pragma unroll kUnroll
  for (int it = tid; it < items; it += kDdcThreads) {
    const int i0 = head + it * L::kItem;
    float2 x[L::kItem];
    L::item(base + (size_t)i0 * L::kBytes, scale, flip4, x);
#pragma unroll
    for (int j = 0; j < L::kItem; ++j)
      stage[Image::at(i0 + j)] = ddc_mix(x[j], phase0 + (unsigned long long)(s0 + i0 + j) * phase_step);
  }
  for (int i = tail0 + tid; i < span; i += kDdcThreads)
    stage[Image::at(i)] = ddc_mix(L::one(base + (size_t)i * L::kBytes, scale, flip4), phase0 + (unsigned long long)(s0 + i) * phase_step);
}

// Reads src[0 .. (M - 1) D + T) samples and taps[0 .. T), writes out[0 .. M), nothing else.  n_tiles = ceil(M / tile); the
// dynamic LDS is ddc_lds_bytes(T, D).
template <class L>
__device__ __forceinline__ void ddc_body(const char* __restrict__ src, float scale, unsigned flip4, unsigned long long phase0,
                                         unsigned long long phase_step, const float* __restrict__ taps, int T, int D,
                                         float2* __restrict__ out, long long M, int tile, long long n_tiles) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ddc_lds[];
  float2* const stage = reinterpret_cast<float2*>(ddc_lds);
  float* const h = reinterpret_cast<float*>(ddc_lds + ddc_stage_bytes((tile - 1) * D + T));
  const int tid = (int)threadIdx.x;
  for (int k = tid; k < T; k += kDdcThreads) h[k] = taps[k];          // (the first tile's barrier orders these too)
  for (long long ti = blockIdx.x; ti < n_tiles; ti += gridDim.x) {
    const long long m0 = ti * tile;
    const int n_out = M - m0 < tile ? (int)(M - m0) : tile;
    const long long s0 = m0 * D;                                       // the span's first input sample
    const int span = (n_out - 1) * D + T;
    const char* const base = src + s0 * L::kBytes;
    ddc_stage_span<L, DdcPadded, 1>(stage, base, s0, span, scale, flip4, phase0, phase_step, tid);
    __syncthreads();
    for (int o = tid; o < n_out; o += kDdcThreads) {
      const int top = o * D + T - 1;                                   // the sample tap 0 multiplies
      const float2 v0 = stage[ddc_pad(top)];
      const float h0 = h[0];
      float re = h0 * v0.x, im = h0 * v0.y;
#pragma unroll 4
      for (int k = 1; k < T; ++k) {
        const float2 v = stage[ddc_pad(top - k)];
        const float hk = h[k];
        re = __builtin_fmaf(hk, v.x, re);
        im = __builtin_fmaf(hk, v.y, im);
      }
      out[m0 + o] = make_float2(re, im);
    }
    __syncthreads();                                                   // the next tile's staging overwrites what was just read
  }
}

#define AMCX_DDC_PARAMS                                                                                                  \
  const char* __restrict__ src, float scale, unsigned flip4, unsigned long long phase0, unsigned long long phase_step,   \
      const float* __restrict__ taps, int T, int D, float2* __restrict__ out, long long M, int tile, long long n_tiles
#define AMCX_DDC_ARGS src, scale, flip4, phase0, phase_step, taps, T, D, out, M, tile, n_tiles

__global__ __launch_bounds__(kDdcThreads) void amcx_ddc_c64_kernel(AMCX_DDC_PARAMS) { ddc_body<DdcC64>(AMCX_DDC_ARGS); }
__global__ __launch_bounds__(kDdcThreads) void amcx_ddc_sc16_kernel(AMCX_DDC_PARAMS) { ddc_body<DdcSc16>(AMCX_DDC_ARGS); }
__global__ __launch_bounds__(kDdcThreads) void amcx_ddc_iq8_kernel(AMCX_DDC_PARAMS) { ddc_body<DdcIq8>(AMCX_DDC_ARGS); }

#undef AMCX_DDC_PARAMS
#undef AMCX_DDC_ARGS

}  // namespace amcx
