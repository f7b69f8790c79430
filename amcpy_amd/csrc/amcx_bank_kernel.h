// The polyphase analysis filter bank (include/amcx.h, amcx_filter_bank; ABI 12): every channel of a raster of C from ONE pass
// over a contiguous stream of complex64 / sc16 / ci8 / cu8 samples, to packed complex64, channel-major.
//
//   phi(n) = phase0 + n * phase_step                                    (uint64, exact; n counts the call's input samples)
//   v[n]   = x[n] * exp(+2 pi j phi(n) / 2^64)                           (ddc_mix of amcx_ddc_kernel.h: the same bits)
//   a(n)   = (sample_index0 + n) mod C
//   n_m    = m D + T - 1
//   y[c,m] = sum_{k < T} h[k] v[n_m - k] exp(-2 pi j c a(n_m - k) / C)   c = 0 ... C - 1
//
// i.e. channel c is the down-converter with phase_step - c 2^64 / C.  Computed in two steps:
//   1. the BRANCH SUMS u_m[p] = sum_{q < P, p + q C < T} h[p + q C] v[n_m - p - q C], P = ceil(T / C): one product, then one
//      FMA per component in ascending q.  A tap index >= T does not exist: it is never read, and no sample is read for it
//      (a branch with no tap at all, p >= T, is +0).
//   2. y[., m] = the unnormalised C-point DFT with kernel e^{+2 pi j c r / C} of g[r] = u_m[(r + a(n_m)) mod C]: the sample-index
//      rotation is a circular shift of the transform's input, not a multiplication.  The transform is radix 2, decimation in
//      frequency, in place: stage s = 0 ... log2 C - 1 (half = C >> (s + 1)) does (A, B) -> (A + B, (A - B) w) on the points
//      half apart, w = exp(2 pi j k / (2 half)), k the index within the half, the product formed as ddc_mix forms its own (two
//      FMAs over two products); y[c] ends at the bit-reversed c.  The twiddles are ddc_mixer(k 2^32 / (2 half)): exact integer
//      angles, +-1 and +-j exact.  EVERY butterfly multiplies, those by 1 too: one arithmetic order per output instant,
//      whatever the tile.  (Two stages are run per pass over the rows, on four points in registers: the same operations.)
//
// POSITION INDEPENDENCE.  The bits of y[c, m] depend on the T samples, the taps, phi at those samples and a(n_m) alone: a mixed
// sample's bits depend on the sample and its phi (amcx_ddc_kernel.h), a branch sum is summed in ascending q by whichever thread,
// the transform of one instant is the fixed sequence above.  A stream cut into calls at any multiple of D, with phase0 and
// sample_index0 advanced, gives the one-call result bit for bit.
//
// THE LAUNCH.  256 threads, a persistent grid over TILES of `tile` consecutive output instants (bank_tile_outputs: a power of
// two, tile C = 4096, so 16 at C = 256).  A workgroup puts the taps and the twiddles into LDS once; per tile it
//   1. stages the span's MIXED samples, (tile - 1) D + T of them, in LDS -- every input is mixed once per tile: the
//      down-converter's ddc_stage_span, with the plain image and its item loop unrolled by 4;
//   2. barrier;
//   3. sums the branches: a thread owns branch p = tid mod C of the 16 instants tid / C + j 256 / C, 16 sums in registers that
//      share every tap it reads; u[p] is written to row `instant`, column (p - a) mod C of the tile x C array;
//   4. barrier; the stages two per pass (a last one alone where log2 C is odd), a barrier behind each pass: a thread loads the
//      four points of 4 groups, computes, stores;
//   5. stores: element e is (channel e / tile, instant e mod tile), read from column bitrev(channel) -- the lanes of a wave
//      write runs of consecutive instants of a channel (tile >= 16: 128 bytes and more per run), 8-byte vector stores, no
//      atomics.  Rows of a ragged last tile that hold no instant are computed on whatever the LDS holds and never stored.
//
// LDS.  [span float2][tile rows of C + 1 float2][C float2 of twiddles][T floats of taps]; 99 456 bytes at C = 256, T = 4096,
// D = 128 and 131 072 at the most (C = 2, T = 4096), never more than 160 KiB: bank_lds_bytes, above 64 KiB through the
// attribute.
//   - the sample image has NO pad: step 3's lanes walk p, CONSECUTIVE samples downwards (conflict-free; where C < 32 the next
//     instant's lanes start D samples on: distinct or identical addresses, never a stride), and its writes walk a row's
//     columns, rotated: conflict-free;
//   - the rows' pitch is C + 1 float2, and the lanes of steps 4 and 5 walk the INSTANTS at one column: 2 (C + 1) dwords apart
//     with C + 1 odd -- the 32 lanes of a half-wave on 32 different bank pairs, conflict-free wherever tile >= 32; at
//     tile = 16 (C = 256) a half-wave holds two columns, 2-way at worst.  All lanes of a column read one twiddle.
//
// KERNEL ORDER (amcx_launch.h): plain kernels in the header amcx.hip includes FIRST; this header includes the down-converter's
// for the loaders, the mixer and the staging routine, whose kernels therefore still come first of all and keep their bytes, as does every other
// kernel: tools/codeobj_gate.py --kernels, profiles/r16_bank_codeobj_kernels.txt.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "amcx_ddc_kernel.h"

namespace amcx {

constexpr int kBankThreads = kDdcThreads;  // ddc_stage_span strides by it
constexpr int kBankMaxTaps = 4096;
constexpr int kBankMaxChannels = 256;
constexpr int kBankTileElems = 4096;       // tile * C
constexpr int kBankMinTile = 16;
constexpr int kBankWavesPerSimd = 4;       // at most 128 VGPRs: four workgroups per CU where the LDS allows them

static_assert(kBankTileElems / kBankMaxChannels >= kBankMinTile, "tile C = 4096 for every C: a thread's 16 elements rely on it");
// outputs per tile for C channels: a power of two
inline int bank_tile_outputs(int C) { return kBankTileElems / C < kBankMinTile ? kBankMinTile : kBankTileElems / C; }
__host__ __device__ __forceinline__ int bank_span(int tile, int T, int D) { return (tile - 1) * D + T; }
// bytes of the span's image, rounded up to 16: where the rows begin
__host__ __device__ __forceinline__ int bank_stage_bytes(int span) { return (8 * span + 15) / 16 * 16; }
__host__ __device__ __forceinline__ int bank_rows_bytes(int tile, int C) { return 8 * tile * (C + 1); }
inline size_t bank_lds_bytes(int T, int C, int D) {
  const int tile = bank_tile_outputs(C);
  return (size_t)bank_stage_bytes(bank_span(tile, T, D)) + (size_t)bank_rows_bytes(tile, C) + (size_t)8 * C + (size_t)4 * T;
}

constexpr int kBankPerThread = kBankTileElems / kBankThreads;        // 16: a thread's branch sums, and its outputs to store

// d * w as ddc_mix forms x * w
__device__ __forceinline__ float2 bank_mul(float2 d, float2 w) {
  return make_float2(__builtin_fmaf(d.x, w.x, -(d.y * w.y)), __builtin_fmaf(d.x, w.y, d.y * w.x));
}
__device__ __forceinline__ float2 bank_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 bank_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
// The thread index, opaque to the compiler: what a step derives from it -- 16 LDS offsets, 16 output offsets -- is then computed
// where the step uses it, not once in front of the persistent loop and kept in registers through every other step (120 of them).
__device__ __forceinline__ int bank_own(int tid) {
  asm volatile("" : "+v"(tid));
  return tid;
}

// Reads src[0 .. (M - 1) D + T) samples and taps[0 .. T), writes out[c stride + m] for c < C, m < M, nothing else.
// C = 1 << logC; a0 = sample_index0 mod C; tile = bank_tile_outputs(C); n_tiles = ceil(M / tile); dynamic LDS bank_lds_bytes.
template <class L>
__device__ __forceinline__ void bank_body(const char* __restrict__ src, float scale, unsigned flip4, unsigned long long phase0,
                                          unsigned long long phase_step, int a0, const float* __restrict__ taps, int T,
                                          int logC, int D, float2* __restrict__ out, long long out_stride, long long M, int tile,
                                          long long n_tiles) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bank_lds[];
  const int C = 1 << logC, pitch = C + 1;
  float2* const stage = reinterpret_cast<float2*>(bank_lds);
  float2* const rows = reinterpret_cast<float2*>(bank_lds + bank_stage_bytes(bank_span(tile, T, D)));
  float2* const tw = rows + tile * pitch;
  float* const h = reinterpret_cast<float*>(tw + C);
  const int tid = (int)threadIdx.x;
  for (int k = tid; k < T; k += kBankThreads) h[k] = taps[k];          // (the first tile's barrier orders these too)
  for (int e = tid; e < C; e += kBankThreads) {                         // entry half + k: exp(2 pi j k / (2 half)); entry 0 unused
    const int s = e ? 31 - __builtin_clz((unsigned)e) : 0;              // half = 1 << s
    tw[e] = ddc_mixer((unsigned)(e - (1 << s)) << (31 - s));
  }
  const int tile_shift = 31 - __builtin_clz((unsigned)tile);            // tile C = 4096: tile_shift + logC = 12
  const int di = kBankThreads >> logC;                                  // step 3: a thread's instants are di apart
  // steps 4 and 5: element e = tid + 256 n is (column or group e >> tile_shift, instant e mod tile): lanes walk the instants
  for (long long ti = blockIdx.x; ti < n_tiles; ti += gridDim.x) {
    const long long m0 = ti * tile;
    const int n_out = M - m0 < tile ? (int)(M - m0) : tile;
    const long long s0 = m0 * D;                                       // the span's first input sample
    const int span = (n_out - 1) * D + T;
    const char* const base = src + s0 * L::kBytes;
    ddc_stage_span<L, DdcPlain, 4>(stage, base, s0, span, scale, flip4, phase0, phase_step, tid);      // 1.
    __syncthreads();
    // 3. the branch sums: 16 instants of one branch in registers, every tap read once for the 16
    {
      // branch p of the instants i0 + j di (C = 256: p = tid, i = j; C = 2: 128 instants per j)
      const int t = bank_own(tid), p = t & (C - 1), i0 = t >> logC;
      float2 u[kBankPerThread];
      const float2* const v = stage + (i0 * D + T - 1 - p);             // tap p's sample of instant i0; instant i0 + j di: + j di D
      const int dv = di * D;
      if (p < T) {
        const float h0 = h[p];
#pragma unroll
        for (int j = 0; j < kBankPerThread; ++j) {
          const float2 x = v[j * dv];
          u[j] = make_float2(h0 * x.x, h0 * x.y);
        }
        for (int k = p + C; k < T; k += C) {
          const float hk = h[k];
#pragma unroll
          for (int j = 0; j < kBankPerThread; ++j) {
            const float2 x = v[j * dv - (k - p)];
            u[j] = make_float2(__builtin_fmaf(hk, x.x, u[j].x), __builtin_fmaf(hk, x.y, u[j].y));
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < kBankPerThread; ++j) u[j] = make_float2(0.0f, 0.0f);
      }
#pragma unroll
      for (int j = 0; j < kBankPerThread; ++j) {
        const int i = i0 + j * di;
        const int a = (int)(((long long)a0 + s0 + (long long)i * D + T - 1) & (C - 1));
        rows[i * pitch + ((p - a) & (C - 1))] = u[j];
      }
    }
    __syncthreads();
    // 4. two stages per pass: the points q = C >> (s + 2) apart, group g of C / 4 at j = ((g >> lq) << (lq + 2)) | k
    int s = 0;
    for (; s + 2 <= logC; s += 2) {
      const int lq = logC - s - 2, q = 1 << lq;
      float2 x0[4], x1[4], x2[4], x3[4], wa[4], wb[4], wc[4];
      int at[4];
      const int t = bank_own(tid);
#pragma unroll
      for (int n = 0; n < 4; ++n) {                                    // (C / 4) tile / 256 = 4 groups per thread
        const int e = t + n * kBankThreads, g = e >> tile_shift, k = g & (q - 1);
        at[n] = (e & (tile - 1)) * pitch + (((g >> lq) << (lq + 2)) | k);
        x0[n] = rows[at[n]];
        x1[n] = rows[at[n] + q];
        x2[n] = rows[at[n] + 2 * q];
        x3[n] = rows[at[n] + 3 * q];
        wa[n] = tw[2 * q + k];                                         // stage s, half = 2 q: the pairs (0, 2) and (1, 3)
        wb[n] = tw[2 * q + k + q];
        wc[n] = tw[q + k];                                             // stage s + 1, half = q: the pairs (0, 1) and (2, 3)
      }
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const float2 e0 = bank_add(x0[n], x2[n]), e2 = bank_mul(bank_sub(x0[n], x2[n]), wa[n]);
        const float2 e1 = bank_add(x1[n], x3[n]), e3 = bank_mul(bank_sub(x1[n], x3[n]), wb[n]);
        rows[at[n]] = bank_add(e0, e1);
        rows[at[n] + q] = bank_mul(bank_sub(e0, e1), wc[n]);
        rows[at[n] + 2 * q] = bank_add(e2, e3);
        rows[at[n] + 3 * q] = bank_mul(bank_sub(e2, e3), wc[n]);
      }
      __syncthreads();
    }
    if (s < logC) {                                                    // log2 C odd: the last stage alone, half = 1, w = 1
      float2 A[8], B[8];
      const float2 w = tw[1];
      const int t = bank_own(tid);
#pragma unroll
      for (int n = 0; n < 8; ++n) {                                    // (C / 2) tile / 256 = 8 pairs per thread
        const int e = t + n * kBankThreads;
        float2* const pair = rows + (e & (tile - 1)) * pitch + 2 * (e >> tile_shift);
        A[n] = pair[0];
        B[n] = pair[1];
      }
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        const int e = t + n * kBankThreads;
        float2* const pair = rows + (e & (tile - 1)) * pitch + 2 * (e >> tile_shift);
        pair[0] = bank_add(A[n], B[n]);
        pair[1] = bank_mul(bank_sub(A[n], B[n]), w);
      }
      __syncthreads();
    }
    // 5. a channel's run of instants per group of lanes; y[c] stands at the bit-reversed c
    {
      float2 y[kBankPerThread];
      const int t = bank_own(tid);
#pragma unroll
      for (int n = 0; n < kBankPerThread; ++n) {
        const int e = t + n * kBankThreads;
        y[n] = rows[(e & (tile - 1)) * pitch + (int)(__builtin_bitreverse32((unsigned)(e >> tile_shift)) >> (32 - logC))];
      }
#pragma unroll
      for (int n = 0; n < kBankPerThread; ++n) {
        const int e = t + n * kBankThreads, i = e & (tile - 1);
        if (i < n_out) out[(long long)(e >> tile_shift) * out_stride + m0 + i] = y[n];
      }
    }
    __syncthreads();                                                   // the next tile's staging and sums overwrite what was just read
  }
}

#define AMCX_BANK_PARAMS                                                                                                   \
  const char* __restrict__ src, float scale, unsigned flip4, unsigned long long phase0, unsigned long long phase_step, int a0, \
      const float* __restrict__ taps, int T, int logC, int D, float2* __restrict__ out, long long out_stride, long long M,   \
      int tile, long long n_tiles
#define AMCX_BANK_ARGS src, scale, flip4, phase0, phase_step, a0, taps, T, logC, D, out, out_stride, M, tile, n_tiles

__global__ __launch_bounds__(kBankThreads, kBankWavesPerSimd) void amcx_bank_c64_kernel(AMCX_BANK_PARAMS) { bank_body<DdcC64>(AMCX_BANK_ARGS); }
__global__ __launch_bounds__(kBankThreads, kBankWavesPerSimd) void amcx_bank_sc16_kernel(AMCX_BANK_PARAMS) { bank_body<DdcSc16>(AMCX_BANK_ARGS); }
__global__ __launch_bounds__(kBankThreads, kBankWavesPerSimd) void amcx_bank_iq8_kernel(AMCX_BANK_PARAMS) { bank_body<DdcIq8>(AMCX_BANK_ARGS); }

#undef AMCX_BANK_PARAMS
#undef AMCX_BANK_ARGS

}  // namespace amcx
