// The Welch spectrogram of a raw stream and its per-row detection (include/amcx.h, amcx_spectrogram / amcx_psd_detect_f32;
// ABI 15): from one contiguous stream of complex64 / sc16 / ci8 / cu8 samples to float32 power rows (R, nfft), and from such
// rows to a noise floor per row and a mask of the occupied bins.
//
//   xw_s[n] = w[n] * x[s hop + n]                                   one float32 product per component
//   X_s[b]  = sum_{n < nfft} xw_s[n] exp(-2 pi j b n / nfft)         b = 0 ... nfft - 1, FFT order
//   P[r, b] = sum_{a < A} |X_{r A + a}[b]|^2                         r < R = floor(nseg / A), nseg = floor((S - nfft) / hop) + 1
//
// No normalisation: 1 / (A sum w^2) is the caller's.  x[n] is what ABI 9 / 10 say -- (float)integer * scale, ONE float32
// multiplication per component -- whichever load brought it in, so the rows of an integer stream are the bits of the complex64
// call on the widened samples.
//
// THE OPERATION SEQUENCE, which depends on nfft alone (L = log2 nfft; tests/psd_ref.py restates it in numpy float32):
//   table   tw[k] = ddc_mixer((0 - k) << 20), k < 2048: exp(-2 pi j k / 4096) at an exact integer angle -- tw[0] = 1 + 0j and
//           tw[1024] = 0 - 1j exactly.
//   stages  radix-2 decimation in frequency, in place, l = 0 ... L - 1 with h = nfft >> (l + 1).  For every block base
//           i0 = 2 h m and j < h:
//               u = v[i0 + j],  d = v[i0 + j + h]
//               v[i0 + j]     = (u.re + d.re, u.im + d.im)
//               v[i0 + j + h] = mul((u.re - d.re, u.im - d.im), tw[j * (2048 / h)])
//               mul(d, w) = (fma(d.re, w.re, -(d.im * w.im)), fma(d.re, w.im, d.im * w.re))          -- as bank_mul forms it
//           EVERY butterfly multiplies, also by tw[0] = 1.  X[b] then stands at the bit-reversed b.
//   power   p_a = fma(X.im, X.im, X.re * X.re);   P = ((p_0 + p_1) + p_2) + ... in ascending a.
// The kernel runs the stages K = 3 or 4 at a time in registers (a thread holds the 8 or 16 points that K consecutive stages'
// butterflies connect; the arithmetic is that of the K radix-2 stages, operation for operation) with one exchange through LDS
// between such passes: ceil(L / 4) passes, the shorter ones first -- 3 + 3 at nfft = 64, 3 + 4 at 128, 4 + 4 at 256,
// 3 + 3 + 3 at 512, 3 + 3 + 4 at 1024, 3 + 4 + 4 at 2048, 4 + 4 + 4 at 4096.  (The first version ran them two per barrier:
// HISTORY.md, round 22.)
//
// POSITION INDEPENDENCE.  A row's bits depend on its (A - 1) hop + nfft samples and the window alone.  Every segment goes
// through the same sequence wherever it stands: a SLOT g of a pass holds one segment in the points [g nfft, (g + 1) nfft), and
// the twiddle of a butterfly depends on j alone.  A sample's bits do not depend on the load that brought it in (16-byte items
// from the segment's first 16-byte boundary on, one sample per step in front of it and behind the last whole item: any
// sample-aligned address).  Hence a stream cut into calls after any whole number of rows gives the one-call rows bit for bit.
//
// THE LAUNCH.  256 threads, a persistent grid over PASSES.  A workgroup holds kPsdPoints = 4096 points at a time: G = 4096 /
// nfft segments of G DIFFERENT consecutive rows (one segment at nfft = 4096).  Per pass it walks a = 0 ... A - 1: stage the G
// segments' windowed samples (256 / G threads each), transform, and every thread adds the power of its own 16 points to 16
// registers; after the last a the sums go through LDS into FFT order and out in runs of consecutive bins (4-byte vector
// stores, consecutive lanes consecutive addresses).  Slots whose row is beyond the call's rows are idle: nothing is read for
// them and nothing stored.  The window is read from global memory (nfft floats, cached); the table is built once per
// workgroup.  LDS: 34 KiB of points (with the pad below) + 16 KiB of table = 50 KiB, static: no attribute.  No atomics, no
// spin loop, nothing shared between workgroups: capturable in a graph.
//
// LDS BANKS.  A float2 access of 64 lanes is served in two halves of 32 lanes x 8 bytes = the 64 banks once; a half-wave is
// conflict-free when its 32 float2 indices are distinct mod 32.  Point i lives at float2 index i + (i >> 4) (psd_pad).  A
// pass whose points are q apart reads and writes v[i + m q], m < 2^K, with i consecutive over the lanes where q >= 32:
// the padded indices of a half-wave are a ... a + 15 and a + 17 ... a + 32, ONE pair of lanes on one bank.  The last pass
// has q = 1: lane l holds the points 2^K l ..., and without the pad all 32 lanes would meet on one or two banks; with it a
// 16-point pass has the lanes 17 apart -- distinct mod 32, no conflict (nfft = 128, 256, 1024, 2048, 4096) --, an 8-point
// last pass (nfft = 64, 512) 8.5 apart, 2-way.  Passes in between (q = 8, 16) cover 32 / q blocks per half-wave and are 2-way
// where a block's padded size is not 16 mod 32.  Staging and the power read touch consecutive points from consecutive lanes.
// Table reads are broadcasts or strided reads of a 16 KiB table: in the last pass a half-wave reads few distinct entries.
// The transpose into FFT order writes one float per lane at bit-reversed offsets (up to 16-way on the top bits, once per
// row) and reads back consecutive floats.
//
// THE DETECTION (amcx_psd_detect_kernel).  One workgroup per spectrogram row at a time, the row's `bins` keys (occ_key of
// amcx_occupancy_kernels.h) in LDS, 16 KiB at 4096 bins.  floor[r] = the value of rank `rank` among them, NaN last, by
// bisection on the keys from bit 31 down (the occupancy floor kernel's method: the largest x with #{key < x} <= rank is that
// element's key); a step counts a thread's keys, sums the wave with shuffles and the four waves through LDS, one barrier per
// step, the partials double-buffered.  Then mask[r, b] = P[r, b] > threshold * floor[r] ? 1 : 0: ONE float32 product, one
// comparison, so a NaN is not occupied.  Any 2 <= bins <= 4096.
//
// KERNEL ORDER (amcx_launch.h): the header amcx.hip includes FIRST, in front of the occupancy kernels': every kernel that was
// there keeps its bytes (tools/codeobj_gate.py --kernels, profiles/r22_psd_codeobj_kernels.txt).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "amcx_occupancy_kernels.h"   // occ_key / occ_unkey
#include "amcx_ddc_kernel.h"          // the loaders DdcC64 / DdcSc16 / DdcIq8, ddc_mixer

namespace amcx {

constexpr int kPsdThreads = 256;
constexpr int kPsdPoints = 4096;                        // points a workgroup holds: kPsdPoints / nfft segments
constexpr int kPsdPerThread = kPsdPoints / kPsdThreads;
constexpr int kPsdMinFft = 64, kPsdMaxFft = 4096;
constexpr int kPsdMaxHop = 65536, kPsdMaxAverages = 65536;
constexpr int kPsdMaxBins = 4096;
constexpr int kPsdPadPoints = kPsdPoints + kPsdPoints / 16;          // with the pad of LDS BANKS
constexpr int kPsdLdsBytes = kPsdPadPoints * 8 + (kPsdPoints / 2) * 8;

__host__ __device__ __forceinline__ int psd_pad(int i) { return i + (i >> 4); }

__device__ __forceinline__ float2 psd_mul(float2 d, float2 w) {
  return make_float2(__builtin_fmaf(d.x, w.x, -(d.y * w.y)), __builtin_fmaf(d.x, w.y, d.y * w.x));
}
__device__ __forceinline__ float2 psd_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 psd_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

// The `sub` threads of a slot (t = 0 ... sub - 1) read the nfft samples from `base` on and nothing else, and store sample n
// times w[n] as point p0 + n.  Items of 16 bytes from the first 16-byte boundary on; single samples in front and behind.
template <class L>
__device__ __forceinline__ void psd_stage_segment(float2* pts, int p0, const char* __restrict__ base, const float* __restrict__ w,
                                                  int nfft, float scale, unsigned flip4, int t, int sub) {
  int head = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(base) & 15u)) & 15u) / L::kBytes;
  if (head > nfft) head = nfft;
  const int items = (nfft - head) / L::kItem;
  const int tail0 = head + items * L::kItem;
  for (int i = t; i < head; i += sub) {
    const float2 x = L::one(base + (size_t)i * L::kBytes, scale, flip4);
    const float wi = w[i];
    pts[psd_pad(p0 + i)] = make_float2(wi * x.x, wi * x.y);
  }
  for (int it = t; it < items; it += sub) {
    const int i0 = head + it * L::kItem;
    float2 x[L::kItem];
    L::item(base + (size_t)i0 * L::kBytes, scale, flip4, x);
#pragma unroll
    for (int j = 0; j < L::kItem; ++j) {
      const float wi = w[i0 + j];
      pts[psd_pad(p0 + i0 + j)] = make_float2(wi * x[j].x, wi * x[j].y);
    }
  }
  for (int i = tail0 + t; i < nfft; i += sub) {
    const float2 x = L::one(base + (size_t)i * L::kBytes, scale, flip4);
    const float wi = w[i];
    pts[psd_pad(p0 + i)] = make_float2(wi * x.x, wi * x.y);
  }
}

// K consecutive stages, the first on blocks of 2^lB points, on all kPsdPoints points: a thread takes the 2^K points i + m q,
// q = 2^(lB - K), of a block into registers, runs the K stages' butterflies among them (THE OPERATION SEQUENCE: the
// butterfly of the points at m and m + half, half = 2^(K - 1 - s) in stage s, has j = (i mod q) + m q) and puts them back.
template <int K>
__device__ __forceinline__ void psd_pass(float2* pts, const float2* tw, int lB, int tid) {
  constexpr int P = 1 << K;
  const int lq = lB - K, q = 1 << lq;
#pragma unroll
  for (int g = 0; g < kPsdPerThread / P; ++g) {
    const int idx = tid + g * kPsdThreads;             // one of the kPsdPoints / P groups
    const int j = idx & (q - 1);
    const int i = ((idx >> lq) << lB) + j;
    float2 x[P];
#pragma unroll
    for (int m = 0; m < P; ++m) x[m] = pts[psd_pad(i + (m << lq))];
#pragma unroll
    for (int s = 0; s < K; ++s) {
      const int half = P >> (s + 1);
      const int sh = 11 - (lB - s - 1);                // tw's index of position j in a half of 2^(lB - s - 1) points: j << sh
#pragma unroll
      for (int m = 0; m < half; ++m) {
        const float2 w = tw[(j + (m << lq)) << sh];
#pragma unroll
        for (int b = 0; b < P; b += 2 * half) {
          const float2 u = x[b + m], d = x[b + m + half];
          x[b + m] = psd_add(u, d);
          x[b + m + half] = psd_mul(psd_sub(u, d), w);
        }
      }
    }
#pragma unroll
    for (int m = 0; m < P; ++m) pts[psd_pad(i + (m << lq))] = x[m];
  }
}

// Reads src[(r A + a) hop + n], n < nfft, a < A, r < R, and window[0 .. nfft); writes out[r stride + b], b < nfft; nothing else.
// lg = log2 nfft; n_passes = ceil(R / (kPsdPoints / nfft)).
template <class L>
__device__ __forceinline__ void psd_body(const char* __restrict__ src, float scale, unsigned flip4, const float* __restrict__ window,
                                         int nfft, int lg, int hop, int A, float* __restrict__ out, long long stride, long long R,
                                         long long n_passes) {
  __shared__ __attribute__((aligned(16))) float2 psd_pts[kPsdPadPoints];
  __shared__ __attribute__((aligned(16))) float2 psd_tw[kPsdPoints / 2];
  const int tid = (int)threadIdx.x;
  for (int k = tid; k < kPsdPoints / 2; k += kPsdThreads) psd_tw[k] = ddc_mixer((0u - (unsigned)k) << 20);
  const int G = kPsdPoints >> lg;                      // slots of a pass: 1 ... 64
  const int sub = kPsdThreads / G;                     // threads that stage one slot: 256 ... 4
  const int slot = tid / sub, t_in = tid - slot * sub;
  for (long long pass = blockIdx.x; pass < n_passes; pass += gridDim.x) {
    const long long r0 = pass * G;
    const bool live = r0 + slot < R;
    float acc[kPsdPerThread] = {};
    for (int a = 0; a < A; ++a) {
      if (live) {
        const long long s0 = ((r0 + slot) * A + a) * (long long)hop;
        psd_stage_segment<L>(psd_pts, slot << lg, src + s0 * L::kBytes, window, nfft, scale, flip4, t_in, sub);
      }
      __syncthreads();                                 // (also orders the table in front of the first stage)
      int lB = lg;                                     // stages left; the next one's blocks have 2^lB points
      for (int left = (lg + 3) >> 2; left > 0; --left) {
        const int K = lB / left;                       // 3 or 4: the shorter passes first
        if (K == 4) psd_pass<4>(psd_pts, psd_tw, lB, tid);
        else psd_pass<3>(psd_pts, psd_tw, lB, tid);
        lB -= K;
        __syncthreads();
      }
#pragma unroll
      for (int k = 0; k < kPsdPerThread; ++k) {
        const float2 X = psd_pts[psd_pad(tid + k * kPsdThreads)];
        const float p = __builtin_fmaf(X.y, X.y, X.x * X.x);
        acc[k] = a == 0 ? p : acc[k] + p;
      }
      __syncthreads();                                 // the next segment's staging overwrites what was just read
    }
    // into FFT order through LDS, then out in runs of consecutive bins
    float* const rows = reinterpret_cast<float*>(psd_pts);
#pragma unroll
    for (int k = 0; k < kPsdPerThread; ++k) {
      const int p = tid + k * kPsdThreads;
      const int n = p & (nfft - 1);
      rows[(p - n) + (int)(__brev((unsigned)n) >> (32 - lg))] = acc[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPsdPerThread; ++k) {
      const int p = tid + k * kPsdThreads;
      const long long r = r0 + (p >> lg);
      if (r < R) out[r * stride + (p & (nfft - 1))] = rows[p];
    }
    __syncthreads();
  }
}

#define AMCX_PSD_PARAMS                                                                                                       \
  const char* __restrict__ src, float scale, unsigned flip4, const float* __restrict__ window, int nfft, int lg, int hop, int A, \
      float* __restrict__ out, long long stride, long long R, long long n_passes
#define AMCX_PSD_ARGS src, scale, flip4, window, nfft, lg, hop, A, out, stride, R, n_passes

__global__ __launch_bounds__(kPsdThreads) void amcx_spectrogram_c64_kernel(AMCX_PSD_PARAMS) { psd_body<DdcC64>(AMCX_PSD_ARGS); }
__global__ __launch_bounds__(kPsdThreads) void amcx_spectrogram_sc16_kernel(AMCX_PSD_PARAMS) { psd_body<DdcSc16>(AMCX_PSD_ARGS); }
__global__ __launch_bounds__(kPsdThreads) void amcx_spectrogram_iq8_kernel(AMCX_PSD_PARAMS) { psd_body<DdcIq8>(AMCX_PSD_ARGS); }

#undef AMCX_PSD_PARAMS
#undef AMCX_PSD_ARGS

// Reads psd[r stride + b], b < bins, r < n_rows; writes floor_out[r] and, where mask is given, mask[r bins + b]; nothing else.
// 2 <= bins <= kPsdMaxBins, 0 <= rank < bins.
__global__ __launch_bounds__(kPsdThreads) void amcx_psd_detect_kernel(const float* __restrict__ psd, long long n_rows, int bins,
                                                                      long long stride, int rank, float threshold,
                                                                      float* __restrict__ floor_out, unsigned char* __restrict__ mask) {
  __shared__ unsigned keys[kPsdMaxBins];
  __shared__ int part[2][kPsdThreads / 64];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (long long r = blockIdx.x; r < n_rows; r += gridDim.x) {
    const float* const row = psd + r * stride;
    for (int b = tid; b < bins; b += kPsdThreads) keys[b] = occ_key(row[b]);
    __syncthreads();
    unsigned ans = 0;
    for (int bit = 31; bit >= 0; --bit) {
      const unsigned cand = ans | (1u << bit);
      int below = 0;
      for (int b = tid; b < bins; b += kPsdThreads) below += keys[b] < cand ? 1 : 0;
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) below += __shfl_xor(below, d, 64);
      int* const mine = part[bit & 1];
      if (lane == 0) mine[wave] = below;
      __syncthreads();
      const int total = (mine[0] + mine[1]) + (mine[2] + mine[3]);
      if (total <= rank) ans = cand;                                  // (every thread decides the same: the same four partials)
    }
    const float fl = occ_unkey(ans);
    if (tid == 0) floor_out[r] = fl;
    if (mask != nullptr) {
      const float limit = threshold * fl;
      for (int b = tid; b < bins; b += kPsdThreads) mask[r * bins + b] = row[b] > limit ? 1 : 0;
    }
    __syncthreads();                                                  // the next row's keys overwrite what was just counted
  }
}

}  // namespace amcx
