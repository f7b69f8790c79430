// The waveform generator (include/amcx.h, amcx_synth_c64; ABI 16.2): rows of linearly modulated IQ -- Philox symbols, a pulse at
// U / V samples per symbol, a carrier, white Gaussian noise -- written as packed complex64 in one launch.  A sibling of the
// resampler (amcx_resample_kernel.h): its sum is the resampler's with L = U, D = V on a stream of symbols that is drawn, not read,
// and the resampler's CODE: both CALL the tap image, the sum and the plan arithmetic of amcx_polyphase.h (poly_*).  The down-converter's mixer (ddc_mix,
// ddc_mixer) and its padded LDS image are CALLED too, and the training kernels' Philox4x32-10 (amcx_mlp_train_kernel.h).  r is the absolute row, n the absolute sample of the row:
//
//   counter(s, j, r) = (j & 0xFFFFFFFF, (s << 28) | (j >> 32), r low, r high)    s = 0 row, 1 symbols, 2 noise; key = the seed's words
//   W        = Philox(counter(0, 0, r))
//   phase0_r = RANDOM_PHASE ? W[0] << 32 : 0,   step_r = phase_step + (int32)W[1] * cfo_max (mod 2^64)
//   tau_r    = RANDOM_TIMING ? mulhi32(W[2], U) : tau0
//   a[k]     = table[mulhi32(Philox(counter(1, k >> 2, r))[k & 3], order)]
//   t_n      = n V + tau_r,   p_n = t_n mod U,   k_n = (P - 1) + floor(t_n / U),   P = ceil(T / U)
//   s[n]     = sum_{q >= 0, p_n + q U < T} g[p_n + q U] * a[k_n - q]             g[p_n] a[k_n], then one FMA per component, ascending q
//   v[n]     = ddc_mix(s[n], phase0_r + n * step_r)
//   X        = Philox(counter(2, n >> 1, r)),   w1 = X[2 (n & 1)],   w2 = X[2 (n & 1) + 1]
//   u        = ((w1 >> 8) + 1) * 2^-24                                           in (0, 1], exact
//   z[n]     = (sigma * sqrt(0 - ln u)) * ddc_mixer(w2)                          two products per component
//   out      = (v.re + z.re, v.im + z.im)                                        one addition per component; sigma == 0: out = v
//
// THE LOGARITHM is the device library's logf (no fast-math: the library's ordinary float32 routine, within 1 ulp as AMD states
// it; tests/synth_ref.py allows the 3 ulp of the OpenCL rule the library is built to), the square root is the correctly rounded
// sqrtf.  The noise is therefore held to a derived bound, not to ==; every integer of the contract is exact.
// SIGMA is read on the device (sigma_dev[f / frames_per_group], f the row's index in the call): the host cannot see it, so a
// NaN or a negative sigma is not refused, it PROPAGATES (NaN rows; a negative sigma is the same noise turned by half a turn).
//
// POSITION INDEPENDENCE.  Nothing above depends on the call's cut, the tile, the grid, the lane, row_stride or n_rows.
//
// THE LAUNCH.  256 threads, a persistent grid over (row, tile) pairs, a tile being `tile` consecutive samples of one row
// (syn_tile_outputs).  A workgroup puts the taps (phase-major, pitch P | 1: poly_stage_taps, as rs_body does) and the table into LDS once, barrier.  Per
// tile it draws the span's symbols -- thread t the Philox blocks t, t + 256, ... of four symbols -- into the padded image,
// barrier, then a thread takes sample PAIRS (2 i, 2 i + 1), i counted on the absolute sample index, so that one noise block
// serves both; it steps (quotient, remainder) of t_n / U with a carry as the resampler does, one division per thread and tile.
// The two samples leave as one 16-byte store where both exist and the address allows, else as 8-byte stores: an odd
// sample_index0 or a row on 8 bytes shifts the pairing of the stores, never a bit.  No atomics, nothing shared between workgroups.
//
// LDS: [span float2, padded][U phases of `pitch` floats][order float2]: 62 716 bytes at the most (syn_lds_bytes): no attribute.
//
// KERNEL ORDER (amcx_launch.h): one plain kernel in the header amcx.hip includes FIRST; it includes the training kernels' header
// and the down-converter's in front of its own kernel: tools/codeobj_gate.py --kernels, profiles/r28_synth_codeobj_kernels.txt.
// amcx_polyphase.h, behind them, holds no kernel and moves nothing; including the resampler's header here would lay its kernels out in front of this one.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "amcx_mlp_train_kernel.h"
#include "amcx_ddc_kernel.h"
#include "amcx_polyphase.h"

namespace amcx {

constexpr int kSynThreads = 256;
constexpr int kSynMaxTaps = 4096;
constexpr int kSynMaxUp = 256;
constexpr int kSynMaxDown = 4096;
constexpr int kSynMaxOrder = 256;
constexpr int kSynStage = 5120;            // most symbols of one tile's span: 5280 float2 with the pad, 42 240 bytes
constexpr int kSynMaxTile = 4096;          // most samples of one tile: 8 pairs per thread
constexpr unsigned kSynRandomPhase = 1u, kSynRandomTiming = 2u;      // AMCX_SYNTH_RANDOM_*

static_assert(kSynMaxTaps <= kSynStage, "one sample's window (U = 1) must fit the stage");

// the plan (amcx_polyphase.h) at this kernel's stage and largest tile; a tile of more than one sample is even (whole pairs)
inline int syn_tile_outputs(int T, int U, int V) {
  const int tile = poly_tile_outputs(T, U, V, kSynStage, kSynMaxTile);
  return tile > 1 ? tile & ~1 : tile;
}
inline int syn_max_span(int T, int U, int V) { return poly_max_span(T, U, V, syn_tile_outputs(T, U, V)); }
// dynamic LDS of a launch: the padded image of the worst span, the phase-major taps, the table
inline size_t syn_lds_bytes(int T, int U, int V, int order) { return (size_t)ddc_stage_bytes(syn_max_span(T, U, V)) + poly_taps_bytes(T, U) + 8u * (size_t)order; }

struct SynArgs {
  unsigned seed_lo, seed_hi;
  unsigned long long row_index0;
  long long sample_index0, n_rows, row_samples, row_stride;
  const float2* table;
  int order;
  const float* taps;
  int T, U, V, P, tau0, max_span;
  unsigned long long phase_step;
  unsigned cfo_max, flags;
  const float* sigma;
  long long frames_per_group;
  float2* out;
  int tile;
  long long tiles_per_row, n_items;
};

// s[n] of the sample whose window tops at stage index off + P - 1 with phase p: the resampler's sum (poly_taps_sum)
__device__ __forceinline__ float2 syn_pulse(const float2* stage, const float* g, int pitch, int P, int full, int off, int p) {
  const int cnt = P - (p >= full ? 1 : 0);                             // taps of phase p (0: T < U, a phase with none)
  float re = 0.0f, im = 0.0f;
  if (cnt > 0) poly_taps_sum(stage, g + p * pitch, off + P - 1, cnt, re, im);
  return make_float2(re, im);
}

// out of one sample: the carrier on s, then the noise of the words (w1, w2)
__device__ __forceinline__ float2 syn_finish(float2 s, unsigned long long phi, unsigned w1, unsigned w2, float sigma) {
  const float2 v = ddc_mix(s, phi);
  const float u = (float)((w1 >> 8) + 1u) * 0x1p-24f;
  const float amp = sigma * sqrtf(0.0f - logf(u));
  const float2 w = ddc_mixer(w2);
  const float2 o = make_float2(v.x + amp * w.x, v.y + amp * w.y);
  return sigma == 0.0f ? v : o;
}

__global__ __launch_bounds__(kSynThreads) void amcx_synth_c64_kernel(SynArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char syn_lds[];
  float2* const stage = reinterpret_cast<float2*>(syn_lds);
  float* const g = reinterpret_cast<float*>(syn_lds + ddc_stage_bytes(a.max_span));
  const int tid = (int)threadIdx.x;
  const int T = a.T, U = a.U, V = a.V, P = a.P;
  const int pitch = poly_pitch(P);
  float* const tabf = g + U * pitch;                                   // the table as floats: U pitch may be odd, 4-byte alignment
  poly_stage_taps(g, a.taps, T, U, pitch, tid, kSynThreads);
  for (int k = tid; k < 2 * a.order; k += kSynThreads) tabf[k] = reinterpret_cast<const float*>(a.table)[k];
  __syncthreads();                                                     // the first tile's DRAW reads the table other threads stored
  const int full = T - (P - 1) * U;                                    // phases p < full have P taps, the others P - 1
  const unsigned stride = 2u * (unsigned)kSynThreads * (unsigned)V;    // a thread's step of t: 256 pairs on
  const int step_q = (int)(stride / (unsigned)U), step_r = (int)(stride - (unsigned)step_q * (unsigned)U);
  const int back_q = (int)((unsigned)V / (unsigned)U), back_r = V - back_q * U;      // one sample back
  for (long long item = blockIdx.x; item < a.n_items; item += gridDim.x) {
    const long long f = item / a.tiles_per_row, ti = item - f * a.tiles_per_row;
    const unsigned long long r = a.row_index0 + (unsigned long long)f;
    const unsigned r_lo = (unsigned)r, r_hi = (unsigned)(r >> 32);
    unsigned W[4];
    philox4x32_10(0u, 0u, r_lo, r_hi, a.seed_lo, a.seed_hi, W);
    const unsigned long long phase0 = (a.flags & kSynRandomPhase) ? (unsigned long long)W[0] << 32 : 0ull;
    const unsigned long long step = a.phase_step + (unsigned long long)((long long)(int)W[1] * (long long)a.cfo_max);
    const int tau = (a.flags & kSynRandomTiming) ? (int)__umulhi(W[2], (unsigned)U) : a.tau0;
    const float sigma = a.sigma[f / a.frames_per_group];

    const long long o0 = ti * a.tile;                                  // the tile's first sample, in the call's row
    const int n_out = a.row_samples - o0 < a.tile ? (int)(a.row_samples - o0) : a.tile;
    const long long n0 = a.sample_index0 + o0;                         // ... and absolute
    const long long t0 = n0 * V + tau;
    const long long s0 = t0 / U;                                       // the span's first symbol
    const int r0 = (int)(t0 - s0 * U);
    const int span = (int)(((unsigned)(n_out - 1) * (unsigned)V + (unsigned)r0) / (unsigned)U) + P;
    if (a.order > 0) {
      const long long b0 = s0 >> 2;
      const int n_blocks = (int)(((s0 + span - 1) >> 2) - b0) + 1;
      for (int b = tid; b < n_blocks; b += kSynThreads) {
        const unsigned long long j = (unsigned long long)(b0 + b);
        unsigned X[4];
        philox4x32_10((unsigned)j, (1u << 28) | (unsigned)(j >> 32), r_lo, r_hi, a.seed_lo, a.seed_hi, X);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const long long i = (long long)(j << 2) + c - s0;             // the symbol's place in the span
          if (i >= 0 && i < span) {
            const unsigned idx = __umulhi(X[c], (unsigned)a.order);
            stage[ddc_pad((int)i)] = make_float2(tabf[2 * idx], tabf[2 * idx + 1]);
          }
        }
      }
    }
    __syncthreads();
    // pairs (2 i, 2 i + 1) of absolute samples; this thread's first pair holds the tile's samples oA, oA + 1, oA = -1 where n0 is odd
    float2* const row_out = a.out + f * a.row_stride + o0;
    const int odd = (int)(n0 & 1);
    const unsigned uB = (unsigned)(2 * tid + 1 - odd) * (unsigned)V + (unsigned)r0;   // the one division of this thread and tile
    int offB = (int)(uB / (unsigned)U), pB = (int)(uB - (unsigned)offB * (unsigned)U);
    for (int oA = 2 * tid - odd; oA < n_out; oA += 2 * kSynThreads) {
      const bool hasA = oA >= 0, hasB = oA + 1 < n_out;
      const unsigned long long nA = (unsigned long long)(n0 + oA), jn = nA >> 1;
      unsigned X[4];
      philox4x32_10((unsigned)jn, (2u << 28) | (unsigned)(jn >> 32), r_lo, r_hi, a.seed_lo, a.seed_hi, X);
      float2 yA = make_float2(0.0f, 0.0f), yB = yA;
      if (hasA) {
        int offA = offB - back_q, pA = pB - back_r;
        if (pA < 0) { pA += U; --offA; }
        const float2 s = a.order > 0 ? syn_pulse(stage, g, pitch, P, full, offA, pA) : make_float2(0.0f, 0.0f);
        yA = syn_finish(s, phase0 + nA * step, X[0], X[1], sigma);
      }
      if (hasB) {
        const float2 s = a.order > 0 ? syn_pulse(stage, g, pitch, P, full, offB, pB) : make_float2(0.0f, 0.0f);
        yB = syn_finish(s, phase0 + (nA + 1ull) * step, X[2], X[3], sigma);
      }
      float2* const dst = row_out + oA;
      if (hasA && hasB && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
        *reinterpret_cast<float4*>(dst) = make_float4(yA.x, yA.y, yB.x, yB.y);
      } else {
        if (hasA) dst[0] = yA;
        if (hasB) dst[1] = yB;
      }
      offB += step_q;
      pB += step_r;
      if (pB >= U) { pB -= U; ++offB; }
    }
    __syncthreads();                                                   // the next tile's symbols overwrite what was just read
  }
}

}  // namespace amcx
