// The rational resampler (include/amcx.h, amcx_resample; ABI 13): mixer, polyphase real FIR, rate change by L / D, from one
// contiguous stream of complex64 / sc16 / ci8 / cu8 samples to packed complex64.  A sibling of the down-converter
// (amcx_ddc_kernel.h): its mixer (ddc_mix), its loaders (Ddc*) and its staging routine (ddc_stage_span) are CALLED here, and
// so are the tap image, the sum and the plan arithmetic it shares with the waveform generator (amcx_polyphase.h: poly_*).
//
//   phi(n) = phase0 + n * phase_step                  (uint64, exact; n counts the call's input samples)
//   v[n]   = x[n] * exp(+2 pi j phi(n) / 2^64)
//   P      = ceil(T / L)                              taps of the longest phase
//   t_m    = m D + tau0                               tau0 = phase_index0, 0 <= tau0 < L: the first output's phase
//   p_m    = t_m mod L,   n_m = (P - 1) + floor(t_m / L)
//   y[m]   = sum_{q >= 0, p_m + q L < T} h[p_m + q L] * v[n_m - q]
//
// i.e. v zero-stuffed by L, filtered with the T taps (given at the upsampled rate), every D-th result kept -- nothing is ever
// zero-stuffed.  No gain is applied: the taps carry it.  A phase with no tap at all (p_m >= T) is +0 + 0j; a tap index >= T does
// not exist: it is never read, and no sample enters a sum for it (the span is STAGED whole: the oldest sample of a phase one tap
// short, the samples between two windows where D > P L are loaded and mixed -- all inside the stream -- and never multiplied).
//
// ONE ORDER.  y[m] is h[p] v[n_m] and then one FMA per component in ascending q, whichever thread of whichever tile sums it, on
// mixed samples whose bits depend on the sample and its phi alone (amcx_ddc_kernel.h).  With L = 1 that is the order k = 0 ...
// T - 1 of the down-converter: the same bits.  A stream cut after any whole number of outputs, continued with
// floor((M D + tau0) / L) inputs dropped, tau0' = (M D + tau0) mod L and phase0 advanced, gives the one-call result bit for bit.
//
// THE LAUNCH.  256 threads, a persistent grid over TILES of `tile` consecutive outputs (rs_tile_outputs: as many as the stage
// holds the worst span of, 4096 at the most -- L = 256, D = 1 would otherwise be a million).  A workgroup puts the taps into LDS
// once; per tile it stages the span's MIXED samples (ddc_stage_span, the padded image), barrier, then thread t sums the
// outputs t, t + 256, ... of the tile and stores them (8-byte vector stores, consecutive lanes consecutive outputs), barrier.
// A tile's first input is s0 = floor((m0 D + tau0) / L) in 64-bit, once per tile; inside the tile output o sits at
// u = o D + r0, r0 = (m0 D + tau0) mod L: phase u mod L, window top (P - 1) + u / L relative to s0.  A thread divides ONCE per
// tile (its first output) and then steps u by 256 D as (quotient, remainder) with a carry: no division per output, nothing in
// 64-bit.  u < kRsStage * 256 + 256 fits 32 bits by far.
//
// LDS: [span float2, the down-converter's pad][L phases of `pitch` floats]; 64 896 bytes at the most (rs_lds_bytes): no attribute.
//   - samples: index i + (i >> 5), the down-converter's padded image (DdcPadded).  Neighbouring lanes read D / L samples
//     apart: the same sample (a broadcast) or a near one for every ratio below 1, the down-converter's pattern at L = 1.
//   - taps: PHASE-MAJOR, g[p * pitch + q] = h[p + q L], pitch = P | 1.  The lanes of a half-wave are at one q and at phases
//     (r0 + o D) mod L; tap reads are 4 bytes, bank (a / 4) mod 32, so with an odd pitch p -> bank is one-to-one mod 32: two
//     lanes meet on a bank only where their phases are equal (a broadcast) or 32 apart, the least a table of one tap per dword
//     allows.  (Tap-major, pitch L, would put D = L / 2 ... on two banks.)  Entries with p + q L >= T are never written or read.
//
// KERNEL ORDER (amcx_launch.h): plain kernels in the header amcx.hip includes FIRST; this header includes the down-converter's,
// whose kernels therefore still come first of all and keep their bytes, as does every other kernel: tools/codeobj_gate.py
// --kernels, profiles/r17_resample_codeobj_kernels.txt.  amcx_polyphase.h, included behind it, holds no kernel: nothing moves.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "amcx_ddc_kernel.h"
#include "amcx_polyphase.h"

namespace amcx {

constexpr int kRsThreads = kDdcThreads;     // ddc_stage_span strides by it
constexpr int kRsMaxTaps = 4096;
constexpr int kRsMaxInterp = 256;
constexpr int kRsMaxDecim = 4096;
constexpr int kRsStage = 5632;             // most samples of one tile's span: 5808 float2 with the pad, 46 464 bytes
constexpr int kRsMaxTile = 4096;           // most outputs of one tile: 16 per thread

static_assert(kRsMaxTaps <= kRsStage, "one output's window (L = 1) must fit the stage");

inline int rs_tile_outputs(int T, int L, int D) { return poly_tile_outputs(T, L, D, kRsStage, kRsMaxTile); }   // the plan: amcx_polyphase.h
inline int rs_max_span(int T, int L, int D) { return poly_max_span(T, L, D, rs_tile_outputs(T, L, D)); }      // most samples any tile stages
// dynamic LDS of a launch: the padded image of the worst span, then the phase-major taps
inline size_t rs_lds_bytes(int T, int L, int D) { return (size_t)ddc_stage_bytes(rs_max_span(T, L, D)) + poly_taps_bytes(T, L); }

// Reads src[0 .. n_{M-1}] samples and taps[0 .. T), writes out[0 .. M), nothing else.  P = ceil(T / L); max_span =
// rs_max_span; n_tiles = ceil(M / tile); the dynamic LDS is rs_lds_bytes(T, L, D).
template <class Ld>
__device__ __forceinline__ void rs_body(const char* __restrict__ src, float scale, unsigned flip4, unsigned long long phase0,
                                        unsigned long long phase_step, const float* __restrict__ taps, int T, int L, int D,
                                        int tau0, int P, int max_span, float2* __restrict__ out, long long M, int tile,
                                        long long n_tiles) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rs_lds[];
  float2* const stage = reinterpret_cast<float2*>(rs_lds);
  float* const g = reinterpret_cast<float*>(rs_lds + ddc_stage_bytes(max_span));
  const int tid = (int)threadIdx.x;
  const int pitch = poly_pitch(P);
  poly_stage_taps(g, taps, T, L, pitch, tid, kRsThreads);             // (the first tile's barrier orders these too)
  const int full = T - (P - 1) * L;                                    // phases p < full have P taps, the others P - 1
  const unsigned stride = (unsigned)kRsThreads * (unsigned)D;          // a thread's step of u, as quotient and remainder
  const int step_q = (int)(stride / (unsigned)L), step_r = (int)(stride - (unsigned)step_q * (unsigned)L);
  for (long long ti = blockIdx.x; ti < n_tiles; ti += gridDim.x) {
    const long long m0 = ti * tile;
    const int n_out = M - m0 < tile ? (int)(M - m0) : tile;
    const long long t0 = m0 * D + tau0;
    const long long s0 = t0 / L;                                       // the span's first input sample
    const int r0 = (int)(t0 - s0 * L);
    const int span = (int)(((unsigned)(n_out - 1) * (unsigned)D + (unsigned)r0) / (unsigned)L) + P;
    const char* const base = src + s0 * Ld::kBytes;
    ddc_stage_span<Ld, DdcPadded, 1>(stage, base, s0, span, scale, flip4, phase0, phase_step, tid);
    __syncthreads();
    const unsigned u = (unsigned)tid * (unsigned)D + (unsigned)r0;     // the one division of this thread and tile
    int off = (int)(u / (unsigned)L), p = (int)(u - (unsigned)off * (unsigned)L);
    for (int o = tid; o < n_out; o += kRsThreads) {
      const int cnt = P - (p >= full ? 1 : 0);                         // taps of phase p (0: T < L, a phase with none)
      float re = 0.0f, im = 0.0f;
      if (cnt > 0) {
        const int top = off + P - 1;                                   // the sample tap p multiplies
        const float* const gp = g + p * pitch;
        poly_taps_sum(stage, gp, top, cnt, re, im);
      }
      out[m0 + o] = make_float2(re, im);
      off += step_q;
      p += step_r;
      if (p >= L) { p -= L; ++off; }
    }
    __syncthreads();                                                   // the next tile's staging overwrites what was just read
  }
}

#define AMCX_RS_PARAMS                                                                                                   \
  const char* __restrict__ src, float scale, unsigned flip4, unsigned long long phase0, unsigned long long phase_step,   \
      const float* __restrict__ taps, int T, int L, int D, int tau0, int P, int max_span, float2* __restrict__ out,      \
      long long M, int tile, long long n_tiles
#define AMCX_RS_ARGS src, scale, flip4, phase0, phase_step, taps, T, L, D, tau0, P, max_span, out, M, tile, n_tiles

__global__ __launch_bounds__(kRsThreads) void amcx_resample_c64_kernel(AMCX_RS_PARAMS) { rs_body<DdcC64>(AMCX_RS_ARGS); }
__global__ __launch_bounds__(kRsThreads) void amcx_resample_sc16_kernel(AMCX_RS_PARAMS) { rs_body<DdcSc16>(AMCX_RS_ARGS); }
__global__ __launch_bounds__(kRsThreads) void amcx_resample_iq8_kernel(AMCX_RS_PARAMS) { rs_body<DdcIq8>(AMCX_RS_ARGS); }

#undef AMCX_RS_PARAMS
#undef AMCX_RS_ARGS

}  // namespace amcx
