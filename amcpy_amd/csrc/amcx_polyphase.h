// What the two polyphase kernels share and no kernel of: the resampler (amcx_resample_kernel.h) and the waveform generator
// (amcx_synth_kernel.h: L = U, D = V, drawn symbols) are ONE sum over a phase-major tap image in LDS and the down-converter's padded
// image of samples, in tiles whose worst span fits a stage.  The tap image, the sum and the plan arithmetic stand here once, so "the
// same bits as the resampler" holds by construction.  No kernel stands here, and both users include the down-converter's header
// (ddc_pad) in front of this one already: including it moves nothing in .text (KERNEL ORDER, amcx_launch.h).
#pragma once

#include "amcx_ddc_kernel.h"

namespace amcx {

__host__ __device__ __forceinline__ int poly_pitch(int P) { return P | 1; }
// The taps PHASE-MAJOR, g[p * pitch + q] = h[p + q L] (amcx_resample_kernel.h says why, and why the pitch is odd), by the `threads`
// threads of a workgroup; entries with p + q L >= T are never written or read.  The caller's barrier orders it.
__device__ __forceinline__ void poly_stage_taps(float* g, const float* taps, int T, int L, int pitch, int tid, int threads) {
  for (int k = tid; k < T; k += threads) {
    const int q = (int)((unsigned)k / (unsigned)L);
    g[(k - q * L) * pitch + q] = taps[k];
  }
}

// ONE ORDER: the sum of a phase with cnt >= 1 taps gp[0 .. cnt) whose window tops at stage index `top`, into (re, im): gp[0] *
// stage[top], then one FMA per component in ascending q.  The branch on cnt stays in the caller (a phase with no tap is +0 + 0j),
// and the sum leaves by reference: returned as float2, or with the branch in here, the callers' kernels change their bytes.
__device__ __forceinline__ void poly_taps_sum(const float2* stage, const float* gp, int top, int cnt, float& re, float& im) {
  const float2 v0 = stage[ddc_pad(top)];
  const float h0 = gp[0];
  re = h0 * v0.x;
  im = h0 * v0.y;
#pragma unroll 4
  for (int q = 1; q < cnt; ++q) {
    const float2 v = stage[ddc_pad(top - q)];
    const float hq = gp[q];
    re = __builtin_fmaf(hq, v.x, re);
    im = __builtin_fmaf(hq, v.y, im);
  }
}

// The plan, on the host: T taps, L phases, a step of D per output, a stage of `stage` samples, at most `max_tile` outputs a tile:
// as many as the stage holds the worst span of, floor(((tile - 1) D + L - 1) / L) + P at remainder L - 1; at least one
inline int poly_phase_taps(int T, int L) { return (T + L - 1) / L; }                     // P: taps of the longest phase
inline int poly_tile_outputs(int T, int L, int D, int stage, int max_tile) {
  const long long fit = (long long)(stage - poly_phase_taps(T, L)) * L / D + 1;
  return fit > max_tile ? max_tile : (int)fit;
}
// most samples a tile of `tile` outputs stages; bytes of the tap image (L pitch <= T + 2 L <= 4608 floats)
inline int poly_max_span(int T, int L, int D, int tile) { return (int)(((long long)(tile - 1) * D + L - 1) / L) + poly_phase_taps(T, L); }
inline size_t poly_taps_bytes(int T, int L) { return (size_t)4 * (size_t)L * (size_t)poly_pitch(poly_phase_taps(T, L)); }

}  // namespace amcx
