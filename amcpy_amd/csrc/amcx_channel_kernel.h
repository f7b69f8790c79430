// The fading multipath channel (include/amcx.h, amcx_channel_c64; ABI 16.2.1): rows of complex64 through a time-varying tapped
// delay line -- per path a sum-of-sinusoids Rayleigh gain (Jakes Doppler spectrum) plus a line-of-sight term, optionally the
// generator's white noise -- written as packed complex64 in one launch.  A sibling of the generator (amcx_synth_kernel.h): its
// Philox key and counter layout with the new stream number 3, its noise finish syn_finish CALLED, not restated (with phase 0
// its mixer returns its input), the down-converter's mixer ddc_mixer and its staging routine ddc_stage_span CALLED too.
// r is the absolute row, n the absolute output sample, L paths, S sinusoids, B = 2^b (b = interp_log2), H the largest delay:
//
//   X        = Philox(counter(3, 32 l + s, r))          XL = Philox(counter(3, 512 + l, r))
//   phase0   = X[0] << 32,   ci = (int64)(ddc_mixer(X[1]).x * 2^31),   step = ci * doppler_max (mod 2^64)
//   los      : phase0 = RANDOM_PHASE ? XL[0] << 32 : 0,   step = (int64)los_doppler_q31 * doppler_max
//   d[k]     = sum_s ddc_mixer(top32(phase0_ls + k B step_ls))           ascending s, from the s = 0 value, one addition per component
//   G_l[k]   = fma(los_gain, w[k], diffuse_gain * d[k])                  per component, w the line of sight's mixer value at k B
//   c_l[n]   = fma(f, G_l[k + 1] - G_l[k], G_l[k])                       k = n >> b,  f = (float)(n & (B - 1)) * 2^-b
//   acc      = c_0 x_0, then per later path four FMAs (re by c.re, re by -c.im, im by c.re, im by c.im);  x_l = in[i + H - delay_l]
//   out      = syn_finish(acc, 0, w1, w2, sigma)                         the generator's stream-2 words of (r, n)
//
// POSITION INDEPENDENCE.  Nothing above depends on the call's cut, the tile, the grid, the lane or the strides.
//
// THE LAUNCH.  256 threads, A PLAIN GRID, not persistent_grid: one workgroup per (row, tile), a tile being `tile` consecutive
// outputs of one row (chan_tile_outputs).  Nothing is worth keeping across items -- the path table is 256 bytes of kernel
// arguments and the draws change with the row -- and a plain grid adds no call site to the table of persistent launches
// (tests/persistent_loops.py), which every grid-stride loop has to be entered in.  Per workgroup: the L S + L (phase0, step) pairs,
// one Philox block each, spread over the threads into LDS, barrier; the tile's node gains, chan_nodes(tile, b) at most per path,
// spread over the threads into LDS; the tile's tile + H input samples staged by ddc_stage_span<DdcC64> at phase 0 (the ONE
// routine that decides which bytes are read; its mixer is computed and selected away: a known cost, not tuned here); barrier;
// then a thread takes sample PAIRS counted on the absolute index, as the generator does, so that one noise block serves both,
// and the pair leaves as one 16-byte store where the address allows, else as 8-byte stores.  The sinusoids of a path whose
// diffuse_gain is 0 are summed all the same: 0 * d carries d's sign into a zero.  No atomics, nothing shared between workgroups.
//
// LDS: [tile + H float2, padded][L x chan_nodes float2][L S + L x (phase0, step)]: 50 176 bytes at the most: no attribute.
//
// KERNEL ORDER (amcx_launch.h): one plain kernel in the header amcx.hip includes FIRST; it includes the generator's header (and
// with it the training kernels' and the down-converter's) in front of its own kernel: tools/codeobj_gate.py --kernels,
// profiles/r34_channel_codeobj_kernels.txt.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "amcx_synth_kernel.h"

namespace amcx {

constexpr int kChanThreads = 256;
constexpr int kChanMaxPaths = 16;          // AMCX_CHANNEL_MAX_PATHS
constexpr int kChanMaxSinusoids = 32;      // AMCX_CHANNEL_MAX_SINUSOIDS
constexpr int kChanMaxDelay = 1024;        // AMCX_CHANNEL_MAX_DELAY
constexpr int kChanMaxInterpLog2 = 16;
constexpr int kChanMaxTile = 2048;         // most outputs of one tile: 4 pairs per thread
constexpr int kChanNodeBudget = 2048;      // float2 of node gains over all paths
constexpr unsigned kChanRandomPhase = 1u;  // AMCX_CHANNEL_RANDOM_PHASE
constexpr unsigned kChanStream = 3u;       // the draws' stream number in the generator's counter layout
constexpr unsigned kChanLosCounter = 512u; // counter of path l's line of sight: 512 + l (32 l + s < 512)

static_assert(kChanMaxPaths * kChanMaxSinusoids <= (int)kChanLosCounter, "the sinusoids' counters stay below the lines of sight's");

struct ChanPath {                          // a path record of include/amcx.h, 16 bytes
  int delay;
  float diffuse_gain, los_gain;
  int los_doppler_q31;
};

// outputs per tile: at most kChanMaxTile, within the node budget, even where more than one
inline int chan_tile_outputs(int L, int b) {
  const long long by_nodes = (long long)(kChanNodeBudget / L - 2) << b;
  const int tile = by_nodes < kChanMaxTile ? (int)by_nodes : kChanMaxTile;
  return tile > 1 ? tile & ~1 : tile;
}
// the most nodes of one path a tile needs, wherever it begins: k of its first sample ... k of its last, and one more
__host__ __device__ __forceinline__ int chan_nodes(int tile, int b) { return (int)(((long long)tile - 2 + (1ll << b)) >> b) + 2; }
// dynamic LDS of a launch: the padded image of tile + H samples, the nodes, the draws
inline size_t chan_lds_bytes(int L, int S, int b, int H) {
  const int tile = chan_tile_outputs(L, b);
  return (size_t)ddc_stage_bytes(tile + H) + 8u * (size_t)(L * chan_nodes(tile, b)) + 16u * (size_t)(L * S + L);
}

struct ChanArgs {
  unsigned seed_lo, seed_hi;
  unsigned long long row_index0;
  long long sample_index0, n_rows, row_samples, in_stride, out_stride;
  const float2* in;
  ChanPath paths[kChanMaxPaths];
  int L, S, b, H;
  unsigned doppler_max, flags;
  const float* sigma;                      // nullptr: no noise
  long long frames_per_group;
  float2* out;
  int tile;
  long long tiles_per_row, n_items;
};

__global__ __launch_bounds__(kChanThreads) void amcx_channel_c64_kernel(ChanArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char chan_lds[];
  const long long item = (long long)blockIdx.y * gridDim.x + blockIdx.x;
  if (item >= a.n_items) return;                                       // (the whole workgroup: the grid's last line)
  const int tid = (int)threadIdx.x;
  const int L = a.L, S = a.S, b = a.b, H = a.H;
  const int npp = chan_nodes(a.tile, b);
  float2* const stage = reinterpret_cast<float2*>(chan_lds);
  float2* const nodes = reinterpret_cast<float2*>(chan_lds + ddc_stage_bytes(a.tile + H));
  unsigned long long* const draws = reinterpret_cast<unsigned long long*>(nodes + L * npp);    // (phase0, step) of (l, s), then of the lines of sight

  const long long f = item / a.tiles_per_row, ti = item - f * a.tiles_per_row;
  const unsigned long long r = a.row_index0 + (unsigned long long)f;
  const unsigned r_lo = (unsigned)r, r_hi = (unsigned)(r >> 32);
  const float sigma = a.sigma != nullptr ? a.sigma[f / a.frames_per_group] : 0.0f;
  const long long o0 = ti * a.tile;                                    // the tile's first output, in the call's row
  const int n_out = a.row_samples - o0 < a.tile ? (int)(a.row_samples - o0) : a.tile;
  const long long n0 = a.sample_index0 + o0;                           // ... and absolute
  const long long k0 = n0 >> b;                                        // the tile's first node
  const int n_nodes = (int)(((n0 + n_out - 1) >> b) - k0) + 2;         // <= npp

  // 1. the draws
  for (int i = tid; i < L * S + L; i += kChanThreads) {
    const bool los = i >= L * S;
    const int l = los ? i - L * S : i / S;
    const unsigned j = los ? kChanLosCounter + (unsigned)l : 32u * (unsigned)l + (unsigned)(i - l * S);
    unsigned X[4];
    philox4x32_10(j, kChanStream << 28, r_lo, r_hi, a.seed_lo, a.seed_hi, X);
    const float c = ddc_mixer(X[1]).x;                                 // the cosine of a uniform arrival angle
    const long long ci = (long long)(c * 0x1p31f);                     // exact product, truncated toward zero
    const long long lq = (long long)a.paths[l].los_doppler_q31;
    const bool phased = !los || (a.flags & kChanRandomPhase) != 0u;
    draws[2 * i] = phased ? (unsigned long long)X[0] << 32 : 0ull;
    draws[2 * i + 1] = (unsigned long long)((los ? lq : ci) * (long long)a.doppler_max);
  }
  __syncthreads();
  // 2. the node gains k0 ... k0 + n_nodes - 1 of every path
  for (int i = tid; i < L * n_nodes; i += kChanThreads) {
    const int l = i / n_nodes, j = i - l * n_nodes;
    const unsigned long long kB = (unsigned long long)(k0 + j) << b;
    const unsigned long long* const ds = draws + 2 * (l * S);
    float2 d = ddc_mixer((unsigned)((ds[0] + kB * ds[1]) >> 32));
    for (int s = 1; s < S; ++s) {
      const float2 m = ddc_mixer((unsigned)((ds[2 * s] + kB * ds[2 * s + 1]) >> 32));
      d.x = d.x + m.x;
      d.y = d.y + m.y;
    }
    const unsigned long long* const dl = draws + 2 * (L * S + l);
    const float2 w = ddc_mixer((unsigned)((dl[0] + kB * dl[1]) >> 32));
    const float dg = a.paths[l].diffuse_gain, lg = a.paths[l].los_gain;
    const float pr = dg * d.x;
    const float pi = dg * d.y;
    nodes[l * npp + j] = make_float2(__builtin_fmaf(lg, w.x, pr), __builtin_fmaf(lg, w.y, pi));
  }
  // 3. the tile's input samples: output o of the tile reads stage index o + H - delay
  const char* const base = reinterpret_cast<const char*>(a.in + f * a.in_stride + o0);
  ddc_stage_span<DdcC64, DdcPadded, 1>(stage, base, 0, n_out + H, 1.0f, 0u, 0ull, 0ull, tid);
  __syncthreads();
  // 5. pairs (2 i, 2 i + 1) of absolute samples; a thread's first pair holds the tile's outputs oA, oA + 1, oA = -1 where n0 is odd
  float2* const row_out = a.out + f * a.out_stride + o0;
  const int odd = (int)(n0 & 1);
  const unsigned frac_mask = (1u << b) - 1u;
  const float frac_scale = __uint_as_float((unsigned)(127 - b) << 23);  // 2^-b
  for (int oA = 2 * tid - odd; oA < n_out; oA += 2 * kChanThreads) {
    const unsigned long long nA = (unsigned long long)(n0 + oA), jn = nA >> 1;
    unsigned X[4] = {0u, 0u, 0u, 0u};
    if (sigma != 0.0f)                                                 // (a NaN sigma draws: it propagates through syn_finish)
      philox4x32_10((unsigned)jn, (2u << 28) | (unsigned)(jn >> 32), r_lo, r_hi, a.seed_lo, a.seed_hi, X);
    float2 y[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int o = oA + h;
      y[h] = make_float2(0.0f, 0.0f);
      if (o < 0 || o >= n_out) continue;
      const long long n = n0 + o;
      const int j = (int)((n >> b) - k0);
      const float fr = (float)((unsigned)n & frac_mask) * frac_scale;
      float re = 0.0f, im = 0.0f;
      for (int l = 0; l < L; ++l) {
        const float2 g0 = nodes[l * npp + j], g1 = nodes[l * npp + j + 1];
        const float dre = g1.x - g0.x;
        const float dim = g1.y - g0.y;
        const float cr = __builtin_fmaf(fr, dre, g0.x), cim = __builtin_fmaf(fr, dim, g0.y);
        const float2 x = stage[ddc_pad(o + H - a.paths[l].delay)];
        if (l == 0) {
          const float pa = cim * x.y;
          const float pb = cim * x.x;
          re = __builtin_fmaf(cr, x.x, -pa);
          im = __builtin_fmaf(cr, x.y, pb);
        } else {
          re = __builtin_fmaf(cr, x.x, re);
          re = __builtin_fmaf(-cim, x.y, re);
          im = __builtin_fmaf(cr, x.y, im);
          im = __builtin_fmaf(cim, x.x, im);
        }
      }
      y[h] = syn_finish(make_float2(re, im), 0ull, X[2 * h], X[2 * h + 1], sigma);
    }
    const bool hasA = oA >= 0, hasB = oA + 1 < n_out;
    float2* const dst = row_out + oA;
    if (hasA && hasB && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
      *reinterpret_cast<float4*>(dst) = make_float4(y[0].x, y[0].y, y[1].x, y[1].y);
    } else {
      if (hasA) dst[0] = y[0];
      if (hasB) dst[1] = y[1];
    }
  }
}

}  // namespace amcx
