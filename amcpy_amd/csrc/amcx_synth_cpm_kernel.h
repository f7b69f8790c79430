// The continuous-phase generator (include/amcx.h, amcx_synth_cpm_c64; ABI 16.2.2): rows of exp(j Phi[n]) -- FSK, MSK, GMSK --
// whose phase is a running sum over EVERY symbol so far, kept in uint32 arithmetic mod 2^32 in units of 2^-32 turn, which is what
// the mixer reads: integer sums are associative, so the sum is exact in whatever order it is taken.  A sibling of the linear
// generator (amcx_synth_kernel.h): its key and counters, its row draw, its timing, its symbol draw on stream 1, its noise
// finish syn_finish CALLED, the plan arithmetic and the tap image of amcx_polyphase.h CALLED.  r the absolute row, n the sample:
//
//   alpha_j  = 2 idx_j - (order - 1),   idx_j = mulhi32(Philox(counter(1, j >> 2, r))[j & 3], order)
//   A(K)     = sum_{j < K} alpha_j
//   cnt_n    = taps of phase p_n = P - (p_n >= T - (P - 1) U)
//   Phi[n]   = phase_full A(k_n - cnt_n + 1) + sum_{q < cnt_n} alpha[k_n - q] phase_taps[p_n + q U]
//   out      = syn_finish((1, 0), phase0_r + n step_r + ((uint64)Phi[n] << 32), w1, w2, sigma)
//
// THE CARRIED SUM.  acc_in[f] = A(K0), K0 = floor(sample_index0 V / U), which the drawn timing does not enter; a null acc_in is
// A(0) = 0.  acc_out[f] = A(floor((sample_index0 + row_samples) V / U)), written by the row's last segment alone.
//
// THE LAUNCH.  256 threads, A PLAIN GRID: one workgroup per (row, segment), a segment being `tiles_per_seg` consecutive tiles of
// the linear generator's plan (syn_tile_outputs), walked in order with A carried in a register.  Once per workgroup: the taps
// phase-major at the polyphase pitch (poly_stage_taps moves their bits), the row draw, and A at the segment's first window,
// acc_in plus a SWEEP over the symbols from K0 on (cpm_sweep: thread t the Philox blocks t, t + 256, ..., one integer
// reduction).  Per tile: the span's symbols drawn into LDS as integers, an inclusive scan of the span (a thread sums a run of
// ODD length, so the lanes of a wave fall on different banks; wave scan by shuffles; four wave totals through LDS), then
// sample pairs counted on the absolute index exactly as the linear kernel takes them.  Where V / U passes the window, the
// symbols between one tile's span and the next are swept as well.  Nothing but 32-bit multiply-adds in the window sum.
//
// LDS: [span int][span + 1 uint, the scan behind a zero][U phases of `pitch` words][8 words]: 59 428 bytes at the most: no attribute.
//
// KERNEL ORDER (amcx_launch.h): one plain kernel in the header amcx.hip includes FIRST; it includes the generator's header (and
// with it the training kernels' and the down-converter's) in front of its own kernel: profiles/r35_cpm_codeobj_kernels.txt.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "amcx_synth_kernel.h"

namespace amcx {

constexpr int kCpmThreads = 256;
constexpr int kCpmMaxSegments = 64;

// dynamic LDS of a launch: the worst span's symbols and their scan, the phase-major taps, the reduction's words
inline size_t cpm_lds_bytes(int T, int U, int V) { return 8u * (size_t)syn_max_span(T, U, V) + 4u + poly_taps_bytes(T, U) + 32u; }

struct CpmArgs {
  unsigned seed_lo, seed_hi;
  unsigned long long row_index0;
  long long sample_index0, n_rows, row_samples, row_stride;
  int order;
  const unsigned* taps;
  unsigned phase_full;
  int T, U, V, P, tau0, max_span;
  unsigned long long phase_step;
  unsigned cfo_max, flags;
  const float* sigma;
  long long frames_per_group;
  const unsigned* acc_in;                  // nullptr: A(0) = 0 (sample_index0 == 0)
  unsigned* acc_out;                       // nullptr: not wanted
  float2* out;
  int tile, segments;
  long long tiles_per_row, tiles_per_seg, n_items;
};

// the workgroup's sum of `x` over its 256 threads, the same in every thread; `red`: 4 words of LDS, free again on return
__device__ __forceinline__ unsigned cpm_wg_sum(unsigned x, unsigned* red, int tid) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x += (unsigned)__shfl_xor((int)x, d, 64);
  if ((tid & 63) == 0) red[tid >> 6] = x;
  __syncthreads();
  const unsigned s = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return s;
}

// sum of alpha_j over lo <= j < hi (0 where hi <= lo) of row r: thread t the Philox blocks t, t + 256, ...
__device__ __forceinline__ unsigned cpm_sweep(long long lo, long long hi, unsigned r_lo, unsigned r_hi, const CpmArgs& a,
                                              unsigned* red, int tid) {
  unsigned sum = 0u;
  if (hi > lo) {
    const long long b0 = lo >> 2, b1 = (hi - 1) >> 2;
    for (long long b = b0 + tid; b <= b1; b += kCpmThreads) {
      unsigned X[4];
      philox4x32_10((unsigned)b, (1u << 28) | (unsigned)((unsigned long long)b >> 32), r_lo, r_hi, a.seed_lo, a.seed_hi, X);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const long long j = (b << 2) + c;
        const unsigned alpha = 2u * __umulhi(X[c], (unsigned)a.order) - (unsigned)(a.order - 1);
        sum += (j >= lo && j < hi) ? alpha : 0u;
      }
    }
  }
  return cpm_wg_sum(sum, red, tid);
}

// Phi of the sample whose window begins at span index off with phase p; `base` = A at the span's first symbol
__device__ __forceinline__ unsigned cpm_phase(const int* val, const unsigned* scn, const unsigned* g, int pitch, int P, int full,
                                              unsigned phase_full, unsigned base, int off, int p) {
  const int cnt = P - (p >= full ? 1 : 0);
  const int top = off + P - 1;
  unsigned phi = phase_full * (base + scn[top - cnt + 1]);
  const unsigned* const gp = g + p * pitch;
#pragma unroll 4
  for (int q = 0; q < cnt; ++q) phi += (unsigned)val[top - q] * gp[q];
  return phi;
}

__global__ __launch_bounds__(kCpmThreads) void amcx_synth_cpm_c64_kernel(CpmArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cpm_lds[];
  const long long item = (long long)blockIdx.y * gridDim.x + blockIdx.x;
  if (item >= a.n_items) return;                                       // (the whole workgroup: the grid's last line)
  int* const val = reinterpret_cast<int*>(cpm_lds);
  unsigned* const scn = reinterpret_cast<unsigned*>(cpm_lds) + a.max_span;
  unsigned* const g = scn + a.max_span + 1;
  const int tid = (int)threadIdx.x;
  const int T = a.T, U = a.U, V = a.V, P = a.P;
  const int pitch = poly_pitch(P);
  unsigned* const red = g + U * pitch;
  // the integer taps are moved, never computed on: the float routine copies their bits
  poly_stage_taps(reinterpret_cast<float*>(g), reinterpret_cast<const float*>(a.taps), T, U, pitch, tid, kCpmThreads);
  const int full = T - (P - 1) * U;                                    // phases p < full have P taps, the others P - 1
  const unsigned stride = 2u * (unsigned)kCpmThreads * (unsigned)V;    // a thread's step of t: 256 pairs on
  const int step_q = (int)(stride / (unsigned)U), step_r = (int)(stride - (unsigned)step_q * (unsigned)U);
  const int back_q = (int)((unsigned)V / (unsigned)U), back_r = V - back_q * U;      // one sample back

  const long long f = item / a.segments, seg = item - f * a.segments;
  const unsigned long long r = a.row_index0 + (unsigned long long)f;
  const unsigned r_lo = (unsigned)r, r_hi = (unsigned)(r >> 32);
  unsigned W[4];
  philox4x32_10(0u, 0u, r_lo, r_hi, a.seed_lo, a.seed_hi, W);
  const unsigned long long phase0 = (a.flags & kSynRandomPhase) ? (unsigned long long)W[0] << 32 : 0ull;
  const unsigned long long step = a.phase_step + (unsigned long long)((long long)(int)W[1] * (long long)a.cfo_max);
  const int tau = (a.flags & kSynRandomTiming) ? (int)__umulhi(W[2], (unsigned)U) : a.tau0;
  const float sigma = a.sigma[f / a.frames_per_group];

  const long long ti0 = seg * a.tiles_per_seg;
  const long long ti1 = ti0 + a.tiles_per_seg < a.tiles_per_row ? ti0 + a.tiles_per_seg : a.tiles_per_row;
  // A at symbol `at`: the call's state at K0, then swept forward to each tile's first symbol
  long long at = a.sample_index0 * V / U;
  unsigned A = a.acc_in != nullptr ? a.acc_in[f] : 0u;
  for (long long ti = ti0; ti < ti1; ++ti) {
    const long long o0 = ti * a.tile;                                  // the tile's first sample, in the call's row
    const int n_out = a.row_samples - o0 < a.tile ? (int)(a.row_samples - o0) : a.tile;
    const long long n0 = a.sample_index0 + o0;                         // ... and absolute
    const long long t0 = n0 * V + tau;
    const long long s0 = t0 / U;                                       // the span's first symbol
    const int r0 = (int)(t0 - s0 * U);
    const int span = (int)(((unsigned)(n_out - 1) * (unsigned)V + (unsigned)r0) / (unsigned)U) + P;
    if (at != s0) {                                                    // the segment's first tile, or a gap between two spans (at < s0)
      A += cpm_sweep(at, s0, r_lo, r_hi, a, red, tid);
      at = s0;
    }
    {
      const long long b0 = s0 >> 2;
      const int n_blocks = (int)(((s0 + span - 1) >> 2) - b0) + 1;
      for (int b = tid; b < n_blocks; b += kCpmThreads) {
        const unsigned long long j = (unsigned long long)(b0 + b);
        unsigned X[4];
        philox4x32_10((unsigned)j, (1u << 28) | (unsigned)(j >> 32), r_lo, r_hi, a.seed_lo, a.seed_hi, X);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const long long i = (long long)(j << 2) + c - s0;             // the symbol's place in the span
          if (i >= 0 && i < span) val[i] = (int)(2u * __umulhi(X[c], (unsigned)a.order) - (unsigned)(a.order - 1));
        }
      }
    }
    __syncthreads();
    // the inclusive scan behind a zero: scn[i] = sum of val[0 .. i)
    {
      const int run = ((span + kCpmThreads - 1) / kCpmThreads) | 1;
      const int i0 = tid * run, i1 = i0 + run < span ? i0 + run : span;
      unsigned mine = 0u;
      for (int i = i0; i < i1; ++i) mine += (unsigned)val[i];
      unsigned incl = mine;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned up = (unsigned)__shfl_up((int)incl, d, 64);
        if ((tid & 63) >= d) incl += up;
      }
      if ((tid & 63) == 63) red[4 + (tid >> 6)] = incl;
      __syncthreads();
      unsigned run_sum = incl - mine;
      for (int w = 0; w < (tid >> 6); ++w) run_sum += red[4 + w];
      if (tid == 0) scn[0] = 0u;
      for (int i = i0; i < i1; ++i) {
        run_sum += (unsigned)val[i];
        scn[i + 1] = run_sum;
      }
    }
    __syncthreads();
    // pairs (2 i, 2 i + 1) of absolute samples; this thread's first pair holds the tile's samples oA, oA + 1, oA = -1 where n0 is odd
    float2* const row_out = a.out + f * a.row_stride + o0;
    const int odd = (int)(n0 & 1);
    const unsigned uB = (unsigned)(2 * tid + 1 - odd) * (unsigned)V + (unsigned)r0;   // the one division of this thread and tile
    int offB = (int)(uB / (unsigned)U), pB = (int)(uB - (unsigned)offB * (unsigned)U);
    for (int oA = 2 * tid - odd; oA < n_out; oA += 2 * kCpmThreads) {
      const bool hasA = oA >= 0, hasB = oA + 1 < n_out;
      const unsigned long long nA = (unsigned long long)(n0 + oA), jn = nA >> 1;
      unsigned X[4] = {0u, 0u, 0u, 0u};
      if (sigma != 0.0f)                                               // (a NaN sigma draws: it propagates through syn_finish)
        philox4x32_10((unsigned)jn, (2u << 28) | (unsigned)(jn >> 32), r_lo, r_hi, a.seed_lo, a.seed_hi, X);
      float2 yA = make_float2(0.0f, 0.0f), yB = yA;
      if (hasA) {
        int offA = offB - back_q, pA = pB - back_r;
        if (pA < 0) { pA += U; --offA; }
        const unsigned phi = cpm_phase(val, scn, g, pitch, P, full, a.phase_full, A, offA, pA);
        yA = syn_finish(make_float2(1.0f, 0.0f), phase0 + nA * step + ((unsigned long long)phi << 32), X[0], X[1], sigma);
      }
      if (hasB) {
        const unsigned phi = cpm_phase(val, scn, g, pitch, P, full, a.phase_full, A, offB, pB);
        yB = syn_finish(make_float2(1.0f, 0.0f), phase0 + (nA + 1ull) * step + ((unsigned long long)phi << 32), X[2], X[3], sigma);
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
    // A moves to where the next tile's span begins -- or, behind the row's last tile, to the symbol acc_out names -- as far as
    // this span's scan reaches; what lies beyond it is swept (above, or below)
    const bool last = ti + 1 == a.tiles_per_row;
    const long long next = last ? (a.sample_index0 + a.row_samples) * V / U : ((n0 + n_out) * V + tau) / U;
    const long long reach = next < s0 ? s0 : next - s0 < span ? next : s0 + span;      // (next >= s0 - 1, and only behind the last tile below s0)
    A += scn[(int)(reach - s0)];
    at = reach;
    __syncthreads();                                                   // the next tile's symbols overwrite what was just read
    if (last && a.acc_out != nullptr) {
      // A(next) from A(at): forward by a sweep, or one symbol back (a drawn timing can put the last span's first symbol behind it)
      const unsigned fwd = cpm_sweep(at, next, r_lo, r_hi, a, red, tid), back = cpm_sweep(next, at, r_lo, r_hi, a, red, tid);
      if (tid == 0) a.acc_out[f] = A + fwd - back;
    }
  }
}

}  // namespace amcx
