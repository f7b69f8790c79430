// Blind carrier recovery (include/amcx.h, amcx_carrier_c64; ABI 16.2.3): rows of N complex64 samples to one 32-byte record per
// row -- power, gain, the carrier's frequency and phase as the down-converter's integer words, a quality figure -- and, where
// asked for, the row with gain, frequency and phase taken out, in ONE launch.  The estimator is the M-th-power one: the
// modulation of an M-ary PSK row collapses in x^M, whose spectrum has a line at M times the carrier offset.
// N = 2^lg, M = 2^lm, sb = search_bins, r a row, n a sample, k a SIGNED bin (Z[k] stands for Z[k mod N]):
//
//   power    q[n] = fma(im, im, re re);  THE TREE: q'[i] = q[2 i] + q[2 i + 1] until one value is left;  power = tree * (1 / N)
//   gain     1.0f / sqrtf(power), root and quotient correctly rounded; 0 where power is 0, NaN or inf (a BAD row: the record is
//            zeros beside power, the output row zeros)
//   u, z     u[n] = (gain re, gain im);  z = u, then lm times z = psd_mul(z, z)
//   Z        THE OPERATION SEQUENCE of amcx_psd_kernel.h on z (no window product): psd_pass<3 / 4> CALLED;  P[k] = fma(Z.im, Z.im, Z.re Z.re)
//   bin      the k of -sb ... sb with the largest key (P[k], or -1 where P[k] is NaN), ties to the lowest k
//   frac     a, b, c = Z[bin - 1], Z[bin], Z[bin + 1];  num = c - a;  den = (b - a) + (b - c);
//            frac = -(fma(num.im, den.im, num.re den.re) / fma(den.im, den.im, den.re den.re)), 0 unless |frac| <= 0.5
//   words    F = (int64)rintf(frac 2^31);  step_M = bin 2^(64 - lg) + F 2^(33 - lg);  phase_step = step_M >> lm (arithmetic)
//            w = (int64)rintf((atan2f(b.im, b.re) * (float)(1 / 2 pi)) * 2^32);  theta_M = (uint32)(w - ((F (N - 1)) >> lg));
//            phase0 = theta_M >> lm (logical: one of the M equivalent phases)
//   quality  P[bin] / ((float)N * tree(|z|^2)), |z|^2 formed as q is
//   output   phi(n) = [PHASE] (phase0 << 32) + [FREQ] n phase_step (mod 2^64);  y[n] = psd_mul(v, ddc_mixer(top32(0 - phi(n)))),
//            v = u[n] under GAIN, x[n] otherwise; the product is always formed
// Every integer is exact; atan2f is the device library's (held to a bound, not to ==: tests/carrier_ref.py).  With GIVEN the
// records are read, nothing is estimated, and a record's gain, phase0 and phase_step are applied as they are.
//
// POSITION INDEPENDENCE.  A record and a row depend on the row's samples and the scalar arguments alone.  A SLOT holds one row
// in the points [slot N, (slot + 1) N); a butterfly's twiddle depends on its place in the row alone; the tree is taken in index
// order whichever lanes hold the values (an addition's bits do not depend on the order of its two operands); the peak is the
// greatest element of a total order, whichever way it is reduced; a sample comes in by one 8-byte load wherever the row begins.
//
// THE LAUNCH.  256 threads, A PLAIN GRID: one workgroup per group of G = 4096 / N consecutive rows (slots beyond the call's rows
// carry zeros and store nothing).  Two views of the 4096 points: COALESCED (thread t holds the points t + 256 k: the loads from
// and the stores to global memory) and RUNS (thread t holds the 16 points 16 t ...: N / 16 consecutive threads per row; the
// tree's first four levels are in registers, the next up to six are xor-shuffles, the last two go through four words of LDS).
// Steps: table and staging | barrier | power, gain | barrier | z in place | barrier | sum |z|^2 | barrier | the passes, a
// barrier each | the peak per thread over its run's bins inside the range, shuffles, LDS | the row's first thread forms the record,
// stores it and leaves the three words the output needs in LDS | barrier | the output from the samples READ A SECOND TIME (the
// same 8-byte loads; AMCX_CARRIER_KEEP_ROW 1 keeps them in registers across the transform instead: tools/carrier_bench.py
// measured both, and keeping them was slower in every cell, x0.73 ... 0.85 -- profiles/r36_carrier_bench_keep.json).
// LDS: the spectrogram's padded image (34 KiB) + its table (16 KiB) + 1.5 KiB of per-slot words, static: no attribute.  No
// atomics, no spin, nothing shared between workgroups: capturable in a graph.
//
// LDS BANKS.  The passes are the spectrogram's (its header's account).  The runs read point 16 t + m at float2 index 17 t + m:
// a half-wave's 32 lanes are 17 apart, distinct mod 32, no conflict; the coalesced view touches consecutive points.  The peak
// reads its run's points, the same pattern, a lane skipping those outside the range.  The record's three reads are single.
//
// KERNEL ORDER (amcx_launch.h): one plain kernel in the header amcx.hip includes FIRST; it includes the spectrogram's header
// (and with it the occupancy kernels' and the down-converter's) in front of its own kernel: tools/codeobj_gate.py --kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "amcx_psd_kernel.h"   // psd_pass, psd_pad, psd_mul, the sizes; ddc_mixer through it

#ifndef AMCX_CARRIER_KEEP_ROW
#define AMCX_CARRIER_KEEP_ROW 0
#endif

namespace amcx {

constexpr int kCarThreads = kPsdThreads;
constexpr int kCarMaxSlots = kPsdPoints / kPsdMinFft;                  // 64 rows of 64 samples
constexpr int kCarLdsBytes = kPsdLdsBytes + kCarMaxSlots * (8 + 4 + 4 + 4) + 3 * 16 + 16;
constexpr unsigned kCarGain = 1u, kCarFreq = 2u, kCarPhase = 4u, kCarGiven = 8u;   // AMCX_CARRIER_*

struct CarrierRecord {                     // a record of include/amcx.h, 32 bytes
  long long phase_step;
  unsigned phase0;
  int bin;
  float frac, power, gain, quality;
};

struct CarrierArgs {
  const float2* in;
  long long n_rows, in_stride;
  int n, lg, lm, search;
  unsigned flags;
  CarrierRecord* est;
  float2* out;                             // nullptr: estimate only
  long long out_stride, n_groups;
};

// THE TREE's first four levels over the 16 values of a run
__device__ __forceinline__ float car_tree16(const float* q) {
  float s[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) s[i] = q[2 * i] + q[2 * i + 1];
#pragma unroll
  for (int i = 0; i < 4; ++i) s[i] = s[2 * i] + s[2 * i + 1];
  return (s[0] + s[1]) + (s[2] + s[3]);
}

// ... and the levels above: `sub` consecutive threads hold a row's runs in order; every one of them returns the row's sum.
// red: four words nobody else uses.  (A barrier where sub > 64: sub is the workgroup's.)
__device__ __forceinline__ float car_row_sum(float v, int sub, int lane, int wave, float* red) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float o = __shfl_xor(v, d, 64);
    if (d < sub) v = v + o;
  }
  if (sub > 64) {
    if (lane == 0) red[wave] = v;
    __syncthreads();
    v = sub == 128 ? red[wave & ~1] + red[wave | 1] : (red[0] + red[1]) + (red[2] + red[3]);
  }
  return v;
}

// the order of the peak search: the larger key, then the lower signed bin
__device__ __forceinline__ bool car_better(float key, int k, float than_key, int than_k) {
  return key > than_key || (key == than_key && k < than_k);
}

// Reads in[r in_stride + n], n < N, r < n_rows (and est[r] under GIVEN); writes est[r] (not under GIVEN) and, where out is
// given, out[r out_stride + n]; nothing else.
__global__ __launch_bounds__(kCarThreads) void amcx_carrier_c64_kernel(CarrierArgs a) {
  __shared__ __attribute__((aligned(16))) float2 car_pts[kPsdPadPoints];
  __shared__ __attribute__((aligned(16))) float2 car_tw[kPsdPoints / 2];
  __shared__ long long car_step[kCarMaxSlots];
  __shared__ unsigned car_ph[kCarMaxSlots];
  __shared__ float car_gain[kCarMaxSlots];
  __shared__ int car_bad[kCarMaxSlots];
  __shared__ float car_red[3][4];
  __shared__ int car_red_k[4];
  const long long grp = (long long)blockIdx.y * gridDim.x + blockIdx.x;
  if (grp >= a.n_groups) return;                                       // (the whole workgroup: the grid's last line)
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.n, lg = a.lg, lm = a.lm;
  const int G = kPsdPoints >> lg;                                      // slots: 1 ... 64
  const int sub = kCarThreads / G;                                     // threads of a row's runs: N / 16 = 4 ... 256
  const int slot = tid / sub, t_in = tid - slot * sub;
  const long long r0 = grp * G;

  // the coalesced view: point tid + 256 k is sample n of slot s
  float2 x[kPsdPerThread];
#pragma unroll
  for (int k = 0; k < kPsdPerThread; ++k) {
    const int p = tid + k * kCarThreads;
    const long long r = r0 + (p >> lg);
    x[k] = r < a.n_rows ? a.in[r * a.in_stride + (p & (N - 1))] : make_float2(0.0f, 0.0f);
  }

  if ((a.flags & kCarGiven) == 0u) {
    for (int k = tid; k < kPsdPoints / 2; k += kCarThreads) car_tw[k] = ddc_mixer((0u - (unsigned)k) << 20);
#pragma unroll
    for (int k = 0; k < kPsdPerThread; ++k) car_pts[psd_pad(tid + k * kCarThreads)] = x[k];
    __syncthreads();
    // power and gain, from the runs
    float q[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const float2 v = car_pts[psd_pad(16 * tid + m)];
      q[m] = __builtin_fmaf(v.y, v.y, v.x * v.x);
    }
    const float power = car_row_sum(car_tree16(q), sub, lane, wave, car_red[0]) * __uint_as_float((unsigned)(127 - lg) << 23);
    const bool bad = !(power > 0.0f && power < __builtin_inff());
    const float gain = bad ? 0.0f : 1.0f / sqrtf(power);
    if (t_in == 0) car_gain[slot] = gain;
    __syncthreads();                                                   // (also: the runs are read before z replaces them)
    // z in place, from the samples in registers
#pragma unroll
    for (int k = 0; k < kPsdPerThread; ++k) {
      const int p = tid + k * kCarThreads;
      const float g = car_gain[p >> lg];
      float2 z = make_float2(g * x[k].x, g * x[k].y);
      for (int i = 0; i < lm; ++i) z = psd_mul(z, z);
      car_pts[psd_pad(p)] = z;
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const float2 v = car_pts[psd_pad(16 * tid + m)];
      q[m] = __builtin_fmaf(v.y, v.y, v.x * v.x);
    }
    const float zsum = car_row_sum(car_tree16(q), sub, lane, wave, car_red[1]);
    __syncthreads();                                                   // the passes overwrite what was just read
    int lB = lg;
    for (int left = (lg + 3) >> 2; left > 0; --left) {
      const int K = lB / left;                                         // 3 or 4: the shorter passes first
      if (K == 4) psd_pass<4>(car_pts, car_tw, lB, tid);
      else psd_pass<3>(car_pts, car_tw, lB, tid);
      lB -= K;
      __syncthreads();
    }
    // the peak: Z[b] stands at the bit-reversed b of its row
    const int sb = a.search;
    float best = -2.0f;
    int bin = 0x7fffffff;
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const int b = (int)(__brev((unsigned)(16 * t_in + m)) >> (32 - lg));
      const int k = b >= (N >> 1) ? b - N : b;
      if (k >= -sb && k <= sb) {
        const float2 Z = car_pts[psd_pad(16 * tid + m)];
        const float P = __builtin_fmaf(Z.y, Z.y, Z.x * Z.x);
        const float key = P == P ? P : -1.0f;
        if (car_better(key, k, best, bin)) { best = key; bin = k; }
      }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float ok = __shfl_xor(best, d, 64);
      const int kk = __shfl_xor(bin, d, 64);
      if (d < sub && car_better(ok, kk, best, bin)) { best = ok; bin = kk; }
    }
    if (sub > 64) {
      if (lane == 0) { car_red[2][wave] = best; car_red_k[wave] = bin; }
      __syncthreads();
      const int w0 = sub == 128 ? (wave & ~1) : 0, w1 = sub == 128 ? w0 + 2 : 4;
      for (int w = w0; w < w1; ++w)
        if (car_better(car_red[2][w], car_red_k[w], best, bin)) { best = car_red[2][w]; bin = car_red_k[w]; }
    }
    if (t_in == 0) {
      CarrierRecord rec;
      rec.phase_step = 0;
      rec.phase0 = 0u;
      rec.bin = 0;
      rec.frac = 0.0f;
      rec.power = power;
      rec.gain = gain;
      rec.quality = 0.0f;
      if (!bad) {
        const int base = slot << lg;
        const float2 A = car_pts[psd_pad(base + (int)(__brev((unsigned)((bin - 1) & (N - 1))) >> (32 - lg)))];
        const float2 B = car_pts[psd_pad(base + (int)(__brev((unsigned)(bin & (N - 1))) >> (32 - lg)))];
        const float2 C = car_pts[psd_pad(base + (int)(__brev((unsigned)((bin + 1) & (N - 1))) >> (32 - lg)))];
        const float2 num = psd_sub(C, A), den = psd_add(psd_sub(B, A), psd_sub(B, C));
        float frac = -(__builtin_fmaf(num.y, den.y, num.x * den.x) / __builtin_fmaf(den.y, den.y, den.x * den.x));
        if (!(__builtin_fabsf(frac) <= 0.5f)) frac = 0.0f;
        const long long F = (long long)rintf(frac * 0x1p31f);
        const long long step_m =
            (long long)(((unsigned long long)(long long)bin << (64 - lg)) + ((unsigned long long)F << (33 - lg)));
        const float turn = atan2f(B.y, B.x) * 0.15915494309189535f;
        const float wf = rintf(turn * 0x1p32f);
        const long long w = wf == wf ? (long long)wf : 0ll;
        const unsigned theta_m = (unsigned)(unsigned long long)(w - ((F * (long long)(N - 1)) >> lg));
        rec.phase_step = step_m >> lm;
        rec.phase0 = theta_m >> lm;
        rec.bin = bin;
        rec.frac = frac;
        rec.quality = best / ((float)N * zsum);
      }
      if (r0 + slot < a.n_rows) a.est[r0 + slot] = rec;
      car_step[slot] = rec.phase_step;
      car_ph[slot] = rec.phase0;
      car_bad[slot] = bad ? 1 : 0;
    }
  } else if (tid < G) {
    const bool live = r0 + tid < a.n_rows;
    car_step[tid] = live ? a.est[r0 + tid].phase_step : 0ll;
    car_ph[tid] = live ? a.est[r0 + tid].phase0 : 0u;
    car_gain[tid] = live ? a.est[r0 + tid].gain : 0.0f;
    car_bad[tid] = 0;
  }
  if (a.out == nullptr) return;                                        // (the whole workgroup)
  __syncthreads();
  const bool with_gain = (a.flags & kCarGain) != 0u, with_freq = (a.flags & kCarFreq) != 0u, with_phase = (a.flags & kCarPhase) != 0u;
#pragma unroll
  for (int k = 0; k < kPsdPerThread; ++k) {
    const int p = tid + k * kCarThreads;
    const int s = p >> lg, n = p & (N - 1);
    const long long r = r0 + s;
    if (r >= a.n_rows) continue;
#if !AMCX_CARRIER_KEEP_ROW
    x[k] = a.in[r * a.in_stride + n];
#endif
    const unsigned long long phi = (with_phase ? (unsigned long long)car_ph[s] << 32 : 0ull) +
                                   (with_freq ? (unsigned long long)n * (unsigned long long)car_step[s] : 0ull);
    const float2 w = ddc_mixer((unsigned)((0ull - phi) >> 32));
    const float g = car_gain[s];
    const float2 v = with_gain ? make_float2(g * x[k].x, g * x[k].y) : x[k];
    const float2 y = psd_mul(v, w);
    a.out[r * a.out_stride + n] = car_bad[s] ? make_float2(0.0f, 0.0f) : y;
  }
}

}  // namespace amcx
