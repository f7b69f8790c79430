// Fixed-point deployment of the classifier's network (include/amcx.h, ABI 16): the range calibration behind a Q-format export
// and the 16-bit integer network itself, each ONE launch over the device-resident (rows x n_cols) float32 feature matrix.
//
// Both kernels keep amcx_mlp_classify_kernel's layout (amcx_mlp_kernel.h): a workgroup of 256 threads walks tiles of
// kMlpTileRows rows, slot s of lane t being row  tile * kMlpTileRows + s * 256 + t;  the parameters sit in LDS, every layer
// zero-padded to 32 x 32 weights plus 32 biases; activations live in registers with compile-time indices, widths are run-time
// values handled in blocks of 8 behind wave-uniform branches.  A row's result depends on nothing but the row.
//
// What they share with it stands once in amcx_mlp_shape.h: mlp_stage_params, mlp_load_rows, mlp_dense_f32, mlp_vote.
//
// amcx_mlp_range_kernel.  The float classifier's prologue (column pick, the scaler's two float32 roundings) and its sums
// (float32 FMAs in the order bias, k = 0, 1, ...), by the classifier's own routines, with relu or nothing between the layers.
// Per row the minimum and maximum of the standardised input and of every layer's pre-activation values are parked in a
// lane-private LDS column; a row all of whose
// values are finite then merges them into the lane's running bounds, any other row is counted as skipped and merges nothing.
// At the end a wave folds its 64 lanes with lane shuffles and lane 0 issues one integer atomic per bound: min and max are
// order-free, so the result is exact whatever the reduction.
//
// amcx_mlp_q15_kernel.  The integer network of include/amcx.h, exact for every int16 block.  int16 weights in LDS (2 KB a
// layer), 8 of one output per ds_read_b128; an activation e (any int16) is split into its signed high byte e >> 8 and its
// unsigned low byte e & 255, packed in pairs, so that one v_dot2_i32_i16 takes two weights times two high (or low) bytes:
// over 32 terms |sum_hi| <= 32 * 2^15 * 2^7 = 2^27 and |sum_lo| < 32 * 2^15 * 2^8 = 2^28 fit an int32 accumulator with room,
// and  acc = (sum_hi << 8) + sum_lo + (b << (P - Nb))  is put together in 64 bits.
#pragma once

#include "amcx_mlp_shape.h"

namespace amcx {

constexpr int kActNone = 3;                                   // AMCX_ACT_NONE: the range kernel's second choice
constexpr int kQ15LayerShorts = kMlpLayerFloats;              // padded W[32][32] then b[32], as the float block's layers
constexpr int kRangeSlots = kMlpMaxLinear + 1;                // the input, then every layer

struct Q15Formats {
  float in_scale;                    // 2^Na of the input
  int shift_b[kMlpMaxLinear];        // P - Nb: what the bias is shifted left by
  int shift_o[kMlpMaxLinear];        // P - No >= 1: what the sum is shifted right by, a half rounding up
};

// ---- calibration -----------------------------------------------------------------------------------------------------------
// min, max and finiteness of the first n of a row's values -> the lane's LDS column of slot `slot`
__device__ inline void range_park(const float (&v)[kMlpRowsPerLane][kMlpMaxWidth], int n, float* cand, int slot, bool (&fin)[kMlpRowsPerLane]) {
#pragma unroll
  for (int s = 0; s < kMlpRowsPerLane; ++s) {
    float lo = __builtin_inff(), hi = -__builtin_inff();
    bool ok = true;
#pragma unroll
    for (int j = 0; j < kMlpMaxWidth; ++j) {
      if (j < n) {
        const float t = v[s][j];
        lo = t < lo ? t : lo;
        hi = t > hi ? t : hi;
        ok = ok && mlp_finite(t);
      }
    }
    fin[s] = fin[s] && ok;
    cand[((slot * kMlpRowsPerLane + s) * 2 + 0) * kMlpThreads + threadIdx.x] = lo;
    cand[((slot * kMlpRowsPerLane + s) * 2 + 1) * kMlpThreads + threadIdx.x] = hi;
  }
}

// float min / max into global memory with the integer atomics: a float32 that is no NaN orders as its bits do, signed where it
// is >= 0 and unsigned (reversed) where it is < 0; v + 0 turns -0 into +0, which sits on the non-negative side
__device__ inline void atomic_min_f32(float* addr, float v) {
  v += 0.0f;
  if (v >= 0.0f) atomicMin(reinterpret_cast<int*>(addr), __float_as_int(v));
  else atomicMax(reinterpret_cast<unsigned*>(addr), __float_as_uint(v));
}
__device__ inline void atomic_max_f32(float* addr, float v) {
  v += 0.0f;
  if (v >= 0.0f) atomicMax(reinterpret_cast<int*>(addr), __float_as_int(v));
  else atomicMin(reinterpret_cast<unsigned*>(addr), __float_as_uint(v));
}

// ranges <- (+inf, -inf) per slot, skipped <- 0, ahead of the range kernel on the same stream (a kernel, as the classifier's
// count zeroing: a kernel node replays in a captured graph as launched)
__global__ __launch_bounds__(64) void amcx_mlp_range_init_kernel(float* __restrict__ ranges, int n_slots,
                                                                 unsigned long long* __restrict__ skipped) {
  const int i = threadIdx.x;
  if (i < n_slots) {
    ranges[2 * i] = __builtin_inff();
    ranges[2 * i + 1] = -__builtin_inff();
  }
  if (i == 0) *skipped = 0ull;
}

__global__ __launch_bounds__(kMlpThreads) void amcx_mlp_range_kernel(
    const float* __restrict__ x, long long n_rows, long long row_stride, SelectCols sel, const double* __restrict__ mean,
    const double* __restrict__ scale, const float* __restrict__ params, MlpShape shape, float* __restrict__ ranges,
    unsigned long long* __restrict__ skipped, long long n_tiles) {
  constexpr int R = kMlpRowsPerLane, P = kMlpMaxWidth;
  __shared__ float4 lds4[kMlpMaxLinear * kMlpLayerFloats / 4];
  __shared__ float cand[kRangeSlots * R * 2 * kMlpThreads];      // a row's bounds per slot, a column per lane
  float* lds = reinterpret_cast<float*>(lds4);
  const int n_linear = shape.n_linear;

  mlp_stage_params(lds, params, shape);
  float run_lo[kRangeSlots], run_hi[kRangeSlots];                 // the lane's running bounds per slot
#pragma unroll
  for (int l = 0; l < kRangeSlots; ++l) {
    run_lo[l] = __builtin_inff();
    run_hi[l] = -__builtin_inff();
  }
  unsigned long long n_skipped = 0ull;                             // lane 0 of a wave counts for the wave

  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    float h[R][P];
    long long row[R];
    bool fin[R];
    mlp_load_rows(x, n_rows, row_stride, sel, mean, scale, tile, h, row);
#pragma unroll
    for (int s = 0; s < R; ++s) fin[s] = true;
    range_park(h, shape.w[0], cand, 0, fin);
    for (int l = 0; l < n_linear; ++l) {
      const int n_in = shape.w[l], n_out = shape.w[l + 1];
      float nx[R][P];
      mlp_dense_f32(lds + l * kMlpLayerFloats, n_in, n_out, h, nx);
      range_park(nx, n_out, cand, l + 1, fin);
      if (l + 1 < n_linear && shape.act == kActRelu) mlp_act_all<kActRelu>(nx, n_out);
#pragma unroll
      for (int s = 0; s < R; ++s) {
#pragma unroll
        for (int j = 0; j < P; ++j) h[s][j] = nx[s][j];
      }
    }
#pragma unroll
    for (int s = 0; s < R; ++s) {
      const bool live = row[s] < n_rows;
      if (live && fin[s]) {
#pragma unroll
        for (int l = 0; l < kRangeSlots; ++l) {
          if (l <= n_linear) {
            const float lo = cand[((l * R + s) * 2 + 0) * kMlpThreads + threadIdx.x];
            const float hi = cand[((l * R + s) * 2 + 1) * kMlpThreads + threadIdx.x];
            run_lo[l] = lo < run_lo[l] ? lo : run_lo[l];
            run_hi[l] = hi > run_hi[l] ? hi : run_hi[l];
          }
        }
      }
      n_skipped += (unsigned long long)__popcll(__ballot(live && !fin[s]));
    }
  }

#pragma unroll
  for (int l = 0; l < kRangeSlots; ++l) {
    if (l <= n_linear) {
      float lo = run_lo[l], hi = run_hi[l];
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const float ol = __shfl_xor(lo, d), oh = __shfl_xor(hi, d);
        lo = ol < lo ? ol : lo;
        hi = oh > hi ? oh : hi;
      }
      if ((threadIdx.x & 63u) == 0u && lo <= hi) {                // (a wave none of whose rows counted holds +inf, -inf)
        atomic_min_f32(ranges + 2 * l, lo);
        atomic_max_f32(ranges + 2 * l + 1, hi);
      }
    }
  }
  if ((threadIdx.x & 63u) == 0u && n_skipped != 0ull) atomicAdd(skipped, n_skipped);
}

// ---- the integer network -----------------------------------------------------------------------------------------------------
typedef short q15_short2 __attribute__((ext_vector_type(2)));

// two int16 weights times two int16 values, added to acc: v_dot2_i32_i16, no clamp
__device__ inline int q15_dot2(int w_pair, int v_pair, int acc) {
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(q15_short2, w_pair), __builtin_bit_cast(q15_short2, v_pair), acc, false);
}

// the sum of one wave's values in every lane
__device__ inline unsigned q15_wave_sum(unsigned v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v += (unsigned)__shfl_xor((int)v, d);
  return v;
}

// e[0 .. 31] (each an int16 value in an int) -> 16 pairs of signed high bytes and 16 pairs of unsigned low bytes
__device__ inline void q15_split(const int (&e)[kMlpMaxWidth], int (&hi)[kMlpMaxWidth / 2], int (&lo)[kMlpMaxWidth / 2]) {
#pragma unroll
  for (int p = 0; p < kMlpMaxWidth / 2; ++p) {
    const int a = e[2 * p], b = e[2 * p + 1];
    hi[p] = (int)(((unsigned)(a >> 8) & 0xffffu) | ((unsigned)(b >> 8) << 16));
    lo[p] = (a & 0xff) | ((b & 0xff) << 16);
  }
}

__global__ __launch_bounds__(kMlpThreads) void amcx_mlp_q15_kernel(
    const float* __restrict__ x, long long n_rows, long long row_stride, SelectCols sel, const double* __restrict__ mean,
    const double* __restrict__ scale, const short* __restrict__ params, MlpShape shape, Q15Formats fmt, int* __restrict__ labels,
    short* __restrict__ logits, long long logits_stride, long long rows_per_group, unsigned long long* __restrict__ counts,
    unsigned long long* __restrict__ saturated, long long n_tiles) {
  constexpr int R = kMlpRowsPerLane, P = kMlpMaxWidth;
  __shared__ int4 lds4[kMlpMaxLinear * kQ15LayerShorts / 8];
  short* lds = reinterpret_cast<short*>(lds4);
  const int n_linear = shape.n_linear, n_cls = shape.w[n_linear];
  const bool lane0 = (threadIdx.x & 63u) == 0u;

  mlp_stage_params(lds, params, shape);

  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    int e[R][P];
    int ahi[R][P / 2], alo[R][P / 2];
    long long row[R];
    bool labelled[R];                  // a live row with a finite standardised input: what `saturated` counts over
    bool finite[R];
    {
      float h[R][P];
      mlp_load_rows(x, n_rows, row_stride, sel, mean, scale, tile, h, row);
      unsigned clamped = 0u;
#pragma unroll
      for (int s = 0; s < R; ++s) {
        bool ok = true;
#pragma unroll
        for (int j = 0; j < P; ++j)
          if (j < sel.n) ok = ok && mlp_finite(h[s][j]);
        finite[s] = ok;
        labelled[s] = ok && row[s] < n_rows;
#pragma unroll
        for (int j = 0; j < P; ++j) {
          int q = 0;
          if (j < sel.n) {
            const float t = h[s][j] * fmt.in_scale;                 // a power of two: exact, or +-inf, which clamps
            const bool below = t < -16384.0f, above = t > 16383.0f;
            const float c = below ? -16384.0f : above ? 16383.0f : t;
            q = ok ? (int)__builtin_rintf(c) : 0;                   // round half to even
            clamped += labelled[s] && (below || above) ? 1u : 0u;
          }
          e[s][j] = q;
        }
        q15_split(e[s], ahi[s], alo[s]);
      }
      if (saturated != nullptr) {
        const unsigned n = q15_wave_sum(clamped);
        if (lane0 && n != 0u) atomicAdd(saturated, (unsigned long long)n);
      }
    }

    for (int l = 0; l < n_linear; ++l) {
      const int n_in = shape.w[l], n_out = shape.w[l + 1];
      const short* wl = lds + l * kQ15LayerShorts;
      const bool hidden = l + 1 < n_linear;
      const int sb = fmt.shift_b[l], so = fmt.shift_o[l];
      const long long half = 1ll << (so - 1);
      unsigned clipped = 0u;
#pragma unroll
      for (int oc = 0; oc < P; oc += 8) {
        if (oc < n_out) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            int sum_hi[R], sum_lo[R];
#pragma unroll
            for (int s = 0; s < R; ++s) sum_hi[s] = sum_lo[s] = 0;
#pragma unroll
            for (int kc = 0; kc < P; kc += 8) {
              if (kc < n_in) {
                const int4 w4 = *reinterpret_cast<const int4*>(wl + (oc + j) * P + kc);
                const int w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
#pragma unroll
                  for (int s = 0; s < R; ++s) {
                    sum_hi[s] = q15_dot2(w[q], ahi[s][kc / 2 + q], sum_hi[s]);
                    sum_lo[s] = q15_dot2(w[q], alo[s][kc / 2 + q], sum_lo[s]);
                  }
                }
              }
            }
            const long long bias = (long long)wl[P * P + oc + j] * (1ll << sb);
#pragma unroll
            for (int s = 0; s < R; ++s) {
              const long long acc = (long long)sum_hi[s] * 256 + (long long)sum_lo[s] + bias;
              const long long v = (acc + half) >> so;               // arithmetic: a half rounds up
              const bool over = v > 32767, under = v < -32768;
              clipped += labelled[s] && (over || (under && !hidden)) ? 1u : 0u;
              int o = over ? 32767 : under ? -32768 : (int)v;
              if (hidden && o < 0) o = 0;
              e[s][oc + j] = o;
            }
          }
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
#pragma unroll
            for (int s = 0; s < R; ++s) e[s][oc + j] = 0;
          }
        }
      }
      if (saturated != nullptr) {
        const unsigned n = q15_wave_sum(clipped);
        if (lane0 && n != 0u) atomicAdd(saturated + l + 1, (unsigned long long)n);
      }
      if (hidden) {
#pragma unroll
        for (int s = 0; s < R; ++s) q15_split(e[s], ahi[s], alo[s]);
      }
    }

#pragma unroll
    for (int s = 0; s < R; ++s) {
      int best = 0, vbest = e[s][0];
#pragma unroll
      for (int j = 1; j < P; ++j) {
        if (j < n_cls && e[s][j] > vbest) {                         // strictly greater: the first maximum wins
          best = j;
          vbest = e[s][j];
        }
      }
      const bool live = row[s] < n_rows;
      if (live) {
        if (labels != nullptr) labels[row[s]] = finite[s] ? best : -1;
        if (logits != nullptr) {
          short* pr = logits + row[s] * logits_stride;
#pragma unroll
          for (int j = 0; j < P; ++j)
            if (j < n_cls) pr[j] = finite[s] ? (short)e[s][j] : (short)0;      // a row without a label: zeros
        }
      }
      if (counts != nullptr) mlp_vote(tile, s, row[s], live, finite[s], best, n_cls, rows_per_group, counts, n_rows);
    }
  }
}

}  // namespace amcx
