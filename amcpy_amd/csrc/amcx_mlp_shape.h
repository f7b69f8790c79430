// What the kernels over the feature matrix share and no kernel of: the column selection of the post-processing entries, the
// scaler's two roundings, the limits and the shape of the dense network, its activations, and the routines the three
// inference kernels are made of -- parameter staging, row load, the float32 sums, the votes (amcx_post_kernels.h,
// amcx_mlp_kernel.h, amcx_mlp_q15_kernel.h, amcx_mlp_train_kernel.h).  No kernel stands here, so including it ahead of others
// moves nothing in .text (KERNEL ORDER, amcx_launch.h).
#pragma once

#include <hip/hip_runtime.h>

namespace amcx {

constexpr int kStatMaxCols = 32;

struct SelectCols {
  int n;
  int c[kStatMaxCols];
};

constexpr int kMlpMaxWidth = 32;      // every layer width, input and output included (kStatMaxCols)
constexpr int kMlpMaxLinear = 6;
constexpr int kMlpThreads = 256;
constexpr int kMlpRowsPerLane = 2;
constexpr int kMlpTileRows = kMlpThreads * kMlpRowsPerLane;
constexpr int kMlpLayerFloats = kMlpMaxWidth * kMlpMaxWidth + kMlpMaxWidth;   // padded W[32][32] then b[32]
constexpr int kActRelu = 0, kActTanh = 1, kActSigmoid = 2;

struct MlpShape {
  int n_linear;
  int act;
  int w[kMlpMaxLinear + 1];    // w[0] inputs ... w[n_linear] classes
};

template <int ACT>
__device__ inline float mlp_act(float v) {
  if (ACT == kActRelu) return v < 0.0f ? 0.0f : v;                 // NaN stays NaN, as torch.relu keeps it
  if (ACT == kActTanh) return tanhf(v);
  return 1.0f / (1.0f + expf(-v));
}

// the activation over the blocks of 8 outputs a layer has (the padding beyond stays 0)
template <int ACT>
__device__ inline void mlp_act_all(float (&v)[kMlpRowsPerLane][kMlpMaxWidth], int n_out) {
#pragma unroll
  for (int oc = 0; oc < kMlpMaxWidth; oc += 8) {
    if (oc < n_out) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int s = 0; s < kMlpRowsPerLane; ++s) v[s][oc + j] = mlp_act<ACT>(v[s][oc + j]);
      }
    }
  }
}

// ---- what the classifier, the range calibration and the integer network share ---------------------------------------------
// the packed block (per layer W[out][in] row-major, then b[out]) -> the padded copy in LDS; returns behind a barrier
template <class T>
__device__ inline void mlp_stage_params(T* lds, const T* __restrict__ params, const MlpShape& shape) {
  constexpr int P = kMlpMaxWidth;
  for (int i = threadIdx.x; i < shape.n_linear * kMlpLayerFloats; i += kMlpThreads) lds[i] = T(0);
  __syncthreads();
  const T* src = params;
  for (int l = 0; l < shape.n_linear; ++l) {
    const int n_in = shape.w[l], n_out = shape.w[l + 1];
    T* dst = lds + l * kMlpLayerFloats;
    for (int i = threadIdx.x; i < n_out * n_in; i += kMlpThreads) {
      const int o = i / n_in, k = i - o * n_in;
      dst[o * P + k] = src[i];
    }
    for (int i = threadIdx.x; i < n_out; i += kMlpThreads) dst[P * P + i] = src[n_out * n_in + i];
    src += n_out * n_in + n_out;
  }
  __syncthreads();
}

// StandardScaler.transform of one value: float(float(x - mean) / scale) with fp64 mean / scale, the two roundings of numpy's
// in-place float32 `X -= mean_; X /= scale_`.  (The training kernel's gather writes the same two lines out: calling this there
// moved amcx_mlp_train_kernel<2, 1>'s bytes in every spelling tried, and that kernel's bytes are held.)
__device__ inline float mlp_standardise(float v, double mean_j, double scale_j) {
  const float c = (float)((double)v - mean_j);
  return (float)((double)c / scale_j);
}

// the lane's rows of a tile: the column pick and the scaler (mean == nullptr: none); the padding is 0.  A row past the end
// reads the last row (its results are masked by the caller).
__device__ inline void mlp_load_rows(const float* __restrict__ x, long long n_rows, long long row_stride, const SelectCols& sel,
                                     const double* __restrict__ mean, const double* __restrict__ scale, long long tile,
                                     float (&h)[kMlpRowsPerLane][kMlpMaxWidth], long long (&row)[kMlpRowsPerLane]) {
  const bool scaled = mean != nullptr;
#pragma unroll
  for (int s = 0; s < kMlpRowsPerLane; ++s) {
    row[s] = tile * kMlpTileRows + s * kMlpThreads + (int)threadIdx.x;
    const long long rr = row[s] < n_rows ? row[s] : n_rows - 1;
    const float* xr = x + rr * row_stride;
#pragma unroll
    for (int j = 0; j < kMlpMaxWidth; ++j) {
      float v = 0.0f;
      if (j < sel.n) {
        v = xr[sel.c[j]];
        if (scaled) v = mlp_standardise(v, mean[j], scale[j]);
      }
      h[s][j] = v;
    }
  }
}

__device__ inline bool mlp_finite(float v) { return __builtin_fabsf(v) < __builtin_inff(); }

// a layer's sums: nx[o] = b[o] + sum_k W[o][k] h[k], float32 FMAs in the order bias, k = 0, 1, ...; the padding comes out 0
__device__ inline void mlp_dense_f32(const float* wl, int n_in, int n_out, const float (&h)[kMlpRowsPerLane][kMlpMaxWidth],
                                     float (&nx)[kMlpRowsPerLane][kMlpMaxWidth]) {
  constexpr int R = kMlpRowsPerLane, P = kMlpMaxWidth;
#pragma unroll
  for (int oc = 0; oc < P; oc += 8) {
    if (oc < n_out) {
      float acc[R][8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float b = wl[P * P + oc + j];
#pragma unroll
        for (int s = 0; s < R; ++s) acc[s][j] = b;
      }
#pragma unroll
      for (int kc = 0; kc < P; kc += 8) {
        if (kc < n_in) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float4 wa = *reinterpret_cast<const float4*>(wl + (oc + j) * P + kc);
            const float4 wb = *reinterpret_cast<const float4*>(wl + (oc + j) * P + kc + 4);
            const float w8[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
#pragma unroll
            for (int k = 0; k < 8; ++k) {
#pragma unroll
              for (int s = 0; s < R; ++s) acc[s][j] = __builtin_fmaf(w8[k], h[s][kc + k], acc[s][j]);
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int s = 0; s < R; ++s) nx[s][oc + j] = acc[s][j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int s = 0; s < R; ++s) nx[s][oc + j] = 0.0f;
      }
    }
  }
}

// the votes of slot s of a tile: counts[group][n_cls + 1], groups being consecutive blocks of rows_per_group rows.  The 64 rows
// of a wave's slot are consecutive, first .. last (uniform), in one group or a few: per group touched, one ballot + popcount
// per class and one 64-bit atomic per non-empty bin from lane 0.  A live row votes for `best`, or for the extra bin n_cls if
// it is not `finite`.  Every lane of the wave calls this.
__device__ inline void mlp_vote(long long tile, int s, long long row, bool live, bool finite, int best, int n_cls,
                                long long rows_per_group, unsigned long long* __restrict__ counts, long long n_rows) {
  const long long first = tile * kMlpTileRows + s * kMlpThreads + (long long)(threadIdx.x & ~63u);
  if (first < n_rows) {
    const long long last = first + 63 < n_rows ? first + 63 : n_rows - 1;
    const long long g_lo = first / rows_per_group, g_hi = last / rows_per_group;
    const int bin = finite ? best : n_cls;
    for (long long g = g_lo; g <= g_hi; ++g) {
      const long long lo = g * rows_per_group;
      const bool mine = live && row >= lo && row < lo + rows_per_group;
      for (int c = 0; c <= n_cls; ++c) {
        const unsigned long long votes = __ballot(mine && bin == c);
        if (votes != 0ull && (threadIdx.x & 63u) == 0u)
          atomicAdd(counts + g * (n_cls + 1) + c, (unsigned long long)__popcll(votes));
      }
    }
  }
}

}  // namespace amcx
