// What the kernels over the feature matrix share and no kernel of: the column selection of the post-processing entries, the
// limits and the shape of the dense network, and its activations (amcx_post_kernels.h, amcx_mlp_kernel.h,
// amcx_mlp_q15_kernel.h).  No kernel stands here, so including it ahead of others moves nothing in .text (KERNEL ORDER,
// amcx_launch.h).
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

}  // namespace amcx
