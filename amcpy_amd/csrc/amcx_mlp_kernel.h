// The classifier behind the feature matrix (the reference's nn_model.AMCClassifier in eval() mode and the
// `model(x_t).argmax(1)` of its evaluate_by_snr), as ONE launch over the device-resident (rows x n_cols) float32
// matrix: column pick + StandardScaler.transform, the dense layers (BatchNorm folded into weights and bias by the
// caller, include/amcx.h), softmax, argmax and the per-group histogram of the labels.
//
// Layout.  One workgroup of 256 threads walks tiles of kMlpTileRows rows; a lane holds kMlpRowsPerLane rows, slot s of
// lane t of a tile being row  tile * kMlpTileRows + s * 256 + t  (so a wave's slot covers 64 consecutive rows and its
// label store is one 256-byte line).  The parameters are the same for every lane: the workgroup copies them once into
// LDS, every layer zero-padded to a 32 x 32 weight matrix plus 32 biases, and the FMAs take them from there with
// wave-uniform addresses (ds_read_b128 broadcasts, 8 weights of one output per pair of reads, shared by the lane's
// rows).  Activations live in registers with compile-time indices: widths are run-time values, handled in blocks of 8
// (outputs and inputs) behind wave-uniform branches, the padding being zero weights.  A padded output is
// 0 + 0 * h ..., at most act(0), finite for every activation here, and meets only zero weights in the next layer.
//
// Arithmetic.  float32 FMAs, every output's sum taken in the order bias, k = 0, 1, ..., K-1 (the zero-weight padding
// adds +-0 to it, which leaves the value as it is), one row's result independent of every other row and of the lane and
// slot it lands in: a row's bits do not depend on how rows are batched.  The scaler is the two roundings of
// amcx_select_scale_kernel, float(float(x - mean) / scale) with fp64 mean / scale.  Softmax subtracts the row maximum
// as torch does; argmax takes the first maximum as torch does.
//
// NaN rule (a deliberate difference from the reference).  A row whose probabilities are not all finite -- a NaN
// kurtosis of a constant frame, a column a feature subset left NaN, an inf -- keeps the probabilities as they come out,
// gets label -1 and is counted in the extra last bin.  The reference's argmax of an all-NaN row answers class 0 (BPSK).
//
// Counts.  counts[group][n_classes + 1], groups being consecutive blocks of rows_per_group rows: per wave and slot, one
// ballot + popcount per class and group touched (one group, or more where boundaries fall inside the 64 rows), then one
// 64-bit vector atomic per non-empty bin from lane 0.
//
// The routines.  Staging, row load, a layer's sums and the votes are mlp_stage_params, mlp_load_rows, mlp_dense_f32 and
// mlp_vote of amcx_mlp_shape.h, which the range calibration and the integer network (amcx_mlp_q15_kernel.h) call too; the
// scaler is its mlp_standardise.  What stands here is the tile loop, the layer loop with the activation choice, the
// softmax / argmax with the NaN rule (nothing else computes it in float32) and the stores.
#pragma once

#include "amcx_mlp_shape.h"      // the limits, MlpShape, the activations and the routines
#include "amcx_post_kernels.h"

namespace amcx {

// counts <- 0 ahead of the classifier launch, on the same stream.  A kernel rather than hipMemsetAsync: inside a captured
// graph the runtime's memset node filled the bins with other bytes from the second replay on (seen with ROCm 7.0 on
// gfx950, tests/test_gpu_classifier.py::test_graph_capture_replays_to_the_same_bits); a kernel node replays as launched.
__global__ __launch_bounds__(256) void amcx_mlp_zero_counts_kernel(unsigned long long* __restrict__ counts, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) counts[i] = 0ull;
}

__global__ __launch_bounds__(kMlpThreads) void amcx_mlp_classify_kernel(
    const float* __restrict__ x, long long n_rows, long long row_stride, SelectCols sel,
    const double* __restrict__ mean, const double* __restrict__ scale, const float* __restrict__ params, MlpShape shape,
    int* __restrict__ labels, float* __restrict__ probs, long long probs_stride, long long rows_per_group,
    unsigned long long* __restrict__ counts, long long n_tiles) {
  constexpr int R = kMlpRowsPerLane, P = kMlpMaxWidth;
  __shared__ float4 lds4[kMlpMaxLinear * kMlpLayerFloats / 4];
  float* lds = reinterpret_cast<float*>(lds4);
  const int n_linear = shape.n_linear, n_cls = shape.w[n_linear];

  mlp_stage_params(lds, params, shape);

  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    float h[R][P];
    long long row[R];
    mlp_load_rows(x, n_rows, row_stride, sel, mean, scale, tile, h, row);

    for (int l = 0; l < n_linear; ++l) {
      const int n_in = shape.w[l], n_out = shape.w[l + 1];
      const float* wl = lds + l * kMlpLayerFloats;
      const bool hidden = l + 1 < n_linear;
      float nx[R][P];
      mlp_dense_f32(wl, n_in, n_out, h, nx);
      if (hidden) {                        // one uniform choice per layer, not one per element
        if (shape.act == kActRelu) mlp_act_all<kActRelu>(nx, n_out);
        else if (shape.act == kActTanh) mlp_act_all<kActTanh>(nx, n_out);
        else mlp_act_all<kActSigmoid>(nx, n_out);
      }
#pragma unroll
      for (int s = 0; s < R; ++s) {
#pragma unroll
        for (int j = 0; j < P; ++j) h[s][j] = nx[s][j];
      }
    }

#pragma unroll
    for (int s = 0; s < R; ++s) {
      // softmax as torch: exp(z - max) / sum; the maximum skips nothing (a NaN makes every probability NaN below)
      float m = h[s][0];
#pragma unroll
      for (int j = 1; j < P; ++j)
        if (j < n_cls) m = h[s][j] > m ? h[s][j] : m;
      float sum = 0.0f;
#pragma unroll
      for (int j = 0; j < P; ++j) {
        if (j < n_cls) {
          h[s][j] = expf(h[s][j] - m);
          sum += h[s][j];
        }
      }
      int best = 0;
      float pbest = 0.0f;
      bool finite = true;
#pragma unroll
      for (int j = 0; j < P; ++j) {
        if (j < n_cls) {
          const float p = h[s][j] / sum;
          h[s][j] = p;
          finite = finite && mlp_finite(p);
          if (j == 0 || p > pbest) {           // strictly greater: the first maximum wins
            best = j;
            pbest = p;
          }
        }
      }
      const int label = finite ? best : -1;
      const bool live = row[s] < n_rows;
      if (live) {
        if (labels != nullptr) labels[row[s]] = label;
        if (probs != nullptr) {
          float* pr = probs + row[s] * probs_stride;
#pragma unroll
          for (int j = 0; j < P; ++j)
            if (j < n_cls) pr[j] = h[s][j];
        }
      }
      if (counts != nullptr) mlp_vote(tile, s, row[s], live, finite, best, n_cls, rows_per_group, counts, n_rows);
    }
  }
}

}  // namespace amcx
