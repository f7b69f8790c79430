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
// ballot + popcount per class and group touched (one group, or two where a boundary falls inside the 64 rows), then one
// 64-bit vector atomic per non-empty bin from lane 0.
#pragma once

#include "amcx_mlp_shape.h"      // the limits, MlpShape and the activations
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

  // the packed block (per layer W[out][in] row-major, then b[out]) -> the padded copy
  for (int i = threadIdx.x; i < n_linear * kMlpLayerFloats; i += kMlpThreads) lds[i] = 0.0f;
  __syncthreads();
  {
    const float* src = params;
    for (int l = 0; l < n_linear; ++l) {
      const int n_in = shape.w[l], n_out = shape.w[l + 1];
      float* dst = lds + l * kMlpLayerFloats;
      for (int i = threadIdx.x; i < n_out * n_in; i += kMlpThreads) {
        const int o = i / n_in, k = i - o * n_in;
        dst[o * P + k] = src[i];
      }
      for (int i = threadIdx.x; i < n_out; i += kMlpThreads) dst[P * P + i] = src[n_out * n_in + i];
      src += n_out * n_in + n_out;
    }
  }
  __syncthreads();

  const bool scaled = mean != nullptr;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    float h[R][P];
    long long row[R];
#pragma unroll
    for (int s = 0; s < R; ++s) {
      row[s] = tile * kMlpTileRows + s * kMlpThreads + (int)threadIdx.x;
      const long long rr = row[s] < n_rows ? row[s] : n_rows - 1;      // past the end: a valid row, results masked
      const float* xr = x + rr * row_stride;
#pragma unroll
      for (int j = 0; j < P; ++j) {
        float v = 0.0f;
        if (j < sel.n) {
          v = xr[sel.c[j]];
          if (scaled) {
            const float c = (float)((double)v - mean[j]);
            v = (float)((double)c / scale[j]);
          }
        }
        h[s][j] = v;
      }
    }

    for (int l = 0; l < n_linear; ++l) {
      const int n_in = shape.w[l], n_out = shape.w[l + 1];
      const float* wl = lds + l * kMlpLayerFloats;
      const bool hidden = l + 1 < n_linear;
      float nx[R][P];
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
          finite = finite && __builtin_fabsf(p) < __builtin_inff();
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
      if (counts != nullptr) {
        // the 64 rows of this wave's slot are consecutive: first .. last (uniform), in one group or a few
        const long long first = tile * kMlpTileRows + s * kMlpThreads + (long long)(threadIdx.x & ~63u);
        if (first < n_rows) {
          const long long last = first + 63 < n_rows ? first + 63 : n_rows - 1;
          const long long g_lo = first / rows_per_group, g_hi = last / rows_per_group;
          const int bin = finite ? best : n_cls;
          for (long long g = g_lo; g <= g_hi; ++g) {
            const long long lo = g * rows_per_group;
            const bool mine = live && row[s] >= lo && row[s] < lo + rows_per_group;
            for (int c = 0; c <= n_cls; ++c) {
              const unsigned long long votes = __ballot(mine && bin == c);
              if (votes != 0ull && (threadIdx.x & 63u) == 0u)
                atomicAdd(counts + g * (n_cls + 1) + c, (unsigned long long)__popcll(votes));
            }
          }
        }
      }
    }
  }
}

}  // namespace amcx
