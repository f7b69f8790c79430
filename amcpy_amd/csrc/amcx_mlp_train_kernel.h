// Training of the classifier's network (the reference's nn_model.train_model: AMCClassifier in train() mode, CrossEntropyLoss on
// the softmax output, RMSprop or Adam) as ONE workgroup of 256 threads per model.  A launch runs steps step0 ... step0 + n_steps - 1
// of one epoch for every model of the grid; nothing but workgroup barriers stands between two steps.  include/amcx.h (ABI 16.1)
// fixes the state block, the workspace and the dropout generator; DESIGN.md 4.17 says why the layout is this one.
//
// Where things live.  LDS: the weights of every layer twice, W[o][k] for the forward chain and WT[k][o] for the backward one
// (both zero-padded to 32 x 32, read as wave-uniform float4), the BatchNorm gammas and betas, two batch x 33 gradient buffers
// (G and H below: a layer's z going forward, dZ / dA going back), the dropout mask words and the reduction scratch.  Global:
// the state block (parameters, running statistics, optimizer slots: one owner thread per value, read and written in place)
// and the workspace, which holds per model its hyperparameters and what backward needs of forward -- the gathered input rows X
// and, per hidden layer, xhat, the activation's output y and the layer's output a = dropout(y), each batch x 32.  The worst
// shape (6 layers of 32 at batch 256) needs 512 KiB of that, more than a CU's LDS, so every shape takes this one path.
//
// Who does what.  Dense forward and dA = dZ W: thread r owns row r (its 32 inputs in registers, the sums in the order
// bias, k = 0 ... 31; the padding contributes +-0).  dW = dZ^T A and db: thread t owns W[t >> 3][4 (t & 7) ... + 3], a float32
// fmaf chain over the rows r = 0, 1, ..., so the optimizer update of a value is its owner's alone.  Everything per feature over
// the batch (BatchNorm's statistics and its backward sums, db) is summed in float64 by 8 threads per feature, rows g, g + 8, ...,
// and combined in the order g = 0 ... 7 (the history's loss and count likewise): fixed orders everywhere, so a launch is bit-reproducible, and no atomic is needed.
//
// Hardware rules.  __syncthreads only; global writes are plain vector stores; no atomic, no spin loop, no grid-wide wait.
#pragma once

#include "amcx_mlp_shape.h"

namespace amcx {

constexpr int kOptRmsprop = 0, kOptAdam = 1;
constexpr int kTrainMaxBatch = 256;
constexpr int kTrainThreads = 256;
constexpr int kTrainGStride = kMlpMaxWidth + 1;                 // rows of G / H: 33 floats, so a thread per row meets no bank twice
constexpr int kTrainHyperWords = 8;                             // the head of a model's workspace: lr, threshold, keep_scale, seed lo / hi
constexpr int kTrainUploadModels = 128;                         // hyperparameters per upload launch (kernel arguments: 4 KiB at most)
constexpr int kTrainMaxHidden = kMlpMaxLinear - 1;
constexpr int kTrainRowGroups = kTrainThreads / kMlpMaxWidth;   // 8 threads per feature in the reductions over the batch

// what follows from a shape: the three parts of the state block and the slots behind them (include/amcx.h, THE STATE BLOCK)
struct TrainLayout {
  int n_params;       // W and b of every layer, the packed block's order
  int n_affine;       // gamma then beta of every BatchNorm, ascending layers
  int n_running;      // running mean then running variance of every BatchNorm
  int n_slots;        // 1 rmsprop, 2 adam
  __host__ __device__ int n_train() const { return n_params + n_affine; }
  __host__ __device__ long long state_floats() const { return (long long)n_train() * (1 + n_slots) + n_running; }
};
__host__ __device__ inline TrainLayout train_layout(const MlpShape& s, unsigned bn_mask, int opt) {
  TrainLayout t{0, 0, 0, opt == kOptAdam ? 2 : 1};
#pragma unroll
  for (int l = 0; l < kMlpMaxLinear; ++l) {
    if (l < s.n_linear) {
      t.n_params += s.w[l + 1] * s.w[l] + s.w[l + 1];
      if (l + 1 < s.n_linear && ((bn_mask >> l) & 1u)) {
        t.n_affine += 2 * s.w[l + 1];
        t.n_running += 2 * s.w[l + 1];
      }
    }
  }
  return t;
}
__host__ __device__ inline long long train_ws_floats(int n_linear, int batch) {
  return kTrainHyperWords + (long long)batch * kMlpMaxWidth * (1 + 3 * (n_linear - 1));
}

// bytes of dynamic LDS at this batch size
constexpr int kTrainLdsDoubles = kTrainRowGroups * kMlpMaxWidth * 2 + kTrainMaxHidden * kMlpMaxWidth + kTrainMaxBatch + 2 * kTrainRowGroups;
constexpr int kTrainLdsWords = kMlpMaxLinear * kMlpLayerFloats + kMlpMaxLinear * kMlpMaxWidth * kMlpMaxWidth +
                               2 * kTrainMaxHidden * kMlpMaxWidth + kTrainMaxHidden * kTrainMaxBatch + kTrainMaxBatch + kMlpMaxWidth + 32;
__host__ __device__ constexpr int train_lds_bytes(int batch) {
  return kTrainLdsDoubles * 8 + kTrainLdsWords * 4 + 2 * batch * kTrainGStride * 4;
}

struct TrainHyperChunk {
  float lr[kTrainUploadModels];
  unsigned thr[kTrainUploadModels];
  float keep[kTrainUploadModels];
  unsigned seed_lo[kTrainUploadModels];
  unsigned seed_hi[kTrainUploadModels];
};

// the hyperparameters of models first ... first + n - 1 into the heads of their workspaces: host arrays reach the device as
// kernel arguments, so the entry allocates nothing, copies nothing and can be captured in a graph
__global__ __launch_bounds__(kTrainUploadModels) void amcx_mlp_train_hyper_kernel(TrainHyperChunk h, int n, float* __restrict__ ws,
                                                                                  long long ws_floats, int first) {
  // the arguments lie in constant memory, which a lane reads at an index of its own as it reads any global memory
  const unsigned* __restrict__ words = reinterpret_cast<const unsigned*>(&h);
  const int i = threadIdx.x;
  if (i >= n) return;
  float* w = ws + (long long)(first + i) * ws_floats;
#pragma unroll
  for (int f = 0; f < 5; ++f) w[f] = __uint_as_float(words[f * kTrainUploadModels + i]);
  w[5] = 0.0f;
  w[6] = 0.0f;
  w[7] = 0.0f;
}

// Philox4x32-10 (Salmon et al., SC'11): counter c, key k -> four words
__device__ inline void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&out)[4]) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0;
    c1 = lo1;
    c2 = n2;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// the activation's derivative from its stored output
template <int ACT>
__device__ inline float mlp_act_grad(float yv) {
  if (ACT == kActRelu) return yv > 0.0f ? 1.0f : 0.0f;
  if (ACT == kActTanh) return 1.0f - yv * yv;
  return yv * (1.0f - yv);
}

// what an optimizer step needs beside the gradient: uniform over the workgroup and the step
struct TrainStep {
  float lr;
  float step_size;      // adam: lr / (1 - beta1^t)
  float bc2_sqrt;       // adam: sqrt(1 - beta2^t)
};

// one value's update, torch's formulas in float32; `i` is the value's index among the trainable ones, its slots stand at
// slot0 + s * n_train + i.  Returns the new value, which the caller stores wherever it keeps copies.
template <int OPT>
__device__ inline float train_update(float* __restrict__ st, long long slot0, int n_train, int i, float g, const TrainStep& ts) {
  const float w = st[i];
  float nw;
  if (OPT == kOptRmsprop) {
    float v = st[slot0 + i];
    v = v * 0.99f + (0.01f * g) * g;
    st[slot0 + i] = v;
    nw = w - ts.lr * (g / (sqrtf(v) + 1e-8f));
  } else {
    float m = st[slot0 + i], v = st[slot0 + n_train + i];
    m = m + (g - m) * 0.1f;
    v = v * 0.999f + (0.001f * g) * g;
    st[slot0 + i] = m;
    st[slot0 + n_train + i] = v;
    nw = w - ts.step_size * (m / (sqrtf(v) / ts.bc2_sqrt + 1e-8f));
  }
  st[i] = nw;
  return nw;
}

#define AMCX_TRAIN_PARAMS                                                                                                        \
  const float* __restrict__ x, long long n_rows, long long row_stride, SelectCols sel, const double* __restrict__ mean,          \
      const double* __restrict__ scale, const int* __restrict__ y, const int* __restrict__ idx, long long n_idx,                 \
      long long idx_model_stride, MlpShape shape, unsigned bn_mask, int batch, float* __restrict__ state,                         \
      long long* __restrict__ steps, float* __restrict__ ws, long long step0, int n_steps, double* __restrict__ history

template <int ACT, int OPT>
__device__ __forceinline__ void train_body(AMCX_TRAIN_PARAMS) {
  constexpr int P = kMlpMaxWidth, GS = kTrainGStride, NB = kTrainMaxBatch;
  extern __shared__ double train_lds[];
  // ---- the carve-up (doubles first) ----
  double* const part = train_lds;                                       // [8][32][2]
  double* const rstd = part + kTrainRowGroups * P * 2;                  // [5][32]: a BatchNorm's 1 / sqrt(var + eps) of this step
  double* const lossr = rstd + kTrainMaxHidden * P;                     // [256]: a row's loss
  double* const hred = lossr + NB;                                      // [8][2]: a row group's summed loss and right rows
  float* const W = reinterpret_cast<float*>(hred + 2 * kTrainRowGroups);   // [6][32 * 32 + 32]
  float* const WT = W + kMlpMaxLinear * kMlpLayerFloats;                // [6][32][32]
  float* const gam = WT + kMlpMaxLinear * P * P;                        // [5][32]
  float* const bet = gam + kTrainMaxHidden * P;                         // [5][32]
  unsigned* const maskw = reinterpret_cast<unsigned*>(bet + kTrainMaxHidden * P);   // [5][256]: bit o = unit o of the row kept
  int* const corr = reinterpret_cast<int*>(maskw + kTrainMaxHidden * NB);           // [256]: the row's argmax is its class
  int* const cols = corr + NB;                                          // [32]
  int* const wd = cols + P;                                             // [8] widths; [8] parameter offsets; [8] affine; [8] running
  int* const poff = wd + 8;
  int* const aoff = poff + 8;
  int* const roff = aoff + 8;
  float* const buf0 = reinterpret_cast<float*>(roff + 8);               // [batch][33]
  float* const buf1 = buf0 + batch * GS;

  const int tid = threadIdx.x;
  const int model = blockIdx.x;
  const int n_linear = shape.n_linear, n_cls = shape.w[n_linear];
  const TrainLayout lay = train_layout(shape, bn_mask, OPT);
  const int n_train = lay.n_train();
  float* const st = state + (long long)model * lay.state_floats();
  float* const run = st + n_train;                                      // the running statistics
  const long long slot0 = (long long)n_train + lay.n_running;           // the first optimizer slot
  const long long ws_floats = train_ws_floats(n_linear, batch);
  float* const wsm = ws + (long long)model * ws_floats;
  float* const X = wsm + kTrainHyperWords;
  const long long lbuf = (long long)batch * P;
  const float lr = wsm[0], keep_scale = wsm[2];
  const unsigned thr = __float_as_uint(wsm[1]), seed_lo = __float_as_uint(wsm[3]), seed_hi = __float_as_uint(wsm[4]);
  const int* const order = idx + (long long)model * idx_model_stride;

  // ---- the shape into LDS (static indices here, run-time ones from there), the parameters into their padded copies ----
  if (tid == 0) {
    int p = 0, a = 0;
#pragma unroll
    for (int l = 0; l <= kMlpMaxLinear; ++l) wd[l] = shape.w[l];
#pragma unroll
    for (int l = 0; l < kMlpMaxLinear; ++l) {
      poff[l] = p;
      aoff[l] = a;
      roff[l] = a;
      if (l < n_linear) {
        p += shape.w[l + 1] * shape.w[l] + shape.w[l + 1];
        if (l + 1 < n_linear && ((bn_mask >> l) & 1u)) a += 2 * shape.w[l + 1];
      }
    }
  }
  if (tid < P) {
    int c = 0;
#pragma unroll
    for (int j = 0; j < P; ++j)
      if (tid == j) c = sel.c[j];
    cols[tid] = c;
  }
  for (int i = tid; i < kMlpMaxLinear * kMlpLayerFloats; i += kTrainThreads) W[i] = 0.0f;
  for (int i = tid; i < kMlpMaxLinear * P * P; i += kTrainThreads) WT[i] = 0.0f;
  for (int i = tid; i < kTrainMaxHidden * P; i += kTrainThreads) {
    gam[i] = 0.0f;
    bet[i] = 0.0f;
  }
  __syncthreads();
  for (int l = 0; l < n_linear; ++l) {
    const int n_in = wd[l], n_out = wd[l + 1];
    const float* src = st + poff[l];
    for (int i = tid; i < n_out * n_in; i += kTrainThreads) {
      const int o = i / n_in, k = i - o * n_in;
      const float v = src[i];
      W[l * kMlpLayerFloats + o * P + k] = v;
      WT[l * P * P + k * P + o] = v;
    }
    for (int i = tid; i < n_out; i += kTrainThreads) W[l * kMlpLayerFloats + P * P + i] = src[n_out * n_in + i];
    if (l + 1 < n_linear && ((bn_mask >> l) & 1u)) {
      for (int i = tid; i < n_out; i += kTrainThreads) {
        gam[l * P + i] = st[lay.n_params + aoff[l] + i];
        bet[l * P + i] = st[lay.n_params + aoff[l] + n_out + i];
      }
    }
  }
  const long long t_first = steps[model];
  double hist_loss = 0.0, hist_corr = 0.0;
  if (tid == 0) {
    hist_loss = history[2 * model];
    hist_corr = history[2 * model + 1];
  }
  __syncthreads();

  const bool scaled = mean != nullptr;
  const int fo = tid & (P - 1), fg = tid >> 5;          // the per-feature phases: feature and row group
  const int wo = tid >> 3, wq = tid & 7;                // the weight-gradient phase: output and block of four inputs

  for (int si = 0; si < n_steps; ++si) {
    const long long first = (step0 + si) * (long long)batch;
    const int nb = (int)(n_idx - first < batch ? n_idx - first : batch);
    const long long t_now = t_first + si;               // the model's step count before this step
    TrainStep ts;
    ts.lr = lr;
    ts.step_size = lr;
    ts.bc2_sqrt = 1.0f;
    if (OPT == kOptAdam) {
      const double tt = (double)(t_now + 1);
      ts.step_size = (float)((double)lr / (1.0 - pow(0.9, tt)));
      ts.bc2_sqrt = (float)sqrt(1.0 - pow(0.999, tt));
    }
    const double inv_nb = 1.0 / (double)nb;

    // ---- the batch's rows: gathered by index, picked by column, standardised with the scaler's two roundings ----
    for (int i = tid; i < nb * P; i += kTrainThreads) {
      const int r = i >> 5, j = i & (P - 1);
      float v = 0.0f;
      if (j < sel.n) {
        long long row = order[first + r];
        row = row < 0 ? 0 : row >= n_rows ? n_rows - 1 : row;        // an index outside the matrix is the caller's error: no read follows it
        v = x[row * row_stride + cols[j]];
        if (scaled) {
          const float c = (float)((double)v - mean[j]);
          v = (float)((double)c / scale[j]);
        }
      }
      X[i] = v;
    }
    __syncthreads();

    // ---- forward ----
    float* G = buf0;
    float* H = buf1;
    for (int l = 0; l < n_linear; ++l) {
      const int n_out = wd[l + 1];
      const bool hidden = l + 1 < n_linear;
      const bool bn = hidden && ((bn_mask >> l) & 1u);
      const float* wl = W + l * kMlpLayerFloats;
      const float* src = l == 0 ? X : wsm + kTrainHyperWords + lbuf * (1 + 3 * (l - 1) + 2);      // a of the layer before
      if (tid < nb) {
        const int r = tid;
        float h[P];
#pragma unroll
        for (int k = 0; k < P; k += 4) {
          const float4 v = *reinterpret_cast<const float4*>(src + r * P + k);
          h[k] = v.x;
          h[k + 1] = v.y;
          h[k + 2] = v.z;
          h[k + 3] = v.w;
        }
        float* gr = G + r * GS;
        for (int o = 0; o < n_out; ++o) {
          float acc = wl[P * P + o];
#pragma unroll
          for (int k = 0; k < P; k += 4) {
            const float4 w4 = *reinterpret_cast<const float4*>(wl + o * P + k);
            acc = __builtin_fmaf(w4.x, h[k], acc);
            acc = __builtin_fmaf(w4.y, h[k + 1], acc);
            acc = __builtin_fmaf(w4.z, h[k + 2], acc);
            acc = __builtin_fmaf(w4.w, h[k + 3], acc);
          }
          gr[o] = acc;
        }
        if (hidden) {
          unsigned m = 0xffffffffu;
          if (thr != 0u) {
            m = 0u;
            for (int q = 0; q * 4 < n_out; ++q) {
              unsigned wds[4];
              philox4x32_10((unsigned)t_now, (unsigned)l, (unsigned)r, (unsigned)q, seed_lo, seed_hi, wds);
#pragma unroll
              for (int j = 0; j < 4; ++j) m |= (wds[j] >= thr ? 1u : 0u) << (q * 4 + j);
            }
          }
          maskw[l * NB + r] = m;
        } else {
          // p = softmax(z); the reference's loss on it: q = softmax(p), loss = -log q[y]; dz = p * (dp - sum_j p_j dp_j).
          // From the float32 sums z on, this chain runs in float64 and dz is rounded once: in float32 its exps, quotients and
          // the difference dp - dot cost some 4 ulp of dz, which the optimizers' second moments show (g * g) -- more than the
          // tolerance leaves where torch's own float32 error happens to be small.  p is parked as a float32 pair (hi in G, lo in H).
          float* hr = H + r * GS;
          float zmf = gr[0];
          for (int j = 1; j < n_cls; ++j) zmf = gr[j] > zmf ? gr[j] : zmf;
          const double zm = (double)zmf;
          double sum = 0.0;
          for (int j = 0; j < n_cls; ++j) sum += exp((double)gr[j] - zm);
          int best = 0;
          double pbest = 0.0;
          for (int j = 0; j < n_cls; ++j) {
            const double p = exp((double)gr[j] - zm) / sum;
            const float hi = (float)p;
            gr[j] = hi;
            hr[j] = (float)(p - (double)hi);
            if (j == 0 || p > pbest) {           // strictly greater: the first maximum wins
              best = j;
              pbest = p;
            }
          }
          double sum2 = 0.0;
          for (int j = 0; j < n_cls; ++j) sum2 += exp(((double)gr[j] + (double)hr[j]) - pbest);
          long long row = order[first + r];
          row = row < 0 ? 0 : row >= n_rows ? n_rows - 1 : row;
          const int cls = y[row];
          const double inv_rows = 1.0 / (double)nb;
          double dot = 0.0, py = pbest;
          for (int j = 0; j < n_cls; ++j) {
            const double p = (double)gr[j] + (double)hr[j];
            if (j == cls) py = p;
            dot += p * ((exp(p - pbest) / sum2 - (j == cls ? 1.0 : 0.0)) * inv_rows);
          }
          for (int j = 0; j < n_cls; ++j) {
            const double p = (double)gr[j] + (double)hr[j];
            const double dp = (exp(p - pbest) / sum2 - (j == cls ? 1.0 : 0.0)) * inv_rows;
            gr[j] = (float)(p * (dp - dot));
          }
          lossr[r] = cls >= 0 && cls < n_cls ? -((py - pbest) - log(sum2)) : 0.0;      // -log q[y]; a class outside matches none
          corr[r] = best == cls ? 1 : 0;
        }
      }
      __syncthreads();
      if (hidden) {
        float* const xh = wsm + kTrainHyperWords + lbuf * (1 + 3 * l);
        float* const yo = xh + lbuf;
        float* const ao = yo + lbuf;
        double mu = 0.0, rs = 1.0;
        if (bn) {
          double s1 = 0.0, s2 = 0.0;
          if (fo < n_out) {                 // the columns beyond hold nothing of this layer
            for (int r = fg; r < nb; r += kTrainRowGroups) {
              const double z = (double)G[r * GS + fo];
              s1 += z;
              s2 += z * z;
            }
          }
          part[(fg * P + fo) * 2] = s1;
          part[(fg * P + fo) * 2 + 1] = s2;
          __syncthreads();
          s1 = 0.0;
          s2 = 0.0;
#pragma unroll
          for (int g = 0; g < kTrainRowGroups; ++g) {
            s1 += part[(g * P + fo) * 2];
            s2 += part[(g * P + fo) * 2 + 1];
          }
          mu = s1 * inv_nb;
          double var = s2 * inv_nb - mu * mu;
          var = var < 0.0 ? 0.0 : var;
          rs = 1.0 / sqrt(var + 1e-5);
          if (fg == 0 && fo < n_out) {
            rstd[l * P + fo] = rs;
            float* rm = run + roff[l];
            rm[fo] = (float)(0.9 * (double)rm[fo] + 0.1 * mu);
            rm[n_out + fo] = (float)(0.9 * (double)rm[n_out + fo] + 0.1 * (var * ((double)nb / (double)(nb - 1))));
          }
        }
        const float gm = gam[l * P + fo], bt = bet[l * P + fo];
        for (int r = fg; r < nb; r += kTrainRowGroups) {
          float xhat = 0.0f, yv = 0.0f, av = 0.0f;
          if (fo < n_out) {
            const float z = G[r * GS + fo];
            float v = z;
            if (bn) {
              xhat = (float)(((double)z - mu) * rs);
              v = __builtin_fmaf(gm, xhat, bt);
            }
            yv = mlp_act<ACT>(v);
            av = ((maskw[l * NB + r] >> fo) & 1u) ? yv * keep_scale : 0.0f;
          }
          xh[r * P + fo] = xhat;
          yo[r * P + fo] = yv;
          ao[r * P + fo] = av;
        }
        __syncthreads();
      }
    }

    // ---- the history: the batch's summed loss and its count of right rows, in a fixed order: eight threads sum the rows
    // g, g + 8, ... here, thread 0 adds the eight sums in the order g = 0 ... 7 behind the next barrier ----
    if (tid < kTrainRowGroups) {
      double bl = 0.0;
      int bc = 0;
      for (int r = tid; r < nb; r += kTrainRowGroups) {
        bl += lossr[r];
        bc += corr[r];
      }
      hred[tid * 2] = bl;
      hred[tid * 2 + 1] = (double)bc;
    }

    // ---- backward: G holds dZ of the last layer ----
    for (int l = n_linear - 1; l >= 0; --l) {
      const int n_in = wd[l], n_out = wd[l + 1];
      const float* src = l == 0 ? X : wsm + kTrainHyperWords + lbuf * (1 + 3 * (l - 1) + 2);
      // dW[wo][4 wq ...] and db[wo]
      float dw[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      double db = 0.0;
      if (wo < n_out && wq * 4 < n_in) {
#pragma unroll 4
        for (int r = 0; r < nb; ++r) {
          const float g = G[r * GS + wo];
          const float4 a4 = *reinterpret_cast<const float4*>(src + r * P + wq * 4);
          dw[0] = __builtin_fmaf(g, a4.x, dw[0]);
          dw[1] = __builtin_fmaf(g, a4.y, dw[1]);
          dw[2] = __builtin_fmaf(g, a4.z, dw[2]);
          dw[3] = __builtin_fmaf(g, a4.w, dw[3]);
          if (wq == 0) db += (double)g;
        }
      }
      // In front of a BatchNorm db is identically zero -- the batch mean is subtracted -- and the float64 statement's is rounding
      // noise of 1e-18, which the optimizers' eps turns into no movement at all.  A float32 sum's noise of 1e-10 would instead
      // walk the bias by lr / 100 a step in a random direction (both optimizers divide by 1e-8 there): the identity is taken.
      if (l + 1 < n_linear && ((bn_mask >> l) & 1u)) db = 0.0;
      // dA = dZ W through the dropout and the activation of the layer before, into H
      if (l > 0 && tid < nb) {
        const int r = tid;
        const float* wt = WT + l * P * P;
        const float* yo = wsm + kTrainHyperWords + lbuf * (1 + 3 * (l - 1) + 1);
        float g[P];
#pragma unroll
        for (int o = 0; o < P; ++o) g[o] = o < n_out ? G[r * GS + o] : 0.0f;
        const unsigned m = maskw[(l - 1) * NB + r];
        for (int k = 0; k < n_in; ++k) {
          float acc = 0.0f;
#pragma unroll
          for (int o = 0; o < P; o += 4) {
            const float4 w4 = *reinterpret_cast<const float4*>(wt + k * P + o);
            acc = __builtin_fmaf(g[o], w4.x, acc);
            acc = __builtin_fmaf(g[o + 1], w4.y, acc);
            acc = __builtin_fmaf(g[o + 2], w4.z, acc);
            acc = __builtin_fmaf(g[o + 3], w4.w, acc);
          }
          const float dy = ((m >> k) & 1u) ? acc * keep_scale : 0.0f;
          H[r * GS + k] = dy * mlp_act_grad<ACT>(yo[r * P + k]);
        }
      }
      __syncthreads();
      if (tid == 0 && l == n_linear - 1) {
        double bl = 0.0, bc = 0.0;
#pragma unroll
        for (int g = 0; g < kTrainRowGroups; ++g) {
          bl += hred[g * 2];
          bc += hred[g * 2 + 1];
        }
        hist_loss += bl;
        hist_corr += bc;
      }
      // the layer's update: every value by the thread that summed its gradient
      if (wo < n_out) {
        float* wl = W + l * kMlpLayerFloats;
        float* wt = WT + l * P * P;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int k = wq * 4 + i;
          if (k < n_in) {
            const float nw = train_update<OPT>(st, slot0, n_train, poff[l] + wo * n_in + k, dw[i], ts);
            wl[wo * P + k] = nw;
            wt[k * P + wo] = nw;
          }
        }
        if (wq == 0) wl[P * P + wo] = train_update<OPT>(st, slot0, n_train, poff[l] + n_out * n_in + wo, (float)db, ts);
      }
      // BatchNorm of the layer before: H holds the gradient behind it and becomes the one in front of it
      if (l > 0 && ((bn_mask >> (l - 1)) & 1u)) {
        const float* xh = wsm + kTrainHyperWords + lbuf * (1 + 3 * (l - 1));
        const float gm = gam[(l - 1) * P + fo];
        double s1 = 0.0, s2 = 0.0;
        if (fo < n_in) {
          for (int r = fg; r < nb; r += kTrainRowGroups) {
            const double d = (double)H[r * GS + fo];
            s1 += d;
            s2 += d * (double)xh[r * P + fo];
          }
        }
        part[(fg * P + fo) * 2] = s1;
        part[(fg * P + fo) * 2 + 1] = s2;
        __syncthreads();
        s1 = 0.0;
        s2 = 0.0;
#pragma unroll
        for (int g = 0; g < kTrainRowGroups; ++g) {
          s1 += part[(g * P + fo) * 2];
          s2 += part[(g * P + fo) * 2 + 1];
        }
        if (fo < n_in) {
          const double k0 = (double)gm * rstd[(l - 1) * P + fo];
          const double m1 = s1 * inv_nb, m2 = s2 * inv_nb;
          for (int r = fg; r < nb; r += kTrainRowGroups) {
            const double d = (double)H[r * GS + fo];
            H[r * GS + fo] = (float)(k0 * (d - m1 - (double)xh[r * P + fo] * m2));
          }
        }
        __syncthreads();                 // every reader of gamma is past it
        if (fg == 0 && fo < n_in) {
          const int a = lay.n_params + aoff[l - 1];
          gam[(l - 1) * P + fo] = train_update<OPT>(st, slot0, n_train, a + fo, (float)s2, ts);
          bet[(l - 1) * P + fo] = train_update<OPT>(st, slot0, n_train, a + n_in + fo, (float)s1, ts);
        }
      }
      float* const swap = G;
      G = H;
      H = swap;
    }
    __syncthreads();
  }

  if (tid == 0) {
    history[2 * model] = hist_loss;
    history[2 * model + 1] = hist_corr;
    steps[model] = t_first + n_steps;
  }
}

// The kernels: explicit specialisations, which are laid out HERE, ahead of every other kernel of the library, and not where the
// host code first names an instantiation: code laid out behind an existing kernel would move the distances some of them hold
// (KERNEL ORDER, amcx_launch.h).
template <int ACT, int OPT>
__global__ void amcx_mlp_train_kernel(AMCX_TRAIN_PARAMS);
#define AMCX_TRAIN_KERNEL(ACT, OPT)                                                                             \
  template <>                                                                                                   \
  __global__ __launch_bounds__(kTrainThreads) void amcx_mlp_train_kernel<ACT, OPT>(AMCX_TRAIN_PARAMS) {         \
    train_body<ACT, OPT>(x, n_rows, row_stride, sel, mean, scale, y, idx, n_idx, idx_model_stride, shape, bn_mask, batch, state, \
                         steps, ws, step0, n_steps, history);                                                   \
  }
AMCX_TRAIN_KERNEL(kActRelu, kOptRmsprop)
AMCX_TRAIN_KERNEL(kActTanh, kOptRmsprop)
AMCX_TRAIN_KERNEL(kActSigmoid, kOptRmsprop)
AMCX_TRAIN_KERNEL(kActRelu, kOptAdam)
AMCX_TRAIN_KERNEL(kActTanh, kOptAdam)
AMCX_TRAIN_KERNEL(kActSigmoid, kOptAdam)
#undef AMCX_TRAIN_KERNEL
#undef AMCX_TRAIN_PARAMS

}  // namespace amcx
