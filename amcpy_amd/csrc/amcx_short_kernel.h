// N = 128, 256 and 512 (RadioML-2016-style short frames): FOUR frames per wavefront, sixteen lanes per frame.
//
// The one-wave-per-frame kernel (amcx_wave_kernel.h) spreads a 128-sample frame over 64 lanes, two samples each: every
// frame then pays a full 64-lane reduction of its 27 sums, another for the envelope's mean, and shares a 1024-point-shaped
// FFT back half with seven other frames -- 327 VALU instructions per frame where the per-sample work is ~210, and at FULL
// clock (not the board's power cap) a quarter of its wave-cycles in s_waitcnt (profiles/r5_short_kernel_ab.txt).  Here a
// frame lives in ONE 16-lane DPP row (247 instructions per frame at N = 128):
//   * lane l of a row holds samples 32 j + 2 l + b, j < 4, b < 2 (four global_load_dwordx4, 256 contiguous bytes per row
//     and load); the statistics sweep is the wave kernel's, with the neighbour's angle from a row rotate (row_ror:15) and
//     the shifts from the row's first 16 samples;
//   * every reduction is a row reduction: four DPP steps (quad xor 1, xor 2, half-mirror, mirror) leave the total in all
//     sixteen lanes -- the mean envelope costs 4 instructions instead of a wave reduction, the 27 sums 108 for FOUR frames;
//   * every frame is multiplied by 2^-ex first (ex the even-rounded exponent of its largest component, a row maximum), as
//     the block kernel does, and finalised through the features' scaling laws (finalize_features<true>): no range check, no
//     re-run pass, any float32 input;
//   * the 128-point FFT, X[kj + 4 (kc + 8 ka)]: pass 1 radix 4 over j in registers (twiddle W_128^(m kj), m = 2 l + b),
//     a transpose through LDS so that lane (kj, a) holds y[kj][4 c + a], c < 8; pass 2 radix 8 over c in registers (twiddle
//     W_32^(a kc)); a second transpose so that lane (kj, h) holds z[kj][kc = 2 h + e][a], a < 4; pass 3 radix 4 over a.
//     All three passes are the wave kernel's compile-time dif<>; the four frames of a wave go through together;
//   * after eight passes (32 frames; four passes at N = 256 / 512) lanes 0-31 turn a stash row each into 18 features in fp64; frames with a phase step
//     within an angle rounding of +-pi get f5 / f9 from the exact fp64 sweep (wave_exact_frequency).
// N = 256 is the same machine with eight rows per lane: pass 1 is a radix 8 over j, and a lane takes TWO of the eight
// 32-point transforms of passes 2 and 3 (kj = l / 4 and l / 4 + 4), one after the other.  N = 512 has sixteen rows per lane:
// pass 1 is a radix 16 over j, its sixteen 32-point transforms go through the exchange block in two batches of eight, only
// four of the sixteen rows are requested a pass ahead (the rest at the head of the pass: with eight ahead three of them were
// stored to scratch straight from their loads), and |x| is parked in the exchange block for the envelope's second sweep.
// N = 128: 16 waves per CU (116 VGPRs); N = 256 / 512: 12 (143 / 162 VGPRs; a 9.5 KB exchange block per wave).  No barrier in the frame loop,
// nothing shared between waves but the twiddle tables.  Algorithmic HBM bytes per frame: 8 N + 72.
#pragma once

#include "amcx_wave_kernel.h"

namespace amcx {
namespace shortk {

using namespace wave;

constexpr int kRowRor15 = 0x12F;                             // DPP row_ror:15: lane l reads lane (l + 1) mod 16 of its row
constexpr int kQuad = 4;                                     // frames per wave per pass
constexpr int kKjStride = 36;                                // complex elements: 32 per (frame, kj) block + 4 (bank spread)
constexpr int kRow = 36;                                     // floats per stash row: 0-26 sums, 27 peak, 28-30 shifts, 31 tie, 32 ex
constexpr int kTw2Bytes = 4 * 8 * 8;                         // pass 2: [a][kc] complex

template <int N>
struct SCfg {
  static_assert(N == 128 || N == 256 || N == 512, "sixteen lanes per frame: 8, 16 or 32 samples a lane");
  static constexpr int kRows = N / 32;                        // rows of 32 samples (16 lanes x 2) per frame
  static constexpr int kLogRows = N == 128 ? 2 : N == 256 ? 3 : 4;
  // passes 2 and 3 take the kRows 32-point transforms of a frame in kHalves batches of kBlocks through the exchange block
  // (N = 512: two batches of eight, so that the block stays at 9.5 KB), a lane kRounds of them per batch
  static constexpr int kHalves = N == 512 ? 2 : 1, kBlocks = kRows / kHalves, kRounds = kBlocks / 4;
  static constexpr int kWavesPerWG = N == 128 ? 16 : 12, kThreads = 64 * kWavesPerWG;
  static constexpr int kBatchPasses = N == 128 ? 8 : 4, kBatch = kQuad * kBatchPasses;   // frames finalised together, one per lane
  // rows requested a pass ahead (the rest at the head of the pass itself: N = 512 has 64 registers of samples)
  static constexpr int kHead = N == 512 ? 4 : kRows;
  // |x| of the sweep for the envelope's second sweep: in registers, or (N = 512) parked in the exchange block
  static constexpr bool kParkA = N == 512;
  static constexpr int kFrameStride = kBlocks * kKjStride + (N == 128 ? 0 : 16);   // the four frames of a pass 128 bytes apart in the banks
  static constexpr int kExBytes = kQuad * kFrameStride * 8;   // 4 608 / 9 728 / 9 728
  static_assert(!kParkA || 2 * kRows * 64 * 4 <= kExBytes, "|x| parking fits the wave's exchange area");
  static constexpr int kStashBytes = kBatch * kRow * 4;       // 4 608 / 2 304
  static constexpr int kTw1Bytes = 16 * (kRows - 1) * 16;     // pass 1: [l][kj - 1] (c0, s0, c1, s1)
  static constexpr int kOffTw1 = kWavesPerWG * (kExBytes + kStashBytes), kOffTw2 = kOffTw1 + kTw1Bytes;
  static constexpr int kLdsBytes = kOffTw2 + kTw2Bytes;       // 148 480 / 146 432
  static_assert(kLdsBytes <= 163840, "one workgroup per CU");
};

// sum / maximum over the 16 lanes of a DPP row, the result in every lane of the row
__device__ __forceinline__ float row_sum(float v) {
  v += dpp<kQuadXor1>(v);
  v += dpp<kQuadXor2>(v);
  v += dpp<kRowHalfMirror>(v);
  v += dpp<kRowMirror>(v);
  return v;
}
__device__ __forceinline__ float row_max(float v) {
  v = __builtin_fmaxf(v, dpp<kQuadXor1>(v));
  v = __builtin_fmaxf(v, dpp<kQuadXor2>(v));
  v = __builtin_fmaxf(v, dpp<kRowHalfMirror>(v));
  v = __builtin_fmaxf(v, dpp<kRowMirror>(v));
  return v;
}

// The statistics sweep of amcx_wave_kernel.h (StatsT) for a frame that lives in one 16-lane row: the right neighbour of
// (j, b = 1) is (j, b = 0) of lane l + 1, or (j + 1, b = 0) of lane 0 for lane 15; the shifts are the means of the row's
// first 16 values.
struct RowLanes {
  static constexpr float kInvLanes = 1.0f / 16.0f;
  static __device__ __forceinline__ float sum_all(float v) { return row_sum(v); }
  static __device__ __forceinline__ float next_lane(float v) { return dpp<kRowRor15>(v); }
  static __device__ __forceinline__ bool is_last(int lane) { return (lane & 15) == 15; }
};
using RowStats = StatsT<RowLanes>;

typedef float v4f __attribute__((ext_vector_type(4)));

// The 18-feature kernel and the feature-subset kernels (amcx_features_c64_subset): PLAN = kPlanNoSpectral or kPlanCumulants,
// columns outside `mask` NaN; the columns the subset kernels keep are bit-identical to amcx_features18_short_kernel<N>'s.
template <int N>
__global__ __launch_bounds__(SCfg<N>::kThreads, SCfg<N>::kWavesPerWG / 4) void amcx_features18_short_kernel(
    const float2* __restrict__ iq, long long n_frames, long long row_stride,
    float* __restrict__ out, long long out_stride) {
  constexpr int PLAN = kPlanAll;
  [[maybe_unused]] constexpr unsigned mask = kMaskAll;
  [[maybe_unused]] constexpr float in_scale = 1.0f;           // (read by the sc16 kernels' loader only)
#include "amcx_short_kernel_body.h"
}

template <int N, int PLAN>
__global__ __launch_bounds__(SCfg<N>::kThreads, SCfg<N>::kWavesPerWG / 4) void amcx_features_subset_short_kernel(
    const float2* __restrict__ iq, long long n_frames, long long row_stride,
    float* __restrict__ out, long long out_stride, unsigned mask) {
  [[maybe_unused]] constexpr float in_scale = 1.0f;
#include "amcx_short_kernel_body.h"
}

}  // namespace shortk
}  // namespace amcx
