// The kernels over sc16 frames (include/amcx.h, amcx_features_sc16; ABI 9): the wave kernels (N = 1024, 2048, 4096) and the
// short kernels (N = 128, 256, 512), 18-feature and both feature plans, with a frame's element type sc16 and the scale as an
// argument (amcx_wave_kernel.h, THE SAMPLE LOADER) -- the same bodies as the complex64 kernels, so their rows equal those
// kernels' on the widened frame bit for bit -- and the kernel that widens sc16 rows to complex64 for every frame size and
// variant that has none.  Names of their own, so that a kernel trace tells them apart.
//
// WHY EXPLICIT SPECIALISATIONS, AND WHY amcx.hip INCLUDES THIS HEADER FIRST.  hipcc lays plain kernels out in .text in the
// order of their definitions, in front of every instantiation of a kernel template.  The stream and group kernels call
// functions the compiler did not inline, and the group kernels' finalisers address a table that the linker places behind
// .text: their bytes hold those distances, and a kernel added anywhere behind the first of them moves one of them (as
// instantiations of kernel templates, these kernels changed the bytes of group_finalise; a plain kernel beside
// amcx_c128_to_c64_kernel changed the stream and group kernels).  An explicit specialisation is a plain function: defined
// here, ahead of every other kernel of the library, these stand at the head of .text, and everything that was there before
// keeps its distance to everything else -- tools/codeobj_gate.py --kernels, profiles/r10_sc16_codeobj_kernels.txt.
// (Since ABI 10 amcx_iq8_kernels.h is included in front of this header, for the same reason: its two kernels shift these and
//  everything behind them by the same amount.)
#pragma once

#include "amcx_short_kernel.h"

namespace amcx {

// sc16 -> complex64, row-packed: dst[f][n] = ((float)I * scale, (float)Q * scale), n < N -- the frame the sc16 kernels compute
// on, as amcx_c128_to_c64_kernel (amcx_pack_kernel.h) rounds complex128 rows
__global__ __launch_bounds__(256) void amcx_sc16_to_c64_kernel(const short2* __restrict__ src,
                                                              long long n_frames, int N,
                                                              long long src_stride, float scale, float2* __restrict__ dst) {
  const long long total = n_frames * N;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long f = i / N;
    const int n = (int)(i - f * N);
    const short2 v = src[f * src_stride + n];
    dst[i] = make_float2((float)v.x * scale, (float)v.y * scale);
  }
}

#define AMCX_SC16_PARAMS                                                                                        \
  const sc16* __restrict__ iq, long long n_frames, long long row_stride, float* __restrict__ out, long long out_stride, \
      float in_scale

namespace shortk {

// amcx_short_kernel_body.h once more (as a function: only the complex64 kernels are held to the bytes they had)
template <int N, int PLAN>
__device__ __forceinline__ void short_sc16_body(AMCX_SC16_PARAMS, [[maybe_unused]] unsigned mask) {
#include "amcx_short_kernel_body.h"
}

template <int N>
__global__ void amcx_features18_short_sc16_kernel(AMCX_SC16_PARAMS);
template <int N, int PLAN>
__global__ void amcx_features_subset_short_sc16_kernel(AMCX_SC16_PARAMS, unsigned mask);

#define AMCX_SC16_SHORT_BOUNDS(N) __launch_bounds__(SCfg<N>::kThreads, SCfg<N>::kWavesPerWG / 4)
#define AMCX_SC16_SHORT(N)                                                                                      \
  template <>                                                                                                   \
  __global__ AMCX_SC16_SHORT_BOUNDS(N) void amcx_features18_short_sc16_kernel<N>(AMCX_SC16_PARAMS) {             \
    short_sc16_body<N, kPlanAll>(iq, n_frames, row_stride, out, out_stride, in_scale, kMaskAll);                \
  }
#define AMCX_SC16_SHORT_PLAN(N, PLAN)                                                                           \
  template <>                                                                                                   \
  __global__ AMCX_SC16_SHORT_BOUNDS(N) void amcx_features_subset_short_sc16_kernel<N, PLAN>(AMCX_SC16_PARAMS,    \
                                                                                            unsigned mask) {    \
    short_sc16_body<N, PLAN>(iq, n_frames, row_stride, out, out_stride, in_scale, mask);                        \
  }
AMCX_SC16_SHORT(128)
AMCX_SC16_SHORT(256)
AMCX_SC16_SHORT(512)
AMCX_SC16_SHORT_PLAN(128, kPlanCumulants)
AMCX_SC16_SHORT_PLAN(256, kPlanCumulants)
AMCX_SC16_SHORT_PLAN(512, kPlanCumulants)
AMCX_SC16_SHORT_PLAN(128, kPlanNoSpectral)
AMCX_SC16_SHORT_PLAN(256, kPlanNoSpectral)
AMCX_SC16_SHORT_PLAN(512, kPlanNoSpectral)
#undef AMCX_SC16_SHORT
#undef AMCX_SC16_SHORT_PLAN
#undef AMCX_SC16_SHORT_BOUNDS

}  // namespace shortk

namespace wave {

// As the complex64 kernels (amcx_wave_kernel.h): where the size takes a ring (Cfg<N>::kHasRing) the kernel has a trailing
// `ring` argument, and its LDS form -- for a launch that has no ring -- is the _lds kernel.
template <int N>
__global__ void amcx_features18_wave_sc16_kernel(AMCX_SC16_PARAMS);
template <int N>
__global__ void amcx_features18_wave_sc16_kernel(AMCX_SC16_PARAMS, float* ring);
template <int N>
__global__ void amcx_features18_wave_sc16_lds_kernel(AMCX_SC16_PARAMS);
template <int N, int PLAN>
__global__ void amcx_features_subset_wave_sc16_kernel(AMCX_SC16_PARAMS, unsigned mask);
template <int N, int PLAN>
__global__ void amcx_features_subset_wave_sc16_kernel(AMCX_SC16_PARAMS, unsigned mask, float* ring);
template <int N, int PLAN>
__global__ void amcx_features_subset_wave_sc16_lds_kernel(AMCX_SC16_PARAMS, unsigned mask);

#define AMCX_SC16_WAVE_BOUNDS(N) __launch_bounds__(Cfg<N>::kThreads, (Cfg<N>::kWavesPerWG + 3) / 4)
// a size without a ring: the 18-feature kernel and the two plans
#define AMCX_SC16_WAVE(N, PLAN)                                                                                          \
  template <>                                                                                                            \
  __global__ AMCX_SC16_WAVE_BOUNDS(N) void amcx_features_subset_wave_sc16_kernel<N, PLAN>(AMCX_SC16_PARAMS, unsigned mask) { \
    static_assert(!Cfg<N>::kHasRing, "this size takes a ring");                                                           \
    wave_body<N, PLAN, false, sc16>(iq, n_frames, row_stride, out, out_stride, mask, nullptr, in_scale);                 \
  }
#define AMCX_SC16_WAVE_ALL(N)                                                                                            \
  template <>                                                                                                            \
  __global__ AMCX_SC16_WAVE_BOUNDS(N) void amcx_features18_wave_sc16_kernel<N>(AMCX_SC16_PARAMS) {                        \
    static_assert(!Cfg<N>::kHasRing, "this size takes a ring");                                                           \
    wave_body<N, kPlanAll, false, sc16>(iq, n_frames, row_stride, out, out_stride, kMaskAll, nullptr, in_scale);         \
  }
// a size with a ring: the ring form and the LDS form of each
#define AMCX_SC16_WAVE_RING(N, PLAN)                                                                                     \
  template <>                                                                                                            \
  __global__ AMCX_SC16_WAVE_BOUNDS(N) void amcx_features_subset_wave_sc16_kernel<N, PLAN>(AMCX_SC16_PARAMS, unsigned mask, \
                                                                                          float* ring) {                 \
    static_assert(Cfg<N>::kHasRing, "no ring form at this frame size");                                                   \
    wave_body<N, PLAN, true, sc16>(iq, n_frames, row_stride, out, out_stride, mask, ring, in_scale);                     \
  }                                                                                                                      \
  template <>                                                                                                            \
  __global__ AMCX_SC16_WAVE_BOUNDS(N) void amcx_features_subset_wave_sc16_lds_kernel<N, PLAN>(AMCX_SC16_PARAMS,           \
                                                                                              unsigned mask) {           \
    wave_body<N, PLAN, false, sc16>(iq, n_frames, row_stride, out, out_stride, mask, nullptr, in_scale);                 \
  }
#define AMCX_SC16_WAVE_RING_ALL(N)                                                                                       \
  template <>                                                                                                            \
  __global__ AMCX_SC16_WAVE_BOUNDS(N) void amcx_features18_wave_sc16_kernel<N>(AMCX_SC16_PARAMS, float* ring) {           \
    static_assert(Cfg<N>::kHasRing, "no ring form at this frame size");                                                   \
    wave_body<N, kPlanAll, true, sc16>(iq, n_frames, row_stride, out, out_stride, kMaskAll, ring, in_scale);             \
  }                                                                                                                      \
  template <>                                                                                                            \
  __global__ AMCX_SC16_WAVE_BOUNDS(N) void amcx_features18_wave_sc16_lds_kernel<N>(AMCX_SC16_PARAMS) {                    \
    wave_body<N, kPlanAll, false, sc16>(iq, n_frames, row_stride, out, out_stride, kMaskAll, nullptr, in_scale);         \
  }
#ifndef AMCX_WAVE_STAMPS
AMCX_SC16_WAVE_ALL(1024)
AMCX_SC16_WAVE_RING_ALL(2048)
AMCX_SC16_WAVE_ALL(4096)
AMCX_SC16_WAVE(1024, kPlanCumulants)
AMCX_SC16_WAVE_RING(2048, kPlanCumulants)
AMCX_SC16_WAVE(4096, kPlanCumulants)
AMCX_SC16_WAVE(1024, kPlanNoSpectral)
AMCX_SC16_WAVE_RING(2048, kPlanNoSpectral)
AMCX_SC16_WAVE(4096, kPlanNoSpectral)
#endif
#undef AMCX_SC16_WAVE
#undef AMCX_SC16_WAVE_ALL
#undef AMCX_SC16_WAVE_RING
#undef AMCX_SC16_WAVE_RING_ALL
#undef AMCX_SC16_WAVE_BOUNDS

}  // namespace wave

#undef AMCX_SC16_PARAMS

}  // namespace amcx
