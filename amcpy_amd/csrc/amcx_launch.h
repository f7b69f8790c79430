// Host launch layer of libamcx.so: which throughput kernel runs a frame size (THE FRAME-SIZE TABLE, for_frame_size) and how
// every kernel of the library is launched (lds_attr_once, persistent_grid, launch) -- all but the FMA probe's, which times
// thousands of launches back to back and asks once at the end (amcx_probe.h).  Host code only: the kernels, their Cfg / SCfg / G
// constants and their documentation live in the kernel headers, which the diagnostic tools include on their own.
#pragma once

#include <stdio.h>
#include <stdlib.h>
#include <atomic>
#include <tuple>
#include <type_traits>

#include "amcx_wave_kernel.h"
#include "amcx_quad_kernel.h"
#include "amcx_group_kernel.h"
#include "amcx_short_kernel.h"
#include "amcx_sc16_kernels.h"

namespace amcx {

constexpr int kMaxDevices = 64;

// DYNAMIC LDS, ONCE.  More than 64 KiB of dynamic LDS needs hipFuncAttributeMaxDynamicSharedMemorySize.  The attribute is
// per device, and it is set once per (kernel, device) to `most`, the most that kernel ever asks for, never per launch: two
// host threads launching different N would otherwise race between one's attribute and the other's launch.  Several host
// threads do launch at once (DeviceFanOut); two that meet here for the first time both set the same value, and the flag is
// an atomic.  No lock, no allocation, no lookup: the flags are this instantiation's own.  (A device index beyond the flags
// sets the attribute on every launch.)
template <auto Kern>
inline hipError_t lds_attr_once(int most) {
  static std::atomic<bool> set[kMaxDevices];
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const bool known = dev >= 0 && dev < kMaxDevices;
  if (known && set[dev].load(std::memory_order_relaxed)) return hipSuccess;
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, most);
  if (e == hipSuccess && known) set[dev].store(true, std::memory_order_relaxed);
  return e;
}

// Workgroups of a persistent launch: wgs_per_cu resident workgroups on every CU, or as many as the work has units for.
inline int64_t persistent_grid(int cus, int wgs_per_cu, int64_t work, int64_t unit) {
  const int64_t full = (int64_t)cus * wgs_per_cu, need = (work + unit - 1) / unit;
  const int64_t grid = full < need ? full : need;
  return grid < 1 ? 1 : grid;
}

// Launch, then ask.  `kern` is a plain pointer: where a kernel name is overloaded the caller has chosen already.
// `grid`: a dim3 for the few two-dimensional grids, a count of workgroups for everything else.
template <class... P, class... A>
inline hipError_t launch(void (*kern)(P...), dim3 grid, int threads, size_t lds, hipStream_t stream, A... args) {
  static_assert(sizeof...(P) == sizeof...(A), "one argument per kernel parameter");
  hipLaunchKernelGGL(kern, grid, dim3((unsigned)threads), lds, stream, static_cast<P>(args)...);
  return hipGetLastError();
}
template <class... P, class... A>
inline hipError_t launch(void (*kern)(P...), int64_t grid, int threads, size_t lds, hipStream_t stream, A... args) {
  return launch(kern, dim3((unsigned)grid), threads, lds, stream, args...);
}

// what every feature kernel is launched over
struct Frames {
  const float2* iq;
  int64_t n_frames, row_stride;
  float* out;
  int64_t out_stride;
  hipStream_t stream;
  int cus;
  // sc16 frames (include/amcx.h, amcx_features_sc16): read through iq16 instead of iq, a sample's components times `scale`
  const wave::sc16* iq16 = nullptr;
  float scale = 1.0f;
};
template <class... Tail>
using FeatureKernel = void (*)(const float2*, long long, long long, float*, long long, Tail...);
// the sc16 kernels: the scale stands behind the five common arguments
template <class... Tail>
using Sc16Kernel = void (*)(const wave::sc16*, long long, long long, float*, long long, float, Tail...);

template <class... Tail>
inline hipError_t launch_frames(FeatureKernel<Tail...> kern, int64_t grid, int threads, int lds, const Frames& a, Tail... tail) {
  return launch(kern, grid, threads, (size_t)lds, a.stream, a.iq, a.n_frames, a.row_stride, a.out, a.out_stride, tail...);
}
template <class... Tail>
inline hipError_t launch_frames(Sc16Kernel<Tail...> kern, int64_t grid, int threads, int lds, const Frames& a, Tail... tail) {
  return launch(kern, grid, threads, (size_t)lds, a.stream, a.iq16, a.n_frames, a.row_stride, a.out, a.out_stride, a.scale,
                tail...);
}

// ---- the kernel families -----------------------------------------------------------------------------------------------
// One struct per family, what THE FRAME-SIZE TABLE hands out: the kernel's name (kStem, and kNameArg in angle brackets
// where it is not 0), kPlanStem where the family has feature-plan kernels (amcx_features_c64_subset) and nullptr where the
// 18-feature kernel and a column mask serve, the bytes of ring a launch over `cus` CUs takes, and launch<PLAN>().
// kSc16Stem / kSc16PlanStem: the family's kernels over sc16 frames, which launch<PLAN, wave::sc16>() runs (nullptr: none --
// amcx_features_sc16 widens into its workspace and runs the complex64 kernel).
// `ring`: ring_bytes(cus) bytes that no other launch in flight uses, or nullptr.  `mask`: read by the plan kernels only.
struct SizeDefaults {                            // no plan kernels, no ring, no template argument in the name
  static constexpr const char* kPlanStem = nullptr;
  static constexpr const char* kSc16Stem = nullptr;
  static constexpr const char* kSc16PlanStem = nullptr;
  static constexpr int kNameArg = 0;
  static constexpr size_t ring_bytes(int) { return 0; }
};

// 128, 256, 512: four frames per wave (amcx_short_kernel.h)
template <int N>
struct ShortSize : SizeDefaults {
  static constexpr const char* kStem = "amcx_features18_short_kernel";
  static constexpr const char* kPlanStem = "amcx_features_subset_short_kernel";
  static constexpr const char* kSc16Stem = "amcx_features18_short_sc16_kernel";
  static constexpr const char* kSc16PlanStem = "amcx_features_subset_short_sc16_kernel";
  static constexpr int kNameArg = N;

  template <int PLAN, class E = float2>
  static hipError_t launch(const Frames& a, float*, unsigned mask) {
    using C = shortk::SCfg<N>;
    const int64_t n_pass = (a.n_frames + shortk::kQuad - 1) / shortk::kQuad;
    const int64_t grid = persistent_grid(a.cus, 1, n_pass, C::kWavesPerWG);      // one resident workgroup per CU
    if constexpr (std::is_same_v<E, wave::sc16>) {
      if constexpr (PLAN == kPlanAll) {
        constexpr Sc16Kernel<> kern = shortk::amcx_features18_short_sc16_kernel<N>;
        if (const hipError_t e = lds_attr_once<kern>(C::kLdsBytes); e != hipSuccess) return e;
        return launch_frames(kern, grid, C::kThreads, C::kLdsBytes, a);
      } else {
        constexpr Sc16Kernel<unsigned> kern = shortk::amcx_features_subset_short_sc16_kernel<N, PLAN>;
        if (const hipError_t e = lds_attr_once<kern>(C::kLdsBytes); e != hipSuccess) return e;
        return launch_frames(kern, grid, C::kThreads, C::kLdsBytes, a, mask);
      }
    } else if constexpr (PLAN == kPlanAll) {
      constexpr FeatureKernel<> kern = shortk::amcx_features18_short_kernel<N>;
      if (const hipError_t e = lds_attr_once<kern>(C::kLdsBytes); e != hipSuccess) return e;
      return launch_frames(kern, grid, C::kThreads, C::kLdsBytes, a);
    } else {
      constexpr FeatureKernel<unsigned> kern = shortk::amcx_features_subset_short_kernel<N, PLAN>;
      if (const hipError_t e = lds_attr_once<kern>(C::kLdsBytes); e != hipSuccess) return e;
      return launch_frames(kern, grid, C::kThreads, C::kLdsBytes, a, mask);
    }
  }
};

// 1024, 2048, 4096: one wave per frame (amcx_wave_kernel.h)
template <int N>
struct WaveSize : SizeDefaults {
  using C = wave::Cfg<N>;
  static constexpr const char* kStem = "amcx_features18_wave_kernel";
  static constexpr const char* kPlanStem = "amcx_features_subset_wave_kernel";
  static constexpr const char* kSc16Stem = "amcx_features18_wave_sc16_kernel";
  static constexpr const char* kSc16PlanStem = "amcx_features_subset_wave_sc16_kernel";
  static constexpr int kNameArg = N;
  static constexpr size_t ring_bytes(int cus) {
    return C::kHasRing ? (size_t)cus * C::kWavesPerWG * C::kRingFloatsPerWave * sizeof(float) : 0;
  }

  // the size's product kernel -- of the two overloads the one with a ring where the size takes one (the pointer's type
  // chooses) -- or, LDS_FORM, the same body without a ring
  template <int PLAN, bool LDS_FORM, class... Tail>
  static constexpr FeatureKernel<Tail...> kernel() {
    if constexpr (LDS_FORM) {
      if constexpr (PLAN == kPlanAll) return wave::amcx_features18_wave_lds_kernel<N>;
      else return wave::amcx_features_subset_wave_lds_kernel<N, PLAN>;
    } else {
      if constexpr (PLAN == kPlanAll) return wave::amcx_features18_wave_kernel<N>;
      else return wave::amcx_features_subset_wave_kernel<N, PLAN>;
    }
  }

  // ... and its form over sc16 frames
  template <int PLAN, bool LDS_FORM, class... Tail>
  static constexpr Sc16Kernel<Tail...> kernel_sc16() {
    if constexpr (LDS_FORM) {
      if constexpr (PLAN == kPlanAll) return wave::amcx_features18_wave_sc16_lds_kernel<N>;
      else return wave::amcx_features_subset_wave_sc16_lds_kernel<N, PLAN>;
    } else {
      if constexpr (PLAN == kPlanAll) return wave::amcx_features18_wave_sc16_kernel<N>;
      else return wave::amcx_features_subset_wave_sc16_kernel<N, PLAN>;
    }
  }

  // A launch that has no ring runs the LDS form of a size whose kernel takes one (amcx_features18_wave_lds_kernel): same results.
  template <int PLAN, class E = float2>
  static hipError_t launch(const Frames& a, float* ring, unsigned mask) {
    // persistent: one resident workgroup per CU; at least a frame per wave
    const int64_t grid = persistent_grid(a.cus, 1, a.n_frames, C::kWavesPerWG);
    auto run = [&](auto lds_form, auto tail) {
      return std::apply([&](auto... t) {
        constexpr auto kern = [] {
          if constexpr (std::is_same_v<E, wave::sc16>) return kernel_sc16<PLAN, decltype(lds_form)::value, decltype(t)...>();
          else return kernel<PLAN, decltype(lds_form)::value, decltype(t)...>();
        }();
        if (const hipError_t e = lds_attr_once<kern>(C::kLdsBytes); e != hipSuccess) return e;
        return launch_frames(kern, grid, C::kThreads, C::kLdsBytes, a, t...);
      }, tail);
    };
    // the kernel's trailing arguments: `mask` for a plan kernel, then `ring` for the ring form
    const auto plan_args = [&] {
      if constexpr (PLAN == kPlanAll) return std::tuple<>{};
      else return std::make_tuple(mask);
    }();
    if constexpr (C::kHasRing) {
      if (ring != nullptr) return run(std::false_type{}, std::tuple_cat(plan_args, std::make_tuple(ring)));
    }
    return run(std::bool_constant<C::kHasRing>{}, plan_args);
  }
};

// 8192: four waves per frame (amcx_quad_kernel.h)
struct QuadSize : SizeDefaults {
  static constexpr const char* kStem = "amcx_features18_quad_kernel";

  template <int PLAN>
  static hipError_t launch(const Frames& a, float*, unsigned) {
    static_assert(PLAN == kPlanAll, "no plan kernels at this size");
    using namespace quad;
    static_assert(kLdsBytes <= 65536, "more needs lds_attr_once");
    // a workgroup's re-run mask covers kMaskFrames frames of its own run: longer inputs (more than 8.4 M frames of
    // 64 KiB at 512 workgroups -- beyond one device's memory unless rows overlap) go as several launches
    int64_t per_launch = (int64_t)a.cus * kWGsPerCU * kMaskFrames;
    // tests only: cut at this many frames (any cut is valid; the real one needs more frames than a device holds).  Read ONCE
    // per process (a function-local static: getenv on every launch raced with setenv / putenv from other threads --
    // Python writes os.environ while DeviceFanOut's threads launch with the GIL released)
    static const long long test_split = [] { const char* t = getenv("AMCX_TEST_QUAD_SPLIT"); return t ? atoll(t) : 0LL; }();
    if (test_split >= kBatch && test_split < per_launch) per_launch = test_split / kBatch * kBatch;
    for (int64_t f0 = 0; f0 < a.n_frames; f0 += per_launch) {
      Frames part = a;
      part.iq += f0 * a.row_stride;
      part.out += f0 * a.out_stride;
      part.n_frames = a.n_frames - f0 < per_launch ? a.n_frames - f0 : per_launch;
      const int64_t grid = persistent_grid(a.cus, kWGsPerCU, part.n_frames, kBatch);   // two resident workgroups per CU
      const hipError_t e = launch_frames<>(amcx_features18_quad_kernel, grid, kThreads, kLdsBytes, part);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
};

// 16384, 32768: W = 8 / 16 waves per frame (amcx_group_kernel.h)
template <int W>
struct GroupSize : SizeDefaults {
  static constexpr const char* kStem = "amcx_features18_group_kernel";
  static constexpr int kNameArg = W;

  template <int PLAN>
  static hipError_t launch(const Frames& a, float*, unsigned) {
    static_assert(PLAN == kPlanAll, "no plan kernels at this size");
    using Cg = group::G<W>;
    constexpr FeatureKernel<> kern = group::amcx_features18_group_kernel<W>;
    if (const hipError_t e = lds_attr_once<kern>(Cg::kLdsBytes); e != hipSuccess) return e;
    const int64_t grid = persistent_grid(a.cus, 1, a.n_frames, Cg::kBatch);       // one resident workgroup per CU
    return launch_frames(kern, grid, Cg::kThreads, Cg::kLdsBytes, a);
  }
};

// every other size: no throughput kernel (AMCX_VARIANT_BLOCK runs it)
struct NoSize : SizeDefaults {
  static constexpr const char* kStem = "";
  template <int PLAN>
  static hipError_t launch(const Frames&, float*, unsigned) { return hipErrorNotSupported; }
};

// THE FRAME-SIZE TABLE: the throughput kernel (AMCX_VARIANT_WAVE) of a run-time frame size, handed to `f` as one of the
// structs above.  Everything the host knows about a size follows from here; a new size, or a ring for one that has none
// (Cfg<N>::kHasRing), is its kernel header and a line of this switch.
// (128, 256 and 512 ran the one-wave-per-frame kernel until late in round 5 -- 8 / 4 / 2 frames sharing one run of FFT
//  passes 2-3 -- and have a kernel of their own now, amcx_short_kernel.h: +34 % / +13 % / +2.5 ... 5 %)
template <class F>
inline auto for_frame_size(int frame_size, F&& f) {
  switch (frame_size) {
    case 128: return f(ShortSize<128>{});
    case 256: return f(ShortSize<256>{});
    case 512: return f(ShortSize<512>{});
    case 1024: return f(WaveSize<1024>{});
    case 2048: return f(WaveSize<2048>{});
    case 4096: return f(WaveSize<4096>{});
    case quad::kN: return f(QuadSize{});
    case group::G<8>::kN: return f(GroupSize<8>{});
    case group::G<16>::kN: return f(GroupSize<16>{});
    default: return f(NoSize{});
  }
}

inline bool wave_supports(int frame_size) {
  return for_frame_size(frame_size, [](auto size) { return !std::is_same_v<decltype(size), NoSize>; });
}
inline bool has_plan_kernels(int frame_size) {
  return for_frame_size(frame_size, [](auto size) { return decltype(size)::kPlanStem != nullptr; });
}
inline bool has_sc16_kernels(int frame_size) {
  return for_frame_size(frame_size, [](auto size) { return decltype(size)::kSc16Stem != nullptr; });
}
// bytes of ring a launch of this frame size over `cus` workgroups needs (0: that size's kernel takes none)
inline size_t wave_ring_bytes(int frame_size, int cus) {
  return for_frame_size(frame_size, [&](auto size) { return decltype(size)::ring_bytes(cus); });
}
// "stem<arg>" of the 18-feature kernel, or "stem<arg, plan>" of a plan kernel
// (sc16: of the size's sc16 kernels where it has them -- has_sc16_kernels -- and of the complex64 kernel otherwise)
inline void wave_kernel_name(int frame_size, int plan, char* buf, size_t len, bool sc16 = false) {
  for_frame_size(frame_size, [&](auto size) {
    using S = decltype(size);
    const bool typed = sc16 && S::kSc16Stem != nullptr;
    if constexpr (S::kPlanStem != nullptr) {
      if (plan != kPlanAll) return snprintf(buf, len, "%s<%d, %d>", typed ? S::kSc16PlanStem : S::kPlanStem, S::kNameArg, plan);
    }
    if constexpr (S::kNameArg != 0) return snprintf(buf, len, "%s<%d>", typed ? S::kSc16Stem : S::kStem, S::kNameArg);
    else return snprintf(buf, len, "%s", S::kStem);
  });
}

// KERNEL ORDER.  hipcc lays kernels out in .text in the order in which the host code first names them, and a kernel that
// calls a function the compiler did not inline (the group kernels: group_finalise; the stream kernels: finalise_frame) holds
// the distance to it in its bytes.  The committed counter profiles are bound to every kernel's bytes (tools/codeobj_gate.py
// --kernels, bench.py), so the order of before is kept where those distances depend on it: the 18-feature kernels of the
// sizes that have plan kernels come first, as when their launchers stood in the kernel headers; amcx.hip names the stream
// and block kernels next, and the dispatch of its entry (run_features) everything else.  Nothing calls this.
// The sc16 kernels (ABI 9) stand in FRONT of all of them, as explicit specialisations in a header amcx.hip includes first
// (amcx_sc16_kernels.h says why): code added behind the first existing kernel would move distances that existing kernels hold.
// The 8-bit widening kernels (ABI 10, amcx_iq8_kernels.h) are plain kernels in a header included in front of that one: the head of the head.
// The down-converter's kernels (ABI 11, amcx_ddc_kernel.h) stand in front of those, and the filter bank's (ABI 12, amcx_bank_kernel.h:
// it includes the down-converter's header, whose loaders and mixer it uses, in front of its own kernels) are included first of all.
// The resampler's (ABI 13, amcx_resample_kernel.h, which includes the down-converter's in the same way) came in front of the bank's, and the
// occupancy kernels (ABI 14, amcx_occupancy_kernels.h: plain kernels that call nothing of the others) in front of everything.
// The spectrogram's (ABI 15, amcx_psd_kernel.h, which includes the occupancy and down-converter headers for occ_key and the
// loaders) are included in front of those.
// The fixed-point kernels (ABI 16, amcx_mlp_q15_kernel.h) come first of all now: plain kernels on amcx_mlp_shape.h, which holds the
// declarations and the device routines (staging, row load, sums, votes, the scaler's roundings) they share with the classifier and
// no kernel, so including it there moves nothing.
// The training kernels (ABI 16.1, amcx_mlp_train_kernel.h, on amcx_mlp_shape.h alone) are included in front of those: one plain kernel and
// six explicit specialisations (an explicit INSTANTIATION is laid out behind the device functions in the middle of .text and moved the group
// and stream kernels' distances; a specialisation is laid out where it stands, as the sc16 kernels are).
// The waveform generator's kernel (ABI 16.2, amcx_synth_kernel.h) is a plain kernel in the header included in front of that one; it includes
// the training kernels' header (for philox4x32_10) and the down-converter's (for the mixer) in front of its own kernel, so it is laid out
// behind the training kernels and in front of the fixed-point ones, and every older kernel keeps its bytes.
// The fading channel's kernel (ABI 16.2.1, amcx_channel_kernel.h) is a plain kernel in the header included in front of that one; it includes the
// generator's header (for syn_finish, and with it Philox, the mixer and the staging routine) in front of its own kernel, so it is laid out behind the
// generator's and in front of the fixed-point ones; calling syn_finish (inlined) from a second kernel left the generator's bytes what they were.
// The continuous-phase generator's kernel (ABI 16.2.2, amcx_synth_cpm_kernel.h) is a plain kernel in the header included in front of that one; it
// includes the generator's header (for syn_finish, Philox, the mixer and the plan) in front of its own kernel and templates nothing that is shared.
// The carrier-recovery kernel (ABI 16.2.3, amcx_carrier_kernel.h) is a plain kernel in the header included in front of that one; it includes the
// spectrogram's header (for psd_pass, psd_pad, psd_mul, and the mixer through it) in front of its own kernel and templates nothing that is shared.
// amcx_polyphase.h (the tap image, the sum and the plan arithmetic the generator and the resampler share) holds NO kernel, as amcx_mlp_shape.h: nothing moves.
// Nor does amcx_exact_passes.h (what the block and the stream kernel share; the wave kernels' header includes it for wave_sum).
// That specialisations are laid out there is what hipcc does today, not a rule it documents: tools/codeobj_gate.py --kernels
// against the parent commit is what guards it, and the only thing that will notice when a compiler lays them out elsewhere.
inline void kernel_order_anchor() {
  for_frame_size(0, [](auto size) {
    using S = decltype(size);
    if constexpr (S::kPlanStem != nullptr) (void)&S::template launch<kPlanAll>;
    return 0;
  });
}

}  // namespace amcx
