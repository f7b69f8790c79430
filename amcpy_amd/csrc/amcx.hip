// libamcx.so -- C ABI (include/amcx.h) over the gfx950 feature kernels.
// Build: hipcc --offload-arch=gfx950 -O3 -fPIC -shared (see build.py).
// This file: the feature dispatch (run_features and the launchers amcx_launch.h does not hold), the post-processing and
// classifier entries, and extern "C".  The contexts and their upload engine: amcx_ctx.h; the probes: amcx_probe.h.
#include "../../include/amcx.h"

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <initializer_list>
#include <mutex>
#include <new>
#include <vector>

#include "amcx_carrier_kernel.h"   // FIRST of all (ABI 16.2.3: it includes the spectrogram's header in front of its one kernel), then the continuous-phase generator's ...
#include "amcx_synth_cpm_kernel.h" // ... (ABI 16.2.2: it includes the generator's header in front of its one kernel), then the channel's ...
#include "amcx_channel_kernel.h"   // ... (ABI 16.2.1: it includes the generator's header in front of its one kernel), then the generator's ...
#include "amcx_synth_kernel.h"     // ... (ABI 16.2: it includes the training kernels' header and the down-converter's in front of its one kernel), ...
#include "amcx_mlp_train_kernel.h" // ... (ABI 16.1: plain and explicitly instantiated kernels on amcx_mlp_shape.h alone), then the fixed-point ones ...
#include "amcx_mlp_q15_kernel.h"   // ... (ABI 16: plain kernels on amcx_mlp_shape.h alone, which holds no kernel), then the spectrogram's ...
#include "amcx_psd_kernel.h"       // ... it includes the occupancy and down-converter headers for their device helpers), ...
#include "amcx_occupancy_kernels.h"  // ... then the occupancy kernels (ABI 14: plain kernels that call nothing of the others), ...
#include "amcx_resample_kernel.h"  // ... then the resampler's (it includes the down-converter's header in front of its own kernels), the bank's next, ...
#include "amcx_bank_kernel.h"
#include "amcx_ddc_kernel.h"       // ... then the 8-bit widening kernels, then the sc16 kernels: KERNEL ORDER, amcx_launch.h
#include "amcx_iq8_kernels.h"
#include "amcx_sc16_kernels.h"
#include "amcx_block_kernel.h"
#include "amcx_stream_kernel.h"
#include "amcx_launch.h"
#include "amcx_post_kernels.h"
#include "amcx_mlp_kernel.h"
#include "amcx_pack_kernel.h"
#include "amcx_upload.h"

namespace {

thread_local char g_hip_err[256] = "";

int hip_fail(hipError_t e, const char* what) {
  snprintf(g_hip_err, sizeof g_hip_err, "%s: %s", what, hipGetErrorString(e));
  return AMCX_EHIP;
}

#define AMCX_HIP(call)                                     \
  do {                                                     \
    hipError_t e_ = (call);                                \
    if (e_ != hipSuccess) return hip_fail(e_, #call);      \
  } while (0)

bool is_pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }

int resolve_variant(int32_t frame_size, int32_t variant) {
  if (frame_size < AMCX_MIN_FRAME_SIZE || frame_size > AMCX_MAX_FRAME_SIZE) return AMCX_EINVAL;
  const bool block_ok = frame_size <= AMCX_MAX_BLOCK_FRAME_SIZE;      // every size in range since ABI 6
  switch (variant) {
    case AMCX_VARIANT_AUTO:
      return amcx::wave_supports(frame_size) ? AMCX_VARIANT_WAVE : block_ok ? AMCX_VARIANT_BLOCK : AMCX_ENOTSUP;
    case AMCX_VARIANT_BLOCK:
      return block_ok ? AMCX_VARIANT_BLOCK : AMCX_ENOTSUP;
    case AMCX_VARIANT_WAVE:
      return amcx::wave_supports(frame_size) ? AMCX_VARIANT_WAVE : AMCX_ENOTSUP;
    default:
      return AMCX_EINVAL;
  }
}

// CUs of the calling thread's current device (cached per device: a node may mix partitioned and whole GPUs)
int cu_count() {
  static std::atomic<int> cus[amcx::kMaxDevices];   // every writer of a slot stores the same value
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 256; }
  const bool known = dev >= 0 && dev < amcx::kMaxDevices;
  if (known && (n = cus[dev].load(std::memory_order_relaxed)) > 0) return n;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    return 256;
  }
  if (known) cus[dev].store(n, std::memory_order_relaxed);
  return n;
}

// ---- rings of stash rows (amcx_wave_kernel.h, wave_body RING) ---------------------------------------
// A launch of a wave kernel that finalises 64 frames per wave at a time parks its stash rows in a ring in global memory
// (amcx::wave_ring_bytes).  Two launches that may overlap must never share one.  A context owns its ring (amcx_ctx::d_ring:
// its launches all go to its own stream).  The context-free entries take theirs from this pool, keyed by (device, stream):
// launches on one stream run one after the other.  A ring is allocated on the first call of a stream and kept; finding it
// later is a short list under a mutex.  No ring -- nullptr, and the launch runs the kernel's LDS form, same results -- for
//   * a stream that is being captured: the graph may be replayed on any stream, beside an eager launch on this one;
//   * hipStreamPerThread: one handle, a different stream in every thread;
//   * a full pool or a failed allocation;
//   * a process started with AMCX_WAVE_RING=0.
struct RingSource {
  float* own = nullptr;     // the caller's ring (a context's), of own_bytes
  size_t own_bytes = 0;
  bool pool = false;        // none of its own: take one from the pool
};
struct PoolRing { int device; hipStream_t stream; void* p; size_t bytes; };
std::mutex g_ring_mu;
std::vector<PoolRing> g_rings;
constexpr size_t kPoolRingsPerDevice = 16;

float* pool_ring(hipStream_t stream, size_t bytes) {
  if (stream == hipStreamPerThread) return nullptr;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cap) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  if (cap != hipStreamCaptureStatusNone) return nullptr;
  std::lock_guard<std::mutex> lock(g_ring_mu);
  size_t on_dev = 0;
  for (PoolRing& r : g_rings) {
    if (r.device != dev) continue;
    ++on_dev;
    if (r.stream != stream) continue;
    if (r.bytes >= bytes) return static_cast<float*>(r.p);
    (void)hipFree(r.p);                        // (waits for the device: nothing still runs on the old one)
    r.p = nullptr; r.bytes = 0;
    if (hipMalloc(&r.p, bytes) != hipSuccess) { (void)hipGetLastError(); r.p = nullptr; return nullptr; }
    r.bytes = bytes;
    return static_cast<float*>(r.p);
  }
  if (on_dev >= kPoolRingsPerDevice) return nullptr;
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  g_rings.push_back(PoolRing{dev, stream, p, bytes});
  return static_cast<float*>(p);
}

// the ring for one launch of frame size N on `stream`, or nullptr
float* ring_for(const RingSource& rs, int32_t N, hipStream_t stream) {
  // AMCX_WAVE_RING=0 (read once per process): no rings, every launch runs the LDS form -- for tests and A/B runs
  static const bool off = [] { const char* t = getenv("AMCX_WAVE_RING"); return t != nullptr && t[0] == '0'; }();
  if (off) return nullptr;
  const size_t need = amcx::wave_ring_bytes(N, cu_count());
  if (need == 0) return nullptr;
  if (rs.own != nullptr) return rs.own_bytes >= need ? rs.own : nullptr;
  return rs.pool ? pool_ring(stream, need) : nullptr;
}

// include/amcx.h, DEVICE OWNERSHIP: a device pointer must live on the current device.  Pointers the
// runtime does not know (or host-visible ones) are let through -- the launch itself will say.
bool on_another_device(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  if (a.type != hipMemoryTypeDevice) return false;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return false; }
  return a.device != dev;
}

// spectral-term variant of the block kernel for this frame size
int block_mode(int N) {
  if (is_pow2(N)) return amcx::kBlockPow2;
  if (N >= amcx::kBluesteinMinN && N <= amcx::kBluesteinMaxN) return amcx::kBlockBluestein;
  return N > amcx::kBluesteinMaxN ? amcx::kBlockBluesteinBig : amcx::kBlockDirect;
}

// 8192 < N <= 32768: one 1024-thread workgroup per frame, the frame read where it lies (amcx_stream_kernel.h).  With a
// workspace of at least one workgroup's share the spectral term is an FFT through it (Bluestein for the sizes that are
// not powers of two), otherwise the DFT by its definition.
struct StreamPlan {
  int M;            // transform length of the FFT form
  bool chirped;     // not a power of two: one more buffer of M for the chirp's spectrum
  int64_t grid;     // workgroups = frames in flight
};

StreamPlan stream_plan(int32_t N, int64_t n_frames) {
  StreamPlan p;
  p.M = amcx::stream::conv_length(N);
  p.chirped = !is_pow2(N);
  p.grid = amcx::persistent_grid(cu_count(), 1, n_frames, 1);   // one resident workgroup per CU, grid-stride beyond
  return p;
}

int launch_stream(const amcx::Frames& a, int32_t N, void* ws, int64_t ws_bytes) {
  namespace st = amcx::stream;
  StreamPlan p = stream_plan(N, a.n_frames);
  const int64_t per = (int64_t)p.M * (int64_t)sizeof(float2);
  int64_t fit = ws != nullptr && ws_bytes > 0 ? ws_bytes / per - (p.chirped ? 1 : 0) : 0;   // workgroups the workspace has room for
  if (fit >= 1 && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0) {
    if (p.grid > fit) p.grid = fit;
    float2* const base = static_cast<float2*>(ws);
    const float2* bspec = nullptr;
    float2* bufs = base;
    if (p.chirped) {
      constexpr auto chirp = st::amcx_stream_chirp_kernel;
      constexpr int lds = st::kTileBytes + st::kFftTabBytes;
      AMCX_HIP(amcx::lds_attr_once<chirp>(lds));
      AMCX_HIP(amcx::launch(chirp, 1, st::kThreads, lds, a.stream, base, N, p.M));
      bspec = base;
      bufs = base + p.M;
    }
    constexpr auto kern = st::amcx_features18_stream_kernel<true>;
    AMCX_HIP(amcx::lds_attr_once<kern>((int)st::lds_bytes_fft(st::kMaxN)));
    AMCX_HIP(amcx::launch(kern, p.grid, st::kThreads, st::lds_bytes_fft(N), a.stream, a.iq, a.n_frames, N, a.row_stride, a.out,
                          a.out_stride, bspec, bufs, p.M));
    return AMCX_OK;
  }
  constexpr auto kern = st::amcx_features18_stream_kernel<false>;
  AMCX_HIP(amcx::lds_attr_once<kern>((int)st::lds_bytes(st::kMaxN)));
  AMCX_HIP(amcx::launch(kern, p.grid, st::kThreads, st::lds_bytes(N), a.stream, a.iq, a.n_frames, N, a.row_stride, a.out,
                        a.out_stride, nullptr, nullptr, 0));
  return AMCX_OK;
}

template <int MODE>
int launch_block_mode(const amcx::Frames& a, int32_t N) {
  constexpr auto kern = amcx::amcx_features18_block_kernel<MODE>;
  constexpr int kMaxLds = 16 * amcx::kBlockMaxN + amcx::kBlockScratchBytes + amcx::kBlockTwiddleBytes;
  const size_t lds = (MODE == amcx::kBlockBluestein      ? (size_t)16 * amcx::bluestein_length(N)
                      : MODE == amcx::kBlockBluesteinBig ? (size_t)8 * amcx::kBluesteinBigM
                                                         : (size_t)16 * N) +
                     amcx::kBlockScratchBytes + amcx::kBlockTwiddleBytes;
  AMCX_HIP(amcx::lds_attr_once<kern>(kMaxLds));
  // enough workgroups to fill every CU at the occupancy LDS allows, grid-stride beyond
  const int per_cu = (int)((160 * 1024) / lds) < 1 ? 1 : (int)((160 * 1024) / lds);
  const int64_t grid = amcx::persistent_grid(a.cus, (per_cu > 8 ? 8 : per_cu) * 4, a.n_frames, 1);
  AMCX_HIP(amcx::launch(kern, grid, amcx::kBlockThreads, lds, a.stream, a.iq, a.n_frames, N, a.row_stride, a.out, a.out_stride));
  return AMCX_OK;
}

int launch_block(const amcx::Frames& a, int32_t N, void* ws = nullptr, int64_t ws_bytes = 0) {
  if (N > amcx::kBlockMaxN) return launch_stream(a, N, ws, ws_bytes);
  switch (block_mode(N)) {
    case amcx::kBlockPow2: return launch_block_mode<amcx::kBlockPow2>(a, N);
    case amcx::kBlockBluestein: return launch_block_mode<amcx::kBlockBluestein>(a, N);
    case amcx::kBlockBluesteinBig: return launch_block_mode<amcx::kBlockBluesteinBig>(a, N);
    default: return launch_block_mode<amcx::kBlockDirect>(a, N);
  }
}

// ---- the feature entry: one validation, one dispatch ------------------------------------------------------------------
bool valid_feature_mask(uint32_t mask) { return mask != 0 && (mask & ~(uint32_t)AMCX_FEATURES_ALL) == 0; }

// which kernel a feature mask runs (include/amcx.h): a plan kernel where one exists for (frame size, resolved
// variant), the 18-feature kernel (+ the column mask) otherwise
int subset_plan(int32_t N, int v, uint32_t mask) {
  if ((mask & 1u) != 0 || v != AMCX_VARIANT_WAVE || !amcx::has_plan_kernels(N)) return amcx::kPlanAll;
  return (mask & ~amcx::kMaskCumulants) == 0 ? amcx::kPlanCumulants : amcx::kPlanNoSpectral;
}

// f(the run-time plan as an integral_constant)  (kPlanAll stands first: KERNEL ORDER, amcx_launch.h)
template <class F>
auto with_plan(int plan, F&& f) {
  using std::integral_constant;
  return plan == amcx::kPlanAll         ? f(integral_constant<int, amcx::kPlanAll>{})
         : plan == amcx::kPlanCumulants ? f(integral_constant<int, amcx::kPlanCumulants>{})
                                        : f(integral_constant<int, amcx::kPlanNoSpectral>{});
}

// sc16 frames of this size are read by a kernel of their own (resolved variant v); false: widened to complex64 first
bool sc16_typed(int32_t N, int v) {
  // (called out of line, as the parent's callers did: the library exports its inline host helpers -- build.py sets no
  //  visibility -- and amcx::has_sc16_kernels stays in that list)
  [[clang::noinline]] return v == AMCX_VARIANT_WAVE && amcx::has_sc16_kernels(N);
}

// The end of a call that ran on a workspace of its own from the stream-ordered allocator (here and amcx_group_stats_f32):
// freed in stream order whatever the call said, and the first failure is the one reported.
int free_own_ws(void* ws, hipStream_t st, int rc) {
  const hipError_t fe = hipFreeAsync(ws, st);
  return rc != AMCX_OK || fe == hipSuccess ? rc : hip_fail(fe, "hipFreeAsync(ws, st)");
}

// The any-size path above 8192 samples runs its FFT form through a workspace from the stream-ordered allocator
// (as amcx_group_stats_f32 does) -- unless the stream is being captured into a graph, or the allocator has nothing:
// then the DFT by its definition, which needs none (amcx_stream_kernel.h).  Everything else allocates nothing.
int launch_block_own_ws(const amcx::Frames& a, int32_t N) {
  const hipStream_t st = a.stream;
  const int64_t want = amcx_features18_workspace_bytes(N, a.n_frames, AMCX_VARIANT_BLOCK);
  if (want <= 0) return launch_block(a, N);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
  void* ws = nullptr;
  if (cap == hipStreamCaptureStatusNone && hipMallocAsync(&ws, (size_t)want, st) != hipSuccess) {
    (void)hipGetLastError();
    ws = nullptr;
  }
  // Which form ran is otherwise invisible (amcx_kernel_name says amcx_features18_stream_kernel either way, the results
  // agree to 8e-7): AMCX_VERBOSE=1 says it once per process on stderr when the O(N^2) form is taken.  A caller that
  // must not fall back hands in its own workspace (amcx_features18_c64_ws), as amcpy_amd.features.features18 does.
  if (ws == nullptr) {
    static const bool verbose = [] { const char* t = getenv("AMCX_VERBOSE"); return t != nullptr && t[0] != '\0' && t[0] != '0'; }();
    static std::atomic<bool> said{false};
    if (verbose && !said.exchange(true))
      fprintf(stderr, "amcx: frame_size %d runs the DFT by its definition (O(N^2)): %s; amcx_features18_c64_ws with %lld "
                      "bytes of workspace selects the FFT form\n", (int)N,
              cap != hipStreamCaptureStatusNone ? "the stream is being captured" : "hipMallocAsync had no workspace", (long long)want);
  }
  const int rc = launch_block(a, N, ws, ws != nullptr ? want : 0);
  return ws != nullptr ? free_own_ws(ws, st, rc) : rc;
}

// where the any-size path's workspace comes from: the caller's (or none), or launch_block_own_ws
struct Workspace {
  void* dev = nullptr;
  int64_t bytes = 0;
  bool own = false;
};

// Integer frames: iq_dev holds int16 pairs (include/amcx.h, amcx_features_sc16) or, iq8 >= 0, pairs of bytes in the format
// AMCX_IQ8_CI8 / AMCX_IQ8_CU8 (amcx_features_iq8); a component's value is (float)integer * scale
struct IntIn {
  float scale;
  int32_t iq8 = -1;
  bool is_iq8() const { return iq8 >= 0; }
  unsigned flip() const { return iq8 == AMCX_IQ8_CU8 ? 0x80u : 0x00u; }     // amcx_iq8_kernels.h
};
inline bool int_scale_ok(float scale) { return scale > 0.0f && scale <= 3.4028235e38f; }   // not NaN, inf, <= 0
inline bool iq8_format_ok(int32_t format) { return format == AMCX_IQ8_CI8 || format == AMCX_IQ8_CU8; }
inline int64_t sc16_widened_bytes(int32_t N, int64_t n_frames) { return (8 * (int64_t)N * n_frames + 255) / 256 * 256; }
// the widened copy of 8-bit frames: sc16 where an sc16 kernel reads it (typed), complex64 otherwise
inline int64_t iq8_widened_bytes(int32_t N, int64_t n_frames, bool typed) {
  return ((typed ? 4 : 8) * (int64_t)N * n_frames + 255) / 256 * 256;
}
// (defined behind run_features: KERNEL ORDER, amcx_launch.h)
hipError_t launch_sc16_plan(const amcx::Frames& frames, int32_t N, int plan, float* ring, uint32_t mask);
hipError_t launch_sc16_widen(const amcx::Frames& frames, int32_t N, float2* dst);
hipError_t launch_iq8_widen(const void* src, int64_t n_frames, int32_t N, int64_t src_stride, const IntIn& in, bool to_sc16,
                            void* dst, hipStream_t stream);

// Behind amcx_features18_c64_ws / _ex, amcx_features_c64_subset, amcx_features_sc16, amcx_features_iq8 and the contexts (ctx_features);
// feature_mask is AMCX_FEATURES_ALL for the 18-feature entries.  The order of the checks is part of the ABI
// (tests/c_abi/abi_check.c).  sc16: the frames are sc16, not complex64 -- a kernel over sc16 where the size has one, otherwise
// widened into the head of the workspace, the complex64 path with the rest of it.  8-bit frames are ALWAYS widened into the
// head of the workspace first: to sc16 where the size has an sc16 kernel, which then runs, to complex64 otherwise.
int run_features(const void* iq_dev, int64_t n_frames, int32_t frame_size, int64_t row_stride_elems, float* out_dev,
                 int64_t out_row_stride, void* hip_stream, int32_t variant, uint32_t feature_mask, const Workspace& ws_in,
                 const RingSource& rings, const IntIn* sc16 = nullptr) {
  if (!valid_feature_mask(feature_mask)) return AMCX_EINVAL;
  if (sc16 != nullptr && !int_scale_ok(sc16->scale)) return AMCX_EINVAL;
  const bool iq8 = sc16 != nullptr && sc16->is_iq8();
  // (amcx_features_iq8 alone: what can be said of its format and of the addresses it was given, before the no-op)
  if (iq8 && (!iq8_format_ok(sc16->iq8) || (reinterpret_cast<uintptr_t>(iq_dev) & 1u) || (reinterpret_cast<uintptr_t>(ws_in.dev) & 7u)))
    return AMCX_EINVAL;
  if (n_frames < 0 || row_stride_elems < frame_size || out_row_stride < AMCX_NUM_FEATURES) return AMCX_EINVAL;
  const int v = resolve_variant(frame_size, variant);
  if (v < 0) return v;
  if (n_frames == 0) return AMCX_OK;
  if (iq_dev == nullptr || out_dev == nullptr) return AMCX_EINVAL;
  if ((reinterpret_cast<uintptr_t>(iq_dev) & (iq8 ? 1u : sc16 != nullptr ? 3u : 7u)) || (reinterpret_cast<uintptr_t>(out_dev) & 3u))
    return AMCX_EINVAL;
  const bool typed = sc16 != nullptr && sc16_typed(frame_size, v);
  const bool widens = sc16 != nullptr && (iq8 || !typed);
  Workspace ws = ws_in;
  if (widens) {      // the widened copy takes the head of the caller's workspace
    const int64_t head = iq8 ? iq8_widened_bytes(frame_size, n_frames, typed) : sc16_widened_bytes(frame_size, n_frames);
    if (ws.own || ws.dev == nullptr || ws.bytes < head || (reinterpret_cast<uintptr_t>(ws.dev) & 7u)) return AMCX_EINVAL;
    ws.dev = static_cast<char*>(ws_in.dev) + head;
    ws.bytes = ws_in.bytes - head;
    if (ws.bytes == 0) ws.dev = nullptr;
  }
  if (on_another_device(iq_dev) || on_another_device(out_dev)) return AMCX_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  amcx::Frames frames{static_cast<const float2*>(iq_dev), n_frames, row_stride_elems, out_dev, out_row_stride, stream, cu_count()};
  if (sc16 != nullptr) {
    frames.iq = nullptr;
    frames.iq16 = static_cast<const amcx::wave::sc16*>(iq_dev);
    frames.scale = sc16->scale;
    if (widens) {
      if (on_another_device(ws_in.dev)) return AMCX_EINVAL;
      if (iq8) {
        const hipError_t e = launch_iq8_widen(iq_dev, n_frames, frame_size, row_stride_elems, *sc16, typed, ws_in.dev, stream);
        if (e != hipSuccess) return hip_fail(e, "8-bit widening kernel launch");
        frames.iq16 = static_cast<const amcx::wave::sc16*>(ws_in.dev);       // (read only where typed)
      } else {
        const hipError_t e = launch_sc16_widen(frames, frame_size, static_cast<float2*>(ws_in.dev));
        if (e != hipSuccess) return hip_fail(e, "sc16 widening kernel launch");
      }
      if (!typed) {
        frames.iq = static_cast<const float2*>(ws_in.dev);
        frames.iq16 = nullptr;
      }
      frames.row_stride = frame_size;
    }
  }
  const int plan = subset_plan(frame_size, v, feature_mask);
  int rc;
  if (typed) {
    const hipError_t e = launch_sc16_plan(frames, frame_size, plan, ring_for(rings, frame_size, stream), feature_mask);
    if (e != hipSuccess) return hip_fail(e, "sc16 kernel launch");
    rc = AMCX_OK;
  } else if (v == AMCX_VARIANT_WAVE) {
    // Every throughput kernel (amcx_launch.h, THE FRAME-SIZE TABLE) has re-run the frames outside its fp32 sums' range
    // itself -- one launch, rows final -- and finished frames with a phase step within an angle rounding of +-pi in its
    // finaliser.
    float* const ring = ring_for(rings, frame_size, stream);
    const hipError_t e = with_plan(plan, [&](auto plan_c) {       // (subset_plan names a plan only where the size has its kernels)
      return amcx::for_frame_size(frame_size, [&](auto size) {
        using S = decltype(size);
        constexpr int kPlan = S::kPlanStem != nullptr ? decltype(plan_c)::value : amcx::kPlanAll;
        return S::template launch<kPlan>(frames, ring, feature_mask);
      });
    });
    if (e != hipSuccess) return hip_fail(e, plan == amcx::kPlanAll ? "wave kernel launch" : "feature-subset kernel launch");
    rc = AMCX_OK;
  } else if (ws.own) {
    rc = launch_block_own_ws(frames, frame_size);
  } else {
    if (ws.dev != nullptr && on_another_device(ws.dev)) return AMCX_EINVAL;
    rc = launch_block(frames, frame_size, ws.dev, ws.bytes < 0 ? 0 : ws.bytes);
  }
  // a plan kernel has written NaN into the columns outside the mask itself
  if (rc != AMCX_OK || plan != amcx::kPlanAll || feature_mask == (uint32_t)AMCX_FEATURES_ALL) return rc;
  int64_t grid = (n_frames * AMCX_NUM_FEATURES + 255) / 256;
  if (grid > 8192) grid = 8192;
  AMCX_HIP(amcx::launch(amcx::amcx_mask_columns_kernel, grid, 256, 0, stream, out_dev, n_frames, out_row_stride, feature_mask));
  return AMCX_OK;
}

// the sc16 kernel of (frame size, plan): amcx_launch.h, THE FRAME-SIZE TABLE
hipError_t launch_sc16_plan(const amcx::Frames& frames, int32_t N, int plan, float* ring, uint32_t mask) {
  return with_plan(plan, [&](auto plan_c) {
    return amcx::for_frame_size(N, [&](auto size) {
      using S = decltype(size);
      if constexpr (S::kSc16Stem != nullptr) return S::template launch<decltype(plan_c)::value, amcx::wave::sc16>(frames, ring, mask);
      else return hipErrorNotSupported;
    });
  });
}

// sc16 rows -> packed complex64 rows of N samples at dst (amcx_sc16_kernels.h)
hipError_t launch_sc16_widen(const amcx::Frames& frames, int32_t N, float2* dst) {
  const int64_t grid = amcx::persistent_grid(frames.cus, 8, frames.n_frames * N, 256);
  return amcx::launch(amcx::amcx_sc16_to_c64_kernel, grid, 256, 0, frames.stream, frames.iq16, frames.n_frames, N,
                      frames.row_stride, frames.scale, dst);
}

// 8-bit rows -> packed sc16 / complex64 rows of N samples at dst (amcx_iq8_kernels.h): an item of 8 samples per thread
hipError_t launch_iq8_widen(const void* src, int64_t n_frames, int32_t N, int64_t src_stride, const IntIn& in, bool to_sc16,
                            void* dst, hipStream_t stream) {
  const int64_t items = n_frames * ((N + amcx::kIq8Item - 1) / amcx::kIq8Item);
  const int64_t grid = amcx::persistent_grid(cu_count(), 8, items, 256);
  const uint8_t* const bytes = static_cast<const uint8_t*>(src);
  if (to_sc16)
    return amcx::launch(amcx::amcx_iq8_to_sc16_kernel, grid, 256, 0, stream, bytes, n_frames, N, src_stride, in.flip(),
                        static_cast<short2*>(dst));
  return amcx::launch(amcx::amcx_iq8_to_c64_kernel, grid, 256, 0, stream, bytes, n_frames, N, src_stride, in.flip(), in.scale,
                      static_cast<float2*>(dst));
}

}  // namespace

#include "amcx_ctx.h"      // the contexts and their upload engine, built on run_features (KERNEL ORDER: it names the packing kernels)
#include "amcx_probe.h"    // the two probes: plain kernels, the last of .text as they always were

namespace {

// how a statistics call is cut: chunks per group and rows per chunk (whole tiles).  n_groups >= 1; chunks <= want, so the
// grid n_groups * chunks stays below n_groups + 1024: a 32-bit count for every n_groups stats_args_ok lets through
void stats_plan(int64_t n_groups, int64_t rows_per_group, int n_cols, int64_t* chunks, int64_t* rows_per_chunk) {
  const int64_t tile = amcx::stat_tile_rows(n_cols);
  const int64_t tiles = (rows_per_group + tile - 1) / tile;
  const int64_t target = 1024;                               // workgroups wanted in all (4 per CU, one resident round); the same on any device
  int64_t want = (target + n_groups - 1) / n_groups;
  if (want > tiles) want = tiles;
  if (want < 1) want = 1;
  const int64_t tiles_per_chunk = (tiles + want - 1) / want;
  *rows_per_chunk = tiles_per_chunk * tile;
  *chunks = (tiles + tiles_per_chunk - 1) / tiles_per_chunk;
}

bool stats_args_ok(int64_t n_groups, int64_t rows_per_group, int64_t row_stride, int32_t n_cols) {
  return n_groups >= 0 && rows_per_group >= 1 && n_cols >= 1 && n_cols <= amcx::kStatMaxCols &&
         row_stride >= n_cols && row_stride <= (1 << 20) && n_groups <= 0x7fffffffLL;
}

// widths[0 .. n_linear]: every width 1 ... 32, 1 ... 6 layers
bool mlp_shape_ok(const int32_t* widths, int32_t n_linear) {
  if (widths == nullptr || n_linear < 1 || n_linear > amcx::kMlpMaxLinear) return false;
  for (int l = 0; l <= n_linear; ++l)
    if (widths[l] < 1 || widths[l] > amcx::kMlpMaxWidth) return false;
  return true;
}

// ---- what the stream entries share (amcx_tune_decimate, amcx_filter_bank, amcx_resample) ------------------------------------
// What such an entry derives from src_kind.
struct StreamSrc {
  int32_t kind;
  bool integer() const { return kind == AMCX_SRC_SC16 || kind == AMCX_SRC_CI8 || kind == AMCX_SRC_CU8; }
  // a source kind at all, and for the integer ones a scale the kernels can multiply by
  bool ok(float scale) const { return (kind == AMCX_SRC_C64 || integer()) && (!integer() || int_scale_ok(scale)); }
  unsigned src_align() const { return kind == AMCX_SRC_C64 ? 7u : kind == AMCX_SRC_SC16 ? 3u : 1u; }      // a sample's bytes, less one
  float kernel_scale(float scale) const { return integer() ? scale : 1.0f; }
  unsigned flip4() const { return kind == AMCX_SRC_CU8 ? 0x80808080u : 0u; }
  // of a family's three: the complex64 kernel's, the sc16 kernel's, the 8-bit kernel's (ci8 and cu8); K{} where `kind` is no source
  template <class K>
  K pick(K c64, K sc16, K iq8) const {
    return kind == AMCX_SRC_C64 ? c64 : kind == AMCX_SRC_SC16 ? sc16 : kind == AMCX_SRC_CI8 || kind == AMCX_SRC_CU8 ? iq8 : K{};
  }
};

// a family's kernel with its name; the bank's, which ask for more than 64 KiB of LDS, with their lds_attr_once too
template <class Kern>
struct StreamKernel {
  Kern kern;
  const char* name;
};
struct BankKernel : StreamKernel<decltype(&amcx::amcx_bank_c64_kernel)> {
  hipError_t (*lds_attr)(int most);
};
#define AMCX_NAMED(k) amcx::k, #k
StreamKernel<decltype(&amcx::amcx_ddc_c64_kernel)> ddc_kernel(StreamSrc s) {
  return s.pick<StreamKernel<decltype(&amcx::amcx_ddc_c64_kernel)>>(
      {AMCX_NAMED(amcx_ddc_c64_kernel)}, {AMCX_NAMED(amcx_ddc_sc16_kernel)}, {AMCX_NAMED(amcx_ddc_iq8_kernel)});
}
BankKernel bank_kernel(StreamSrc s) {
  return s.pick<BankKernel>({{AMCX_NAMED(amcx_bank_c64_kernel)}, amcx::lds_attr_once<amcx::amcx_bank_c64_kernel>},
                            {{AMCX_NAMED(amcx_bank_sc16_kernel)}, amcx::lds_attr_once<amcx::amcx_bank_sc16_kernel>},
                            {{AMCX_NAMED(amcx_bank_iq8_kernel)}, amcx::lds_attr_once<amcx::amcx_bank_iq8_kernel>});
}
StreamKernel<decltype(&amcx::amcx_resample_c64_kernel)> rs_kernel(StreamSrc s) {
  return s.pick<StreamKernel<decltype(&amcx::amcx_resample_c64_kernel)>>(
      {AMCX_NAMED(amcx_resample_c64_kernel)}, {AMCX_NAMED(amcx_resample_sc16_kernel)}, {AMCX_NAMED(amcx_resample_iq8_kernel)});
}
StreamKernel<decltype(&amcx::amcx_spectrogram_c64_kernel)> psd_kernel(StreamSrc s) {
  return s.pick<StreamKernel<decltype(&amcx::amcx_spectrogram_c64_kernel)>>(
      {AMCX_NAMED(amcx_spectrogram_c64_kernel)}, {AMCX_NAMED(amcx_spectrogram_sc16_kernel)}, {AMCX_NAMED(amcx_spectrogram_iq8_kernel)});
}
#undef AMCX_NAMED

// ---- the host gates of the entries that launch: limits (these), the no-op return, then the pointers (ptrs_ok) ---------------
// n_rows rows at row_stride elements: the stride holds a row, and the product stays below 2^58 (each factor bounded first)
bool rows_ok(int64_t n_rows, int64_t row_stride, int32_t row_elems) {
  return n_rows >= 0 && row_stride >= row_elems && (n_rows == 0 || row_stride <= (int64_t(1) << 58) / n_rows);
}
// an optional output of n_rows rows of row_elems elements: where it is asked for, its stride passes rows_ok
bool opt_rows_ok(const void* out, int64_t n_rows, int64_t row_stride, int32_t row_elems) {
  return out == nullptr || rows_ok(n_rows, row_stride, row_elems);
}
// rows_per_group of an entry that counts per group: never below 0, 1 at least where counts are asked for, and then whole groups
bool groups_ok(int64_t n_rows, int64_t rows_per_group, const void* counts) {
  return rows_per_group >= 0 && (rows_per_group > 0 || counts == nullptr) && (rows_per_group == 0 || n_rows % rows_per_group == 0);
}
bool threshold_ok(float threshold) { return int_scale_ok(threshold); }      // the same rule: a finite float32 > 0
int log2_exact(int n) {      // of a power of two
  int lg = 0;
  while ((1 << lg) < n) ++lg;
  return lg;
}
int psd_log2(int32_t nfft) {
  return nfft < amcx::kPsdMinFft || nfft > amcx::kPsdMaxFft || !is_pow2(nfft) ? -1 : log2_exact(nfft);
}

// one pointer of a call that launches: its element's bytes less one, and whether the call needs it
struct Ptr { const void* p; unsigned align_mask; bool required; };
// a required pointer is there; then every pointer that is there is aligned to its element; then none of them is on another device
bool ptrs_ok(std::initializer_list<Ptr> ptrs) {
  for (const Ptr& a : ptrs)
    if (a.required && a.p == nullptr) return false;
  for (const Ptr& a : ptrs)
    if (reinterpret_cast<uintptr_t>(a.p) & a.align_mask) return false;
  for (const Ptr& a : ptrs)
    if (a.p != nullptr && on_another_device(a.p)) return false;
  return true;
}
// a stream entry's three, all required (out: complex64, or float32 rows with out_align = 3)
bool stream_ptrs_ok(const void* src, const float* taps, const void* out, StreamSrc s, unsigned out_align = 7u) {
  return ptrs_ok({{src, s.src_align(), true}, {taps, 3u, true}, {out, out_align, true}});
}

// resident workgroups per CU of a launch with `lds_bytes` of dynamic LDS: what the CU's 160 KiB leave room for, `cap` at most
int wgs_per_cu(size_t lds_bytes, int cap) {
  const int fit = (int)((size_t)(160 * 1024) / lds_bytes);
  return fit < 1 ? 1 : fit > cap ? cap : fit;
}
int ddc_wgs_per_cu(int n_taps, int decim) { return wgs_per_cu(amcx::ddc_lds_bytes(n_taps, decim), 8); }
int rs_wgs_per_cu(int n_taps, int interp, int decim) { return wgs_per_cu(amcx::rs_lds_bytes(n_taps, interp, decim), 8); }
int bank_wgs_per_cu(int n_taps, int channels, int decim) { return wgs_per_cu(amcx::bank_lds_bytes(n_taps, channels, decim), 4); }

int put_kernel_name(const char* name, char* buf, int32_t buf_len) {
  if (buf == nullptr || buf_len <= 0 || name == nullptr) return AMCX_EINVAL;
  snprintf(buf, (size_t)buf_len, "%s", name);
  return AMCX_OK;
}

// the columns a post-processing entry selects (n_sel in range already); false: one of them is not a column of the input
bool make_select_cols(const int32_t* cols_host, int32_t n_sel, int32_t n_cols, amcx::SelectCols* sel) {
  sel->n = n_sel;
  for (int j = 0; j < amcx::kStatMaxCols; ++j) sel->c[j] = 0;
  for (int j = 0; j < n_sel; ++j) {
    if (cols_host[j] < 0 || cols_host[j] >= n_cols) return false;
    sel->c[j] = cols_host[j];
  }
  return true;
}

// what the three network entries (amcx_mlp_classify_f32, amcx_mlp_range_f32, amcx_mlp_classify_q15) ask of their rows, columns,
// scaler and shape
bool mlp_rows_ok(int64_t n_rows, int64_t row_stride, int32_t n_cols, const int32_t* cols_host, int32_t n_sel, const double* mean_dev,
                 const double* scale_dev, const int32_t* widths_host, int32_t n_linear, amcx::SelectCols* sel) {
  if (n_cols < 1 || n_cols > amcx::kStatMaxCols || !rows_ok(n_rows, row_stride, n_cols) || cols_host == nullptr ||
      !mlp_shape_ok(widths_host, n_linear) || n_sel != widths_host[0])
    return false;
  if ((mean_dev == nullptr) != (scale_dev == nullptr)) return false;
  return make_select_cols(cols_host, n_sel, n_cols, sel);
}
amcx::MlpShape mlp_shape(const int32_t* widths_host, int32_t n_linear, int32_t activation) {
  amcx::MlpShape shape;
  shape.n_linear = n_linear;
  shape.act = activation;
  for (int l = 0; l <= amcx::kMlpMaxLinear; ++l) shape.w[l] = l <= n_linear ? widths_host[l] : 0;
  return shape;
}
int64_t mlp_tiles(int64_t n_rows) { return (n_rows + amcx::kMlpTileRows - 1) / amcx::kMlpTileRows; }      // what a network kernel walks
// n 64-bit counters to zero on the stream: a classifier's counts, the Q15 entry's saturation counters (nullptr: not asked for, no launch)
int zero_counters(unsigned long long* counters, int64_t n, hipStream_t st, const char* what) {
  if (counters == nullptr) return AMCX_OK;
  const int64_t zgrid = (n + 255) / 256;
  const hipError_t e = amcx::launch(amcx::amcx_mlp_zero_counts_kernel, zgrid < 1024 ? zgrid : 1024, 256, 0, st, counters, n);
  return e != hipSuccess ? hip_fail(e, what) : AMCX_OK;
}

// the two launches of a statistics call, behind its entry's gate: a chunk's triple per workgroup into `ws`, then the pooling
int launch_stats(const float* x_dev, int64_t n_groups, int64_t rows_per_group, int64_t row_stride, int32_t n_cols, double* mean_dev,
                 double* std_dev, void* ws, hipStream_t st) {
  int64_t chunks, rpc;
  stats_plan(n_groups, rows_per_group, n_cols, &chunks, &rpc);
  double* const part = static_cast<double*>(ws);
  hipError_t e = amcx::launch(amcx::amcx_stats_part_kernel, n_groups * chunks, amcx::kStatThreads, 0, st, x_dev, rows_per_group,
                              row_stride, n_cols, rpc, chunks, part);
  if (e != hipSuccess) return hip_fail(e, "statistics chunk kernel launch");
  // one small workgroup per (column, group); groups beyond the grid's y limit go in slices
  const int pool_threads = chunks > 128 ? 256 : chunks > 64 ? 128 : 64;
  for (int64_t g0 = 0; g0 < n_groups; g0 += 65535) {
    const int64_t ng = n_groups - g0 < 65535 ? n_groups - g0 : 65535;
    e = amcx::launch(amcx::amcx_stats_combine_kernel, dim3((unsigned)n_cols, (unsigned)ng), pool_threads, 0, st,
                     part + g0 * n_cols * 3 * chunks, chunks, n_cols, mean_dev + g0 * n_cols, std_dev + g0 * n_cols);
    if (e != hipSuccess) return hip_fail(e, "statistics pooling kernel launch");
  }
  return AMCX_OK;
}

}  // namespace

extern "C" {

int amcx_abi_version(void) { return AMCX_ABI_VERSION; }

const char* amcx_strerror(int code) {
  switch (code) {
    case AMCX_OK: return "ok";
    case AMCX_EINVAL: return "invalid argument (null pointer, negative count, stride or frame_size out of range)";
    case AMCX_ENOTSUP: return "kernel variant does not support this frame_size";
    case AMCX_EHIP: return "HIP runtime error (see amcx_last_hip_error)";
    case AMCX_ENODEV: return "no usable gfx950 device";
    case AMCX_ENOMEM: return "device memory allocation failed";
    case AMCX_EIO: return "reading the container's file failed (see amcx_last_hip_error for the errno text)";
    default: return "unknown amcx error code";
  }
}

const char* amcx_last_hip_error(void) { return g_hip_err; }

int amcx_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e == hipErrorNoDevice) return 0;
  if (e != hipSuccess) return hip_fail(e, "hipGetDeviceCount");
  int ok = 0;
  for (int d = 0; d < n; ++d) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, d) == hipSuccess && strncmp(p.gcnArchName, "gfx950", 6) == 0) ++ok;
  }
  return ok;
}

int64_t amcx_features18_workspace_bytes(int32_t frame_size, int64_t n_frames, int32_t variant) {
  if (n_frames < 0) return -1;
  const int v = resolve_variant(frame_size, variant);
  if (v < 0) return -1;
  if (v != AMCX_VARIANT_BLOCK || frame_size <= amcx::kBlockMaxN || n_frames == 0) return 0;
  const StreamPlan p = stream_plan(frame_size, n_frames);
  return (p.grid + (p.chirped ? 1 : 0)) * (int64_t)p.M * (int64_t)sizeof(float2);
}

int amcx_features18_c64_ws(const void* iq_dev, int64_t n_frames, int32_t frame_size,
                           int64_t row_stride_elems, float* out_dev, int64_t out_row_stride,
                           void* hip_stream, int32_t variant, void* workspace_dev, int64_t workspace_bytes) {
  return amcx_features_c64_subset(iq_dev, n_frames, frame_size, row_stride_elems, out_dev, out_row_stride, hip_stream, variant,
                                  AMCX_FEATURES_ALL, workspace_dev, workspace_bytes);
}

int amcx_features_c64_subset(const void* iq_dev, int64_t n_frames, int32_t frame_size, int64_t row_stride_elems,
                             float* out_dev, int64_t out_row_stride, void* hip_stream, int32_t variant, uint32_t feature_mask,
                             void* workspace_dev, int64_t workspace_bytes) {
  Workspace ws;
  ws.dev = workspace_dev;
  ws.bytes = workspace_bytes;
  RingSource rings;
  rings.pool = true;
  return run_features(iq_dev, n_frames, frame_size, row_stride_elems, out_dev, out_row_stride, hip_stream, variant,
                      feature_mask, ws, rings);
}

int64_t amcx_features_sc16_workspace_bytes(int32_t frame_size, int64_t n_frames, int32_t variant) {
  if (n_frames < 0) return -1;
  const int v = resolve_variant(frame_size, variant);
  if (v < 0) return -1;
  if (n_frames == 0 || sc16_typed(frame_size, v)) return 0;
  return sc16_widened_bytes(frame_size, n_frames) + amcx_features18_workspace_bytes(frame_size, n_frames, variant);
}

int amcx_features_sc16(const void* iq_dev, int64_t n_frames, int32_t frame_size, int64_t row_stride_samples, float scale,
                       float* out_dev, int64_t out_row_stride, void* hip_stream, int32_t variant, uint32_t feature_mask,
                       void* workspace_dev, int64_t workspace_bytes) {
  Workspace ws;
  ws.dev = workspace_dev;
  ws.bytes = workspace_bytes;
  RingSource rings;
  rings.pool = true;
  const IntIn in{scale};
  return run_features(iq_dev, n_frames, frame_size, row_stride_samples, out_dev, out_row_stride, hip_stream, variant,
                      feature_mask, ws, rings, &in);
}

int64_t amcx_features_iq8_workspace_bytes(int32_t frame_size, int64_t n_frames, int32_t variant) {
  if (n_frames < 0) return -1;
  const int v = resolve_variant(frame_size, variant);
  if (v < 0) return -1;
  if (n_frames == 0) return 0;
  if (sc16_typed(frame_size, v)) return iq8_widened_bytes(frame_size, n_frames, true);
  return iq8_widened_bytes(frame_size, n_frames, false) + amcx_features18_workspace_bytes(frame_size, n_frames, variant);
}

int amcx_features_iq8(const void* iq_dev, int64_t n_frames, int32_t frame_size, int64_t row_stride_samples, int32_t format,
                      float scale, float* out_dev, int64_t out_row_stride, void* hip_stream, int32_t variant,
                      uint32_t feature_mask, void* workspace_dev, int64_t workspace_bytes) {
  Workspace ws;
  ws.dev = workspace_dev;
  ws.bytes = workspace_bytes;
  RingSource rings;
  rings.pool = true;
  const IntIn in{scale, format < 0 ? INT32_MAX : format};      // (a format below 0 is a bad format, not sc16)
  return run_features(iq_dev, n_frames, frame_size, row_stride_samples, out_dev, out_row_stride, hip_stream, variant,
                      feature_mask, ws, rings, &in);
}

int amcx_features18_c64_ex(const void* iq_dev, int64_t n_frames, int32_t frame_size,
                           int64_t row_stride_elems, float* out_dev, int64_t out_row_stride,
                           void* hip_stream, int32_t variant) {
  Workspace ws;
  ws.own = true;                   // (launch_block_own_ws: asked for only once the arguments have passed)
  RingSource rings;
  rings.pool = true;
  return run_features(iq_dev, n_frames, frame_size, row_stride_elems, out_dev, out_row_stride, hip_stream, variant,
                      AMCX_FEATURES_ALL, ws, rings);
}

int amcx_features18_c64(const void* iq_dev, int64_t n_frames, int32_t frame_size,
                        int64_t row_stride_elems, float* out_dev, int64_t out_row_stride,
                        void* hip_stream) {
  return amcx_features18_c64_ex(iq_dev, n_frames, frame_size, row_stride_elems, out_dev,
                                out_row_stride, hip_stream, AMCX_VARIANT_AUTO);
}

int amcx_ctx_create(int32_t device, amcx_ctx** ctx_out) {
  if (ctx_out == nullptr) return AMCX_EINVAL;
  *ctx_out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
    (void)hipGetLastError();
    return AMCX_ENODEV;
  }
  DeviceGuard guard;
  AMCX_HIP(guard.enter(device));
  amcx_ctx* c = new (std::nothrow) amcx_ctx();
  if (c == nullptr) return AMCX_ENOMEM;
  c->device = device;
  hipError_t e = c->stream.create();
  if (e != hipSuccess) { delete c; return hip_fail(e, "hipStreamCreateWithFlags"); }
  // Warm the runtime HERE, under the creating thread's own affinity mask: the first pinned allocation and the first
  // copy on a stream may start HIP / HSA helper threads, and a thread inherits its creator's mask for good.  Left to the
  // first upload they would be started inside its AffinityGuard window (ctx_run_strided narrows the calling thread to
  // the device's socket for the duration of a threaded upload) and stay on those CPUs.  Best effort: a failure here
  // surfaces where the real allocation is made.
  {
    PinnedBuffer warm_pin;
    DeviceBuffer warm_dev;
    if (warm_pin.reserve(4096) == AMCX_OK && warm_dev.reserve(4096) == AMCX_OK) {
      memset(warm_pin.p, 0, 4096);
      if (hipMemcpyAsync(warm_dev.p, warm_pin.p, 4096, hipMemcpyHostToDevice, c->stream) == hipSuccess)
        (void)hipStreamSynchronize(c->stream);
    }
    (void)hipGetLastError();
  }
  // which CPUs are local to this device: from the kernel's PCI tree, unless AMCX_NUMA=0 (AMCX_SYSFS_ROOT: another tree)
  if (hipDeviceGetPCIBusId(c->pci_bus_id, (int)sizeof c->pci_bus_id, device) != hipSuccess) {
    (void)hipGetLastError();
    c->pci_bus_id[0] = '\0';
  }
  const char* numa_env = getenv("AMCX_NUMA");
  if (c->pci_bus_id[0] != '\0' && !(numa_env != nullptr && numa_env[0] == '0')) {
    const char* root = getenv("AMCX_SYSFS_ROOT");
    const amcx::NumaPlace place = amcx::numa_place_of(root != nullptr && root[0] != '\0' ? root : "/sys", c->pci_bus_id);
    if (!place.empty()) {
      c->numa_node = place.node;
      c->bind_cpus = place.cpus;
      c->pool.set_cpus(c->bind_cpus);
    }
  }
  *ctx_out = c;
  return AMCX_OK;
}

int amcx_ctx_bind_cpus(amcx_ctx* ctx, const int32_t* cpus, int32_t n_cpus) {
  if (ctx == nullptr || n_cpus < 0 || (n_cpus > 0 && cpus == nullptr)) return AMCX_EINVAL;
  std::vector<int> v;
  for (int32_t i = 0; i < n_cpus; ++i) {
    if (cpus[i] < 0 || cpus[i] >= CPU_SETSIZE) return AMCX_EINVAL;
    v.push_back((int)cpus[i]);
  }
  // not while an upload runs on this context: its staging threads are reading the list this call replaces
  const amcx::CallGate::Token idle = ctx->gate.claim_idle();
  if (!idle) return AMCX_EINVAL;
  ctx->bind_cpus = v;
  if (v.empty()) ctx->numa_node = -1;
  ctx->pool.set_cpus(ctx->bind_cpus);
  return AMCX_OK;
}

int amcx_ctx_set_feature_mask(amcx_ctx* ctx, uint32_t feature_mask) {
  if (ctx == nullptr || !valid_feature_mask(feature_mask)) return AMCX_EINVAL;
  const amcx::CallGate::Token idle = ctx->gate.claim_idle();     // fails while a call is running on the context
  if (!idle) return AMCX_EINVAL;
  ctx->feature_mask.store(feature_mask, std::memory_order_release);
  return AMCX_OK;
}

int amcx_ctx_set_iq8_scale(amcx_ctx* ctx, float scale) {
  if (ctx == nullptr || !int_scale_ok(scale)) return AMCX_EINVAL;
  const amcx::CallGate::Token idle = ctx->gate.claim_idle();
  if (!idle) return AMCX_EINVAL;
  ctx->iq8_scale.store(scale, std::memory_order_release);
  return AMCX_OK;
}

int amcx_ctx_set_sc16_scale(amcx_ctx* ctx, float scale) {
  if (ctx == nullptr || !int_scale_ok(scale)) return AMCX_EINVAL;
  const amcx::CallGate::Token idle = ctx->gate.claim_idle();
  if (!idle) return AMCX_EINVAL;
  ctx->sc16_scale.store(scale, std::memory_order_release);
  return AMCX_OK;
}

int amcx_ctx_placement(const amcx_ctx* ctx, amcx_placement* out) {
  if (ctx == nullptr || out == nullptr) return AMCX_EINVAL;
  memset(out, 0, sizeof *out);
  out->device = ctx->device;
  out->numa_node = ctx->numa_node;
  out->n_cpus = (int32_t)ctx->bind_cpus.size();
  out->n_cpus_allowed = (int32_t)amcx::allowed_subset(ctx->bind_cpus).size();
  out->first_cpu = ctx->bind_cpus.empty() ? -1 : ctx->bind_cpus.front();
  out->last_cpu = ctx->bind_cpus.empty() ? -1 : ctx->bind_cpus.back();
  snprintf(out->pci_bus_id, sizeof out->pci_bus_id, "%s", ctx->pci_bus_id);
  return AMCX_OK;
}

int amcx_device_pci_bus_id(int32_t device, char* buf, int32_t buf_len) {
  if (buf == nullptr || buf_len < 16) return AMCX_EINVAL;
  buf[0] = '\0';
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
    (void)hipGetLastError();
    return AMCX_ENODEV;
  }
  AMCX_HIP(hipDeviceGetPCIBusId(buf, buf_len, device));
  for (char* p = buf; *p; ++p) *p = (char)tolower((unsigned char)*p);
  return AMCX_OK;
}

int amcx_numa_place(const char* sysfs_root, const char* pci_bus_id, int32_t* node_out, int32_t* cpus_out,
                    int32_t cpus_cap, int32_t* n_cpus_out) {
  if (pci_bus_id == nullptr || node_out == nullptr || n_cpus_out == nullptr || cpus_cap < 0 ||
      (cpus_cap > 0 && cpus_out == nullptr))
    return AMCX_EINVAL;
  const amcx::NumaPlace place = amcx::numa_place_of(sysfs_root != nullptr && sysfs_root[0] != '\0' ? sysfs_root : "/sys", pci_bus_id);
  *node_out = place.empty() ? -1 : place.node;
  *n_cpus_out = place.empty() ? 0 : (int32_t)place.cpus.size();
  for (int32_t i = 0; i < *n_cpus_out && i < cpus_cap; ++i) cpus_out[i] = place.cpus[(size_t)i];
  return AMCX_OK;
}

int amcx_ctx_destroy(amcx_ctx* c) {
  if (c == nullptr) return AMCX_OK;
  DeviceGuard guard;
  (void)guard.enter(c->device);
  for (hipStream_t s : {c->stream.s, c->copy_stream.s}) if (s != nullptr) (void)hipStreamSynchronize(s);
  delete c;                                     // every member frees itself (amcx_ctx, MEMBER ORDER); joins the staging threads
  return AMCX_OK;
}

int amcx_ctx_features18_strided_host(amcx_ctx* ctx, const void* re, const void* im, int32_t kind,
                                     int64_t n_snr, int64_t n_frames, int32_t frame_size,
                                     int64_t stride_snr, int64_t stride_frame, int64_t stride_sample,
                                     float* out_host, int64_t out_row_stride, int32_t variant) {
  return ctx_run_strided(ctx, amcx::Source::memory(re, im, kind), n_snr, n_frames, frame_size, stride_snr, stride_frame, stride_sample,
                         out_host, out_row_stride, variant);
}

int amcx_ctx_features18_strided_file(amcx_ctx* ctx, int32_t fd, int64_t re_offset, int64_t im_offset, int32_t kind,
                                     int64_t n_snr, int64_t n_frames, int32_t frame_size,
                                     int64_t stride_snr, int64_t stride_frame, int64_t stride_sample,
                                     float* out_host, int64_t out_row_stride, int32_t variant) {
  if (fd < 0 || re_offset < 0) return AMCX_EINVAL;
  return ctx_run_strided(ctx, amcx::Source::file(fd, re_offset, im_offset, kind), n_snr, n_frames, frame_size, stride_snr, stride_frame, stride_sample,
                         out_host, out_row_stride, variant);
}

int amcx_stage_host(const void* re, const void* im, int32_t kind, int64_t n_snr, int64_t n_frames,
                    int32_t frame_size, int64_t stride_snr, int64_t stride_frame, int64_t stride_sample,
                    int64_t first_unit, int64_t n_units, void* dst, int64_t dst_bytes, int32_t threads,
                    int32_t* plane_major, int32_t* inner_snr_out) {
  return stage_any(amcx::Source::memory(re, im, kind), n_snr, n_frames, frame_size, stride_snr, stride_frame, stride_sample, first_unit, n_units, dst,
                   dst_bytes, threads, plane_major, inner_snr_out);
}

int amcx_stage_file(int32_t fd, int64_t re_offset, int64_t im_offset, int32_t kind, int64_t n_snr, int64_t n_frames,
                    int32_t frame_size, int64_t stride_snr, int64_t stride_frame, int64_t stride_sample,
                    int64_t first_unit, int64_t n_units, void* dst, int64_t dst_bytes, int32_t threads,
                    int32_t* plane_major, int32_t* inner_snr_out) {
  if (fd < 0 || re_offset < 0) return AMCX_EINVAL;
  return stage_any(amcx::Source::file(fd, re_offset, im_offset, kind), n_snr, n_frames, frame_size, stride_snr, stride_frame, stride_sample, first_unit, n_units, dst,
                   dst_bytes, threads, plane_major, inner_snr_out);
}

int amcx_ctx_configure(amcx_ctx* ctx, int32_t threads, int64_t slot_bytes, int32_t round_on_device) {
  if (ctx == nullptr || threads < 0 || threads > 256 || slot_bytes < 0) return AMCX_EINVAL;
  if (threads > 0) ctx->threads = threads;
  if (slot_bytes > 0) ctx->slot_bytes = (size_t)slot_bytes < 4096 ? 4096 : (size_t)slot_bytes;
  if (round_on_device >= 0) ctx->round_on_device = round_on_device != 0;
  return AMCX_OK;
}

int amcx_ctx_upload_stats(const amcx_ctx* ctx, amcx_upload_stats* out) {
  if (ctx == nullptr || out == nullptr) return AMCX_EINVAL;
  *out = ctx->stats;
  return AMCX_OK;
}

int amcx_pack_planes_c64(const void* slab_dev, int32_t src_kind, int32_t n_planes, int64_t plane_stride,
                         int64_t n_snr, int64_t n_frames, int32_t inner_snr, void* frames_dev,
                         int64_t row_stride_elems, int32_t n0, void* hip_stream) {
  if (n_planes < 0 || n_snr < 0 || n_frames < 0 || n0 < 0 || (src_kind != AMCX_SRC_C64 && src_kind != AMCX_SRC_C128))
    return AMCX_EINVAL;
  if (n_snr > 0x7fffffffLL || (n_frames > 0 && n_snr > (int64_t(1) << 40) / n_frames)) return AMCX_EINVAL;
  const int64_t P = n_snr * n_frames;
  if (plane_stride < P || row_stride_elems < (int64_t)n0 + n_planes) return AMCX_EINVAL;
  if (n_planes == 0 || P == 0) return AMCX_OK;
  if (slab_dev == nullptr || frames_dev == nullptr) return AMCX_EINVAL;
  if (on_another_device(slab_dev) || on_another_device(frames_dev)) return AMCX_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  float2* dst = static_cast<float2*>(frames_dev);
  hipError_t e = src_kind == AMCX_SRC_C128
      ? amcx::launch_pack_planes(static_cast<const double2*>(slab_dev), n_planes, P, plane_stride, (int)n_snr, n_frames,
                                 inner_snr, dst, row_stride_elems, n0, stream)
      : amcx::launch_pack_planes(static_cast<const float2*>(slab_dev), n_planes, P, plane_stride, (int)n_snr, n_frames,
                                 inner_snr, dst, row_stride_elems, n0, stream);
  if (e != hipSuccess) return hip_fail(e, "amcx_pack_planes_c64");
  return AMCX_OK;
}

int amcx_ctx_features18_c64_host(amcx_ctx* ctx, const void* iq_host, int64_t n_frames, int32_t frame_size,
                                 int64_t row_stride_elems, float* out_host, int64_t out_row_stride,
                                 int32_t variant) {
  return ctx_run(ctx, iq_host, AMCX_SRC_C64, n_frames, frame_size, row_stride_elems, out_host, out_row_stride, variant);
}

int amcx_ctx_features18_sc16_host(amcx_ctx* ctx, const void* iq_host, int64_t n_frames, int32_t frame_size,
                                  int64_t row_stride_samples, float* out_host, int64_t out_row_stride,
                                  int32_t variant) {
  return ctx_run(ctx, iq_host, AMCX_SRC_SC16, n_frames, frame_size, row_stride_samples, out_host, out_row_stride, variant);
}

int amcx_ctx_features18_iq8_host(amcx_ctx* ctx, const void* iq_host, int64_t n_frames, int32_t frame_size,
                                 int64_t row_stride_samples, int32_t format, float* out_host, int64_t out_row_stride,
                                 int32_t variant) {
  if (!iq8_format_ok(format)) return AMCX_EINVAL;
  return ctx_run(ctx, iq_host, format == AMCX_IQ8_CU8 ? AMCX_SRC_CU8 : AMCX_SRC_CI8, n_frames, frame_size, row_stride_samples,
                 out_host, out_row_stride, variant);
}

int amcx_ctx_features18_c128_host(amcx_ctx* ctx, const void* iq_host, int64_t n_frames, int32_t frame_size,
                                  int64_t row_stride_elems, float* out_host, int64_t out_row_stride,
                                  int32_t variant) {
  return ctx_run(ctx, iq_host, AMCX_SRC_C128, n_frames, frame_size, row_stride_elems, out_host, out_row_stride, variant);
}

int amcx_features18_c64_host(const void* iq_host, int64_t n_frames, int32_t frame_size,
                             int64_t row_stride_elems, float* out_host, int64_t out_row_stride,
                             int32_t device, int32_t variant) {
  return one_shot(iq_host, false, n_frames, frame_size, row_stride_elems, out_host, out_row_stride, device, variant);
}

int amcx_features18_c128_host(const void* iq_host, int64_t n_frames, int32_t frame_size,
                              int64_t row_stride_elems, float* out_host, int64_t out_row_stride,
                              int32_t device, int32_t variant) {
  return one_shot(iq_host, true, n_frames, frame_size, row_stride_elems, out_host, out_row_stride, device, variant);
}

int amcx_kernel_name(int32_t frame_size, int32_t variant, char* buf, int32_t buf_len) {
  if (buf == nullptr || buf_len <= 0) return AMCX_EINVAL;
  const int v = resolve_variant(frame_size, variant);
  if (v < 0) return v;
  if (v == AMCX_VARIANT_WAVE) {
    amcx::wave_kernel_name(frame_size, amcx::kPlanAll, buf, (size_t)buf_len);
    return AMCX_OK;
  }
  const char* name = frame_size > amcx::kBlockMaxN                   ? "amcx_features18_stream_kernel"     /* <true> with a workspace, <false> without */
                     : block_mode(frame_size) == amcx::kBlockPow2      ? "amcx_features18_block_kernel<1>"
                     : block_mode(frame_size) == amcx::kBlockBluestein ? "amcx_features18_block_kernel<2>"
                     : block_mode(frame_size) == amcx::kBlockBluesteinBig ? "amcx_features18_block_kernel<3>"
                                                                       : "amcx_features18_block_kernel<0>";
  snprintf(buf, (size_t)buf_len, "%s", name);
  return AMCX_OK;
}

int amcx_kernel_name_subset(int32_t frame_size, int32_t variant, uint32_t feature_mask, char* buf, int32_t buf_len) {
  if (buf == nullptr || buf_len <= 0 || !valid_feature_mask(feature_mask)) return AMCX_EINVAL;
  const int v = resolve_variant(frame_size, variant);
  if (v < 0) return v;
  const int plan = subset_plan(frame_size, v, feature_mask);
  if (plan == amcx::kPlanAll) return amcx_kernel_name(frame_size, variant, buf, buf_len);
  amcx::wave_kernel_name(frame_size, plan, buf, (size_t)buf_len);
  return AMCX_OK;
}

int amcx_kernel_name_sc16(int32_t frame_size, int32_t variant, uint32_t feature_mask, char* buf, int32_t buf_len) {
  if (buf == nullptr || buf_len <= 0 || !valid_feature_mask(feature_mask)) return AMCX_EINVAL;
  const int v = resolve_variant(frame_size, variant);
  if (v < 0) return v;
  if (!sc16_typed(frame_size, v))     // widened, then the complex64 kernel
    return amcx_kernel_name_subset(frame_size, variant, feature_mask, buf, buf_len);
  amcx::wave_kernel_name(frame_size, subset_plan(frame_size, v, feature_mask), buf, (size_t)buf_len, true);
  return AMCX_OK;
}

int amcx_kernel_name_iq8(int32_t frame_size, int32_t variant, uint32_t feature_mask, char* buf, int32_t buf_len) {
  return amcx_kernel_name_sc16(frame_size, variant, feature_mask, buf, buf_len);     // widened to what that kernel reads
}

// ---- the digital down-converter (amcx_ddc_kernel.h) ------------------------------------------------------------------
int64_t amcx_tune_decimate_out_samples(int64_t n_samples, int32_t n_taps, int32_t decim) {
  if (n_taps < 1 || n_taps > amcx::kDdcMaxTaps || decim < 1 || decim > amcx::kDdcMaxDecim) return -1;
  if (n_samples < 0 || n_samples >= (int64_t(1) << 40)) return -1;
  return n_samples < n_taps ? 0 : (n_samples - n_taps) / decim + 1;
}

int amcx_tune_decimate_plan(int32_t n_taps, int32_t decim, int32_t* tile_outputs, int32_t* max_workgroups) {
  if (amcx_tune_decimate_out_samples(0, n_taps, decim) < 0) return AMCX_EINVAL;
  if (tile_outputs != nullptr) *tile_outputs = amcx::ddc_tile_outputs(n_taps, decim);
  if (max_workgroups != nullptr) *max_workgroups = cu_count() * ddc_wgs_per_cu(n_taps, decim);
  return AMCX_OK;
}

int amcx_tune_decimate(const void* src_dev, int32_t src_kind, int64_t n_samples, float scale, uint64_t phase0,
                       uint64_t phase_step, const float* taps_dev, int32_t n_taps, int32_t decim, void* out_c64_dev,
                       int64_t out_capacity_samples, void* hip_stream) {
  const StreamSrc src{src_kind};
  if (!src.ok(scale)) return AMCX_EINVAL;
  const int64_t M = amcx_tune_decimate_out_samples(n_samples, n_taps, decim);
  if (M < 0 || out_capacity_samples < M) return AMCX_EINVAL;
  if (M == 0) return AMCX_OK;
  if (!stream_ptrs_ok(src_dev, taps_dev, out_c64_dev, src)) return AMCX_EINVAL;
  const int tile = amcx::ddc_tile_outputs(n_taps, decim);
  const int64_t n_tiles = (M + tile - 1) / tile;
  const int64_t grid = amcx::persistent_grid(cu_count(), ddc_wgs_per_cu(n_taps, decim), n_tiles, 1);
  const hipError_t e = amcx::launch(ddc_kernel(src).kern, grid, amcx::kDdcThreads, amcx::ddc_lds_bytes(n_taps, decim),
                                    static_cast<hipStream_t>(hip_stream), static_cast<const char*>(src_dev), src.kernel_scale(scale),
                                    src.flip4(), (unsigned long long)phase0, (unsigned long long)phase_step, taps_dev, n_taps, decim,
                                    static_cast<float2*>(out_c64_dev), (long long)M, tile, (long long)n_tiles);
  if (e != hipSuccess) return hip_fail(e, "down-converter kernel launch");
  return AMCX_OK;
}

int amcx_kernel_name_ddc(int32_t src_kind, char* buf, int32_t buf_len) {
  return put_kernel_name(ddc_kernel({src_kind}).name, buf, buf_len);
}

// ---- the polyphase filter bank (amcx_bank_kernel.h) -------------------------------------------------------------------
int64_t amcx_filter_bank_out_samples(int64_t n_samples, int32_t n_taps, int32_t channels, int32_t decim) {
  if (channels < 2 || channels > amcx::kBankMaxChannels || (channels & (channels - 1)) != 0) return -1;
  if (n_taps < 1 || n_taps > amcx::kBankMaxTaps || decim < 1 || decim > channels) return -1;
  if (n_samples < 0 || n_samples >= (int64_t(1) << 40)) return -1;
  return n_samples < n_taps ? 0 : (n_samples - n_taps) / decim + 1;
}

int amcx_filter_bank_plan(int32_t n_taps, int32_t channels, int32_t decim, int32_t* tile_outputs, int32_t* max_workgroups,
                          int32_t* lds_bytes) {
  if (amcx_filter_bank_out_samples(0, n_taps, channels, decim) < 0) return AMCX_EINVAL;
  if (tile_outputs != nullptr) *tile_outputs = amcx::bank_tile_outputs(channels);
  if (max_workgroups != nullptr) *max_workgroups = cu_count() * bank_wgs_per_cu(n_taps, channels, decim);
  if (lds_bytes != nullptr) *lds_bytes = (int32_t)amcx::bank_lds_bytes(n_taps, channels, decim);
  return AMCX_OK;
}

int amcx_filter_bank(const void* src_dev, int32_t src_kind, int64_t n_samples, float scale, uint64_t phase0,
                     uint64_t phase_step, uint64_t sample_index0, const float* taps_dev, int32_t n_taps, int32_t channels,
                     int32_t decim, void* out_c64_dev, int64_t out_channel_stride, int64_t out_capacity_samples,
                     void* hip_stream) {
  const StreamSrc src{src_kind};
  if (!src.ok(scale)) return AMCX_EINVAL;
  const int64_t M = amcx_filter_bank_out_samples(n_samples, n_taps, channels, decim);
  if (M < 0) return AMCX_EINVAL;
  if (out_channel_stride < M || out_channel_stride > (INT64_MAX - M) / (channels - 1)) return AMCX_EINVAL;
  if (out_capacity_samples < (int64_t)(channels - 1) * out_channel_stride + M) return AMCX_EINVAL;
  if (M == 0) return AMCX_OK;
  if (!stream_ptrs_ok(src_dev, taps_dev, out_c64_dev, src)) return AMCX_EINVAL;
  const int tile = amcx::bank_tile_outputs(channels);
  const int64_t n_tiles = (M + tile - 1) / tile;
  const int64_t grid = amcx::persistent_grid(cu_count(), bank_wgs_per_cu(n_taps, channels, decim), n_tiles, 1);
  const int a0 = (int)(sample_index0 & (uint64_t)(channels - 1));
  const auto k = bank_kernel(src);
  // the most a bank kernel ever asks for: C = 2 (tile 2048), T = 4096, D = 2
  if (const hipError_t e = k.lds_attr((int)amcx::bank_lds_bytes(amcx::kBankMaxTaps, 2, 2)); e != hipSuccess)
    return hip_fail(e, "filter-bank kernel attribute");
  const hipError_t e = amcx::launch(k.kern, grid, amcx::kBankThreads, amcx::bank_lds_bytes(n_taps, channels, decim),
                                    static_cast<hipStream_t>(hip_stream), static_cast<const char*>(src_dev), src.kernel_scale(scale),
                                    src.flip4(), (unsigned long long)phase0, (unsigned long long)phase_step, a0, taps_dev, n_taps,
                                    log2_exact(channels), decim, static_cast<float2*>(out_c64_dev), (long long)out_channel_stride,
                                    (long long)M, tile, (long long)n_tiles);
  if (e != hipSuccess) return hip_fail(e, "filter-bank kernel launch");
  return AMCX_OK;
}

int amcx_kernel_name_bank(int32_t src_kind, char* buf, int32_t buf_len) {
  return put_kernel_name(bank_kernel({src_kind}).name, buf, buf_len);
}

// ---- the rational resampler (amcx_resample_kernel.h) --------------------------------------------------------------------
int64_t amcx_resample_out_samples(int64_t n_samples, int32_t n_taps, int32_t interp, int32_t decim, int32_t phase_index0) {
  if (n_taps < 1 || n_taps > amcx::kRsMaxTaps || interp < 1 || interp > amcx::kRsMaxInterp || decim < 1 ||
      decim > amcx::kRsMaxDecim)
    return -1;
  if (phase_index0 < 0 || phase_index0 >= interp) return -1;
  if (n_samples < 0 || n_samples >= (int64_t(1) << 40)) return -1;
  const int64_t P = amcx::poly_phase_taps(n_taps, interp);
  if (n_samples < P) return 0;
  const int64_t last = (n_samples - P + 1) * interp - 1 - phase_index0;      // the largest t with n(t) <= n_samples - 1, less tau0
  return last < 0 ? 0 : last / decim + 1;
}

int amcx_resample_plan(int32_t n_taps, int32_t interp, int32_t decim, int32_t* tile_outputs, int32_t* max_span_samples,
                       int32_t* max_workgroups, int32_t* lds_bytes) {
  if (amcx_resample_out_samples(0, n_taps, interp, decim, 0) < 0) return AMCX_EINVAL;
  if (tile_outputs != nullptr) *tile_outputs = amcx::rs_tile_outputs(n_taps, interp, decim);
  if (max_span_samples != nullptr) *max_span_samples = amcx::rs_max_span(n_taps, interp, decim);
  if (max_workgroups != nullptr) *max_workgroups = cu_count() * rs_wgs_per_cu(n_taps, interp, decim);
  if (lds_bytes != nullptr) *lds_bytes = (int32_t)amcx::rs_lds_bytes(n_taps, interp, decim);
  return AMCX_OK;
}

int amcx_resample(const void* src_dev, int32_t src_kind, int64_t n_samples, float scale, uint64_t phase0, uint64_t phase_step,
                  const float* taps_dev, int32_t n_taps, int32_t interp, int32_t decim, int32_t phase_index0,
                  void* out_c64_dev, int64_t out_capacity_samples, void* hip_stream) {
  const StreamSrc src{src_kind};
  if (!src.ok(scale)) return AMCX_EINVAL;
  const int64_t M = amcx_resample_out_samples(n_samples, n_taps, interp, decim, phase_index0);
  if (M < 0 || out_capacity_samples < M) return AMCX_EINVAL;
  if (M == 0) return AMCX_OK;
  if (!stream_ptrs_ok(src_dev, taps_dev, out_c64_dev, src)) return AMCX_EINVAL;
  const int tile = amcx::rs_tile_outputs(n_taps, interp, decim);
  const int64_t n_tiles = (M + tile - 1) / tile;
  const int64_t grid = amcx::persistent_grid(cu_count(), rs_wgs_per_cu(n_taps, interp, decim), n_tiles, 1);
  const hipError_t e = amcx::launch(rs_kernel(src).kern, grid, amcx::kRsThreads, amcx::rs_lds_bytes(n_taps, interp, decim),
                                    static_cast<hipStream_t>(hip_stream), static_cast<const char*>(src_dev), src.kernel_scale(scale),
                                    src.flip4(), (unsigned long long)phase0, (unsigned long long)phase_step, taps_dev, n_taps, interp,
                                    decim, phase_index0, amcx::poly_phase_taps(n_taps, interp),
                                    amcx::rs_max_span(n_taps, interp, decim), static_cast<float2*>(out_c64_dev), (long long)M,
                                    tile, (long long)n_tiles);
  if (e != hipSuccess) return hip_fail(e, "resampler kernel launch");
  return AMCX_OK;
}

const char* amcx_kernel_name_resample(int32_t src_kind) { return rs_kernel({src_kind}).name; }

// ---- occupancy detection (amcx_occupancy_kernels.h) ----------------------------------------------------------------------
namespace {
bool occ_grid_ok(int32_t channels, int64_t n_frames) {
  return channels >= 2 && channels <= amcx::kOccMaxChannels && n_frames >= 0 && n_frames < (int64_t(1) << 31) &&
         (int64_t)channels * n_frames < (int64_t(1) << 31);
}
int64_t occ_blocks(int64_t n_cells) { return (n_cells + amcx::kOccBlockRows - 1) / amcx::kOccBlockRows; }
}  // namespace

int amcx_row_power_c64(const void* rows_dev, int64_t n_rows, int32_t row_samples, int64_t row_stride_samples, float* power_dev,
                       void* hip_stream) {
  if (row_samples < 2 || row_samples > AMCX_MAX_FRAME_SIZE || !rows_ok(n_rows, row_stride_samples, row_samples)) return AMCX_EINVAL;
  if (n_rows == 0) return AMCX_OK;
  if (!ptrs_ok({{rows_dev, 7u, true}, {power_dev, 3u, true}})) return AMCX_EINVAL;
  const int64_t grid = amcx::persistent_grid(cu_count(), 8, n_rows, amcx::kOccWaves);
  const hipError_t e = amcx::launch(amcx::amcx_row_power_kernel, grid, amcx::kOccThreads, 0, static_cast<hipStream_t>(hip_stream),
                                    static_cast<const float2*>(rows_dev), (long long)n_rows, row_samples,
                                    (long long)row_stride_samples, power_dev);
  if (e != hipSuccess) return hip_fail(e, "row-power kernel launch");
  return AMCX_OK;
}

int64_t amcx_occupancy_workspace_bytes(int32_t channels, int64_t n_frames) {
  if (!occ_grid_ok(channels, n_frames)) return -1;
  return (occ_blocks((int64_t)channels * n_frames) * (int64_t)sizeof(int32_t) + 255) / 256 * 256;
}

int amcx_occupancy_detect_f32(const float* power_dev, int32_t channels, int64_t n_frames, int32_t floor_rank, float threshold,
                              float* floor_dev, uint8_t* mask_dev, int32_t* rows_dev, int32_t* count_dev, void* workspace_dev,
                              int64_t workspace_bytes, void* hip_stream) {
  if (!occ_grid_ok(channels, n_frames) || floor_rank < 0 || floor_rank >= channels) return AMCX_EINVAL;
  if (!threshold_ok(threshold)) return AMCX_EINVAL;
  const bool counted = rows_dev != nullptr || count_dev != nullptr;
  if (counted && workspace_bytes < amcx_occupancy_workspace_bytes(channels, n_frames)) return AMCX_EINVAL;
  if (n_frames == 0) return AMCX_OK;
  if (!ptrs_ok({{power_dev, 3u, true}, {floor_dev, 3u, true}, {mask_dev, 0u, false}, {rows_dev, 3u, false},
                {count_dev, 3u, rows_dev != nullptr}, {workspace_dev, 3u, counted}}))
    return AMCX_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const int cus = cu_count();
  const int64_t n_cells = (int64_t)channels * n_frames, n_blocks = occ_blocks(n_cells);
  const int64_t n_tiles = (n_frames + amcx::kOccTileFrames - 1) / amcx::kOccTileFrames;
  const size_t lds = amcx::occ_detect_lds_bytes(channels);         // 67 584 bytes at C = 256: the attribute, once
  hipError_t e = amcx::lds_attr_once<amcx::amcx_occupancy_detect_kernel>((int)amcx::occ_detect_lds_bytes(amcx::kOccMaxChannels));
  if (e != hipSuccess) return hip_fail(e, "occupancy floor kernel attribute");
  e = amcx::launch(amcx::amcx_occupancy_detect_kernel, amcx::persistent_grid(cus, wgs_per_cu(lds, 4), n_tiles, 1), amcx::kOccThreads,
                   lds, st, power_dev, channels, (long long)n_frames, floor_rank, floor_dev, (long long)n_tiles);
  if (e != hipSuccess) return hip_fail(e, "occupancy floor kernel launch");
  if (!counted && mask_dev == nullptr) return AMCX_OK;
  const int64_t grid = amcx::persistent_grid(cus, 4, n_blocks, 1);
  int* const counts = counted ? static_cast<int*>(workspace_dev) : nullptr;
  e = amcx::launch(amcx::amcx_occupancy_count_kernel, grid, amcx::kOccThreads, 0, st, power_dev, floor_dev, (unsigned)n_frames,
                   (long long)n_cells, threshold, mask_dev, counts, (long long)n_blocks);
  if (e != hipSuccess) return hip_fail(e, "occupancy count kernel launch");
  if (!counted) return AMCX_OK;
  e = amcx::launch(amcx::amcx_occupancy_scan_kernel, 1, amcx::kOccThreads, 0, st, counts, (long long)n_blocks, count_dev);
  if (e != hipSuccess) return hip_fail(e, "occupancy scan kernel launch");
  if (rows_dev == nullptr) return AMCX_OK;
  e = amcx::launch(amcx::amcx_occupancy_scatter_kernel, grid, amcx::kOccThreads, 0, st, power_dev, floor_dev, (unsigned)n_frames,
                   (long long)n_cells, threshold, counts, rows_dev, (long long)n_blocks);
  if (e != hipSuccess) return hip_fail(e, "occupancy scatter kernel launch");
  return AMCX_OK;
}

int amcx_gather_rows_c64(const void* src_dev, int64_t n_src_rows, int32_t row_samples, int64_t row_stride_samples,
                         const int32_t* index_dev, int64_t n_index, void* dst_dev, int64_t dst_stride_samples, void* hip_stream) {
  if (row_samples < 2 || row_samples > AMCX_MAX_FRAME_SIZE) return AMCX_EINVAL;
  if (!rows_ok(n_src_rows, row_stride_samples, row_samples) || !rows_ok(n_index, dst_stride_samples, row_samples)) return AMCX_EINVAL;
  if (n_index == 0) return AMCX_OK;
  if (!ptrs_ok({{src_dev, 7u, n_src_rows > 0}, {index_dev, 3u, true}, {dst_dev, 7u, true}})) return AMCX_EINVAL;
  const int64_t grid = amcx::persistent_grid(cu_count(), 8, n_index, amcx::kOccWaves);
  const hipError_t e = amcx::launch(amcx::amcx_gather_rows_kernel, grid, amcx::kOccThreads, 0, static_cast<hipStream_t>(hip_stream),
                                    static_cast<const float2*>(src_dev), (long long)n_src_rows, row_samples,
                                    (long long)row_stride_samples, index_dev, (long long)n_index, static_cast<float2*>(dst_dev),
                                    (long long)dst_stride_samples);
  if (e != hipSuccess) return hip_fail(e, "row-gather kernel launch");
  return AMCX_OK;
}

const char* amcx_kernel_name_occupancy(int32_t which) {
  switch (which) {
    case 0: return "amcx_row_power_kernel";
    case 1: return "amcx_occupancy_detect_kernel";
    case 2: return "amcx_gather_rows_kernel";
    case 3: return "amcx_occupancy_count_kernel";
    case 4: return "amcx_occupancy_scan_kernel";
    case 5: return "amcx_occupancy_scatter_kernel";
    default: return nullptr;
  }
}

// ---- the spectrogram and its detection (amcx_psd_kernel.h) ----------------------------------------------------------------
int64_t amcx_spectrogram_out_rows(int64_t n_samples, int32_t nfft, int32_t hop, int32_t averages) {
  if (psd_log2(nfft) < 0 || hop < 1 || hop > amcx::kPsdMaxHop || averages < 1 || averages > amcx::kPsdMaxAverages) return -1;
  if (n_samples < 0 || n_samples >= (int64_t(1) << 40)) return -1;
  if (n_samples < nfft) return 0;
  return ((n_samples - nfft) / hop + 1) / averages;
}

int amcx_spectrogram_plan(int32_t nfft, int32_t hop, int32_t averages, int32_t* segments_per_pass, int32_t* lds_bytes,
                          int32_t* max_workgroups) {
  if (amcx_spectrogram_out_rows(0, nfft, hop, averages) < 0) return AMCX_EINVAL;
  if (segments_per_pass != nullptr) *segments_per_pass = amcx::kPsdPoints / nfft;
  if (lds_bytes != nullptr) *lds_bytes = amcx::kPsdLdsBytes;
  if (max_workgroups != nullptr) *max_workgroups = cu_count() * wgs_per_cu(amcx::kPsdLdsBytes, 8);
  return AMCX_OK;
}

int amcx_spectrogram(const void* src_dev, int32_t src_kind, int64_t n_samples, float scale, const float* window_dev, int32_t nfft,
                     int32_t hop, int32_t averages, float* psd_dev, int64_t row_stride, int64_t n_rows, void* hip_stream) {
  const StreamSrc src{src_kind};
  if (!src.ok(scale)) return AMCX_EINVAL;
  const int64_t R = amcx_spectrogram_out_rows(n_samples, nfft, hop, averages);
  if (R < 0 || n_rows > R || !rows_ok(n_rows, row_stride, nfft)) return AMCX_EINVAL;
  if (n_rows == 0) return AMCX_OK;
  if (!stream_ptrs_ok(src_dev, window_dev, psd_dev, src, 3u)) return AMCX_EINVAL;
  const int segs = amcx::kPsdPoints / nfft;
  const int64_t n_passes = (n_rows + segs - 1) / segs;
  const int64_t grid = amcx::persistent_grid(cu_count(), wgs_per_cu(amcx::kPsdLdsBytes, 8), n_passes, 1);
  const hipError_t e = amcx::launch(psd_kernel(src).kern, grid, amcx::kPsdThreads, 0, static_cast<hipStream_t>(hip_stream),
                                    static_cast<const char*>(src_dev), src.kernel_scale(scale), src.flip4(), window_dev, nfft,
                                    psd_log2(nfft), hop, averages, psd_dev, (long long)row_stride, (long long)n_rows,
                                    (long long)n_passes);
  if (e != hipSuccess) return hip_fail(e, "spectrogram kernel launch");
  return AMCX_OK;
}

int amcx_psd_detect_f32(const float* psd_dev, int64_t n_rows, int32_t bins, int64_t row_stride, int32_t floor_rank, float threshold,
                        float* floor_dev, uint8_t* mask_dev, void* hip_stream) {
  if (bins < 2 || bins > amcx::kPsdMaxBins || floor_rank < 0 || floor_rank >= bins || !threshold_ok(threshold)) return AMCX_EINVAL;
  if (!rows_ok(n_rows, row_stride, bins)) return AMCX_EINVAL;
  if (n_rows == 0) return AMCX_OK;
  if (!ptrs_ok({{psd_dev, 3u, true}, {floor_dev, 3u, true}, {mask_dev, 0u, false}})) return AMCX_EINVAL;
  const int64_t grid = amcx::persistent_grid(cu_count(), 8, n_rows, 1);
  const hipError_t e = amcx::launch(amcx::amcx_psd_detect_kernel, grid, amcx::kPsdThreads, 0, static_cast<hipStream_t>(hip_stream),
                                    psd_dev, (long long)n_rows, bins, (long long)row_stride, floor_rank, threshold, floor_dev,
                                    mask_dev);
  if (e != hipSuccess) return hip_fail(e, "spectrogram detection kernel launch");
  return AMCX_OK;
}

int amcx_kernel_name_psd(int32_t src_kind, char* buf, int32_t buf_len) {
  return put_kernel_name(psd_kernel({src_kind}).name, buf, buf_len);
}

const char* amcx_kernel_name_psd_detect(void) { return "amcx_psd_detect_kernel"; }

int64_t amcx_group_stats_workspace_bytes(int64_t n_groups, int64_t rows_per_group, int32_t n_cols) {
  if (!stats_args_ok(n_groups, rows_per_group, n_cols, n_cols)) return -1;
  if (n_groups == 0) return 0;
  int64_t chunks, rpc;
  stats_plan(n_groups, rows_per_group, n_cols, &chunks, &rpc);
  return n_groups * chunks * n_cols * 3 * (int64_t)sizeof(double);
}

int amcx_group_stats_ws_f32(const float* x_dev, int64_t n_groups, int64_t rows_per_group,
                            int64_t row_stride, int32_t n_cols, double* mean_dev, double* std_dev,
                            void* workspace_dev, int64_t workspace_bytes, void* hip_stream) {
  if (!stats_args_ok(n_groups, rows_per_group, row_stride, n_cols)) return AMCX_EINVAL;
  if (n_groups > 0 && workspace_bytes < amcx_group_stats_workspace_bytes(n_groups, rows_per_group, n_cols)) return AMCX_EINVAL;
  if (n_groups == 0) return AMCX_OK;
  if (!ptrs_ok({{x_dev, 3u, true}, {mean_dev, 7u, true}, {std_dev, 7u, true}, {workspace_dev, 7u, true}})) return AMCX_EINVAL;
  return launch_stats(x_dev, n_groups, rows_per_group, row_stride, n_cols, mean_dev, std_dev, workspace_dev,
                      static_cast<hipStream_t>(hip_stream));
}

int amcx_group_stats_f32(const float* x_dev, int64_t n_groups, int64_t rows_per_group,
                         int64_t row_stride, int32_t n_cols, double* mean_dev, double* std_dev,
                         void* hip_stream) {
  if (!stats_args_ok(n_groups, rows_per_group, row_stride, n_cols)) return AMCX_EINVAL;
  if (n_groups == 0) return AMCX_OK;
  if (!ptrs_ok({{x_dev, 3u, true}, {mean_dev, 7u, true}, {std_dev, 7u, true}})) return AMCX_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const int64_t bytes = amcx_group_stats_workspace_bytes(n_groups, rows_per_group, n_cols);
  void* ws = nullptr;
  AMCX_HIP(hipMallocAsync(&ws, (size_t)bytes, st));           // stream-ordered: no synchronisation
  return free_own_ws(ws, st, launch_stats(x_dev, n_groups, rows_per_group, row_stride, n_cols, mean_dev, std_dev, ws, st));
}

int64_t amcx_standardize_workspace_bytes(int64_t n_rows, int32_t n_cols) {
  if (n_rows < 1) return n_rows == 0 ? 0 : -1;
  const int64_t part = amcx_group_stats_workspace_bytes(1, n_rows, n_cols);
  return part < 0 ? -1 : part + 2 * (int64_t)amcx::kStatMaxCols * (int64_t)sizeof(double);
}

int amcx_standardize_fit_transform_f32(const float* x_dev, int64_t n_rows, int64_t row_stride,
                                       int32_t n_cols, const int32_t* cols_host, int32_t n_sel,
                                       float* out_dev, int64_t out_stride, double* mean_dev,
                                       double* scale_dev, void* workspace_dev, int64_t workspace_bytes,
                                       void* hip_stream) {
  if (n_sel < 1 || n_sel > amcx::kStatMaxCols || n_cols < 1 || n_cols > amcx::kStatMaxCols || cols_host == nullptr ||
      !rows_ok(n_rows, row_stride, n_cols) || !rows_ok(n_rows, out_stride, n_sel))
    return AMCX_EINVAL;
  amcx::SelectCols sel;
  if (!make_select_cols(cols_host, n_sel, n_cols, &sel)) return AMCX_EINVAL;
  // the statistics' own limits (row_stride <= 2^20) over the one group of n_rows rows, and the transform's grid in 31 bits
  const int64_t grid = (n_rows + amcx::kSelectRows - 1) / amcx::kSelectRows;
  if (n_rows > 0 && (!stats_args_ok(1, n_rows, row_stride, n_cols) || grid > 0x7fffffffLL)) return AMCX_EINVAL;
  if (n_rows > 0 && workspace_bytes < amcx_standardize_workspace_bytes(n_rows, n_cols)) return AMCX_EINVAL;
  if (n_rows == 0) return AMCX_OK;
  if (!ptrs_ok({{x_dev, 3u, true}, {out_dev, 3u, true}, {mean_dev, 7u, true}, {scale_dev, 7u, true}, {workspace_dev, 7u, true}}))
    return AMCX_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  double* all_mean = static_cast<double*>(workspace_dev);
  double* all_std = all_mean + amcx::kStatMaxCols;
  const int rc = launch_stats(x_dev, 1, n_rows, row_stride, n_cols, all_mean, all_std, all_std + amcx::kStatMaxCols, st);
  if (rc != AMCX_OK) return rc;
  const hipError_t e = amcx::launch(amcx::amcx_select_fit_scale_kernel, grid, amcx::kBlockThreads, 0, st, x_dev, n_rows, row_stride, sel,
                                    all_mean, all_std, out_dev, out_stride, mean_dev, scale_dev);
  if (e != hipSuccess) return hip_fail(e, "scaler fit-and-transform kernel launch");
  return AMCX_OK;
}

int amcx_select_scale_f32(const float* x_dev, int64_t n_rows, int64_t row_stride,
                          const int32_t* cols_dev, int32_t n_sel, const double* mean_dev,
                          const double* scale_dev, float* out_dev, int64_t out_stride,
                          void* hip_stream) {
  // (the input's width is not an argument: a row holds one element at least; n_rows * n_sel <= n_rows * out_stride <= 2^58)
  if (n_sel < 1 || !rows_ok(n_rows, row_stride, 1) || !rows_ok(n_rows, out_stride, n_sel)) return AMCX_EINVAL;
  if (n_rows == 0) return AMCX_OK;
  if (!ptrs_ok({{x_dev, 3u, true}, {cols_dev, 3u, true}, {mean_dev, 7u, true}, {scale_dev, 7u, true}, {out_dev, 3u, true}}))
    return AMCX_EINVAL;
  const int64_t grid = amcx::persistent_grid(cu_count(), 8, n_rows * n_sel, amcx::kBlockThreads);
  const hipError_t e = amcx::launch(amcx::amcx_select_scale_kernel, grid, amcx::kBlockThreads, 0, static_cast<hipStream_t>(hip_stream),
                                    x_dev, n_rows, row_stride, cols_dev, n_sel, mean_dev, scale_dev, out_dev, out_stride);
  if (e != hipSuccess) return hip_fail(e, "select-and-scale kernel launch");
  return AMCX_OK;
}

int64_t amcx_mlp_params_floats(const int32_t* widths_host, int32_t n_linear) {
  if (!mlp_shape_ok(widths_host, n_linear)) return -1;
  int64_t n = 0;
  for (int l = 0; l < n_linear; ++l) n += (int64_t)widths_host[l + 1] * widths_host[l] + widths_host[l + 1];
  return n;
}

int amcx_mlp_kernel_name(const int32_t* widths_host, int32_t n_linear, char* buf, int32_t buf_len) {
  if (buf == nullptr || buf_len <= 0 || !mlp_shape_ok(widths_host, n_linear)) return AMCX_EINVAL;
  snprintf(buf, (size_t)buf_len, "%s", "amcx_mlp_classify_kernel");      // one kernel: widths are run-time values
  return AMCX_OK;
}

int amcx_mlp_classify_f32(const float* x_dev, int64_t n_rows, int64_t row_stride, int32_t n_cols,
                          const int32_t* cols_host, int32_t n_sel, const double* mean_dev, const double* scale_dev,
                          const float* params_dev, const int32_t* widths_host, int32_t n_linear, int32_t activation,
                          int32_t* labels_dev, float* probs_dev, int64_t probs_stride, int64_t rows_per_group,
                          int64_t* counts_dev, void* hip_stream) {
  amcx::SelectCols sel;
  if (!mlp_rows_ok(n_rows, row_stride, n_cols, cols_host, n_sel, mean_dev, scale_dev, widths_host, n_linear, &sel)) return AMCX_EINVAL;
  if (activation != AMCX_ACT_RELU && activation != AMCX_ACT_TANH && activation != AMCX_ACT_SIGMOID) return AMCX_EINVAL;
  const int n_cls = widths_host[n_linear];
  if (!opt_rows_ok(probs_dev, n_rows, probs_stride, n_cls) || !groups_ok(n_rows, rows_per_group, counts_dev)) return AMCX_EINVAL;
  if (n_rows == 0) return AMCX_OK;
  if (!ptrs_ok({{x_dev, 3u, true}, {mean_dev, 7u, false}, {scale_dev, 7u, false}, {params_dev, 3u, true}, {labels_dev, 3u, false},
                {probs_dev, 3u, false}, {counts_dev, 7u, false}}))
    return AMCX_EINVAL;
  if (labels_dev == nullptr && probs_dev == nullptr && counts_dev == nullptr) return AMCX_OK;      // nothing asked for
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  unsigned long long* const counts = reinterpret_cast<unsigned long long*>(counts_dev);
  const int64_t bins = counts != nullptr ? (n_rows / rows_per_group) * (int64_t)(n_cls + 1) : 0;
  if (const int rc = zero_counters(counts, bins, st, "classifier count-zeroing kernel launch")) return rc;
  // every workgroup stages the parameters once, then walks tiles
  const int64_t tiles = mlp_tiles(n_rows);
  const int64_t grid = amcx::persistent_grid(cu_count(), 4, tiles, 1);
  const hipError_t e = amcx::launch(amcx::amcx_mlp_classify_kernel, grid, amcx::kMlpThreads, 0, st, x_dev, n_rows, row_stride, sel,
                                    mean_dev, scale_dev, params_dev, mlp_shape(widths_host, n_linear, activation), labels_dev, probs_dev,
                                    probs_stride, counts != nullptr ? rows_per_group : 1, counts, tiles);
  if (e != hipSuccess) return hip_fail(e, "classifier kernel launch");
  return AMCX_OK;
}

int64_t amcx_mlp_q15_params_shorts(const int32_t* widths_host, int32_t n_linear) { return amcx_mlp_params_floats(widths_host, n_linear); }

const char* amcx_kernel_name_mlp_q15(int32_t which) {
  return which == 0 ? "amcx_mlp_q15_kernel" : which == 1 ? "amcx_mlp_range_kernel" : which == 2 ? "amcx_mlp_range_init_kernel" : nullptr;
}

int amcx_mlp_range_f32(const float* x_dev, int64_t n_rows, int64_t row_stride, int32_t n_cols, const int32_t* cols_host,
                       int32_t n_sel, const double* mean_dev, const double* scale_dev, const float* params_dev,
                       const int32_t* widths_host, int32_t n_linear, int32_t activation, float* ranges_dev, int64_t* skipped_dev,
                       void* hip_stream) {
  amcx::SelectCols sel;
  if (!mlp_rows_ok(n_rows, row_stride, n_cols, cols_host, n_sel, mean_dev, scale_dev, widths_host, n_linear, &sel)) return AMCX_EINVAL;
  if (activation != AMCX_ACT_RELU && activation != AMCX_ACT_NONE) return AMCX_EINVAL;
  if (n_rows == 0) return AMCX_OK;
  if (!ptrs_ok({{x_dev, 3u, true}, {mean_dev, 7u, false}, {scale_dev, 7u, false}, {params_dev, 3u, true}, {ranges_dev, 3u, true},
                {skipped_dev, 7u, true}}))
    return AMCX_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  unsigned long long* const skipped = reinterpret_cast<unsigned long long*>(skipped_dev);
  hipError_t e = amcx::launch(amcx::amcx_mlp_range_init_kernel, 1, 64, 0, st, ranges_dev, n_linear + 1, skipped);
  if (e != hipSuccess) return hip_fail(e, "range initialising kernel launch");
  const int64_t tiles = mlp_tiles(n_rows);
  const int64_t grid = amcx::persistent_grid(cu_count(), 2, tiles, 1);         // 53 KiB of LDS: two workgroups a CU
  e = amcx::launch(amcx::amcx_mlp_range_kernel, grid, amcx::kMlpThreads, 0, st, x_dev, n_rows, row_stride, sel, mean_dev, scale_dev,
                   params_dev, mlp_shape(widths_host, n_linear, activation), ranges_dev, skipped, tiles);
  if (e != hipSuccess) return hip_fail(e, "range kernel launch");
  return AMCX_OK;
}

int amcx_mlp_classify_q15(const float* x_dev, int64_t n_rows, int64_t row_stride, int32_t n_cols, const int32_t* cols_host,
                          int32_t n_sel, const double* mean_dev, const double* scale_dev, const int16_t* params_dev,
                          const int32_t* widths_host, int32_t n_linear, int32_t activation, int32_t frac_input,
                          const int32_t* frac_weights_host, const int32_t* frac_biases_host, const int32_t* frac_outputs_host,
                          int32_t* labels_dev, int16_t* logits_dev, int64_t logits_stride, int64_t rows_per_group,
                          int64_t* counts_dev, int64_t* saturated_dev, void* hip_stream) {
  amcx::SelectCols sel;
  if (!mlp_rows_ok(n_rows, row_stride, n_cols, cols_host, n_sel, mean_dev, scale_dev, widths_host, n_linear, &sel)) return AMCX_EINVAL;
  if (activation != AMCX_ACT_RELU) return AMCX_EINVAL;
  if (frac_weights_host == nullptr || frac_biases_host == nullptr || frac_outputs_host == nullptr) return AMCX_EINVAL;
  const auto frac_ok = [](int32_t n) { return n >= 0 && n <= 15; };
  if (!frac_ok(frac_input)) return AMCX_EINVAL;
  amcx::Q15Formats fmt;
  fmt.in_scale = (float)(1 << frac_input);
  for (int l = 0, na = frac_input; l < amcx::kMlpMaxLinear; ++l) {
    fmt.shift_b[l] = 0;
    fmt.shift_o[l] = 1;
    if (l >= n_linear) continue;
    const int32_t nw = frac_weights_host[l], nb = frac_biases_host[l], no = frac_outputs_host[l];
    if (!frac_ok(nw) || !frac_ok(nb) || !frac_ok(no)) return AMCX_EINVAL;
    const int p = nw + na;
    if (p < nb || p <= no) return AMCX_EINVAL;
    fmt.shift_b[l] = p - nb;
    fmt.shift_o[l] = p - no;
    na = no;
  }
  const int n_cls = widths_host[n_linear];
  if (!opt_rows_ok(logits_dev, n_rows, logits_stride, n_cls) || !groups_ok(n_rows, rows_per_group, counts_dev)) return AMCX_EINVAL;
  if (n_rows == 0) return AMCX_OK;
  if (!ptrs_ok({{x_dev, 3u, true}, {mean_dev, 7u, false}, {scale_dev, 7u, false}, {params_dev, 1u, true}, {labels_dev, 3u, false},
                {logits_dev, 1u, false}, {counts_dev, 7u, false}, {saturated_dev, 7u, false}}))
    return AMCX_EINVAL;
  if (labels_dev == nullptr && logits_dev == nullptr && counts_dev == nullptr && saturated_dev == nullptr) return AMCX_OK;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  unsigned long long* const counts = reinterpret_cast<unsigned long long*>(counts_dev);
  unsigned long long* const saturated = reinterpret_cast<unsigned long long*>(saturated_dev);
  const int64_t bins = counts != nullptr ? (n_rows / rows_per_group) * (int64_t)(n_cls + 1) : 0;
  if (const int rc = zero_counters(counts, bins, st, "Q15 count-zeroing kernel launch")) return rc;
  if (const int rc = zero_counters(saturated, n_linear + 1, st, "Q15 saturation-zeroing kernel launch")) return rc;
  const int64_t tiles = mlp_tiles(n_rows);
  const int64_t grid = amcx::persistent_grid(cu_count(), 4, tiles, 1);
  const hipError_t e = amcx::launch(amcx::amcx_mlp_q15_kernel, grid, amcx::kMlpThreads, 0, st, x_dev, n_rows, row_stride, sel, mean_dev,
                                    scale_dev, params_dev, mlp_shape(widths_host, n_linear, activation), fmt, labels_dev, logits_dev,
                                    logits_stride, counts != nullptr ? rows_per_group : 1, counts, saturated, tiles);
  if (e != hipSuccess) return hip_fail(e, "Q15 classifier kernel launch");
  return AMCX_OK;
}

// ---- ABI 16.1: training ------------------------------------------------------------------------------------------------------
}  // extern "C"

namespace {

bool train_shape_ok(const int32_t* widths_host, int32_t n_linear, uint32_t bn_mask, int32_t optimizer) {
  return mlp_shape_ok(widths_host, n_linear) && (bn_mask >> (n_linear - 1)) == 0u &&
         (optimizer == AMCX_OPT_RMSPROP || optimizer == AMCX_OPT_ADAM);
}

template <int ACT, int OPT>
struct TrainKernel {
  static constexpr auto kern = amcx::amcx_mlp_train_kernel<ACT, OPT>;
  static constexpr const char* name() {
    return ACT == amcx::kActRelu ? (OPT == amcx::kOptRmsprop ? "amcx_mlp_train_kernel<0, 0>" : "amcx_mlp_train_kernel<0, 1>")
           : ACT == amcx::kActTanh ? (OPT == amcx::kOptRmsprop ? "amcx_mlp_train_kernel<1, 0>" : "amcx_mlp_train_kernel<1, 1>")
                                   : (OPT == amcx::kOptRmsprop ? "amcx_mlp_train_kernel<2, 0>" : "amcx_mlp_train_kernel<2, 1>");
  }
};
// the kernel of an (activation, optimizer), handed to `f` as one of the six; both in range already
template <class F>
auto for_train_kernel(int32_t activation, int32_t optimizer, F&& f) {
  const bool adam = optimizer == AMCX_OPT_ADAM;
  if (activation == AMCX_ACT_RELU) return adam ? f(TrainKernel<amcx::kActRelu, amcx::kOptAdam>{}) : f(TrainKernel<amcx::kActRelu, amcx::kOptRmsprop>{});
  if (activation == AMCX_ACT_TANH) return adam ? f(TrainKernel<amcx::kActTanh, amcx::kOptAdam>{}) : f(TrainKernel<amcx::kActTanh, amcx::kOptRmsprop>{});
  return adam ? f(TrainKernel<amcx::kActSigmoid, amcx::kOptAdam>{}) : f(TrainKernel<amcx::kActSigmoid, amcx::kOptRmsprop>{});
}
bool train_act_ok(int32_t activation) {
  return activation == AMCX_ACT_RELU || activation == AMCX_ACT_TANH || activation == AMCX_ACT_SIGMOID;
}
bool finite32(float v) { return v - v == 0.0f; }

}  // namespace

extern "C" {

int amcx_abi_minor(void) { return AMCX_ABI_MINOR; }

int64_t amcx_mlp_train_state_floats(const int32_t* widths_host, int32_t n_linear, uint32_t bn_mask, int32_t optimizer) {
  if (!train_shape_ok(widths_host, n_linear, bn_mask, optimizer)) return -1;
  return amcx::train_layout(mlp_shape(widths_host, n_linear, 0), bn_mask, optimizer).state_floats();
}

int64_t amcx_mlp_train_workspace_floats(const int32_t* widths_host, int32_t n_linear, int32_t batch) {
  if (!mlp_shape_ok(widths_host, n_linear) || batch < 2 || batch > amcx::kTrainMaxBatch) return -1;
  return amcx::train_ws_floats(n_linear, batch);
}

const char* amcx_kernel_name_mlp_train(int32_t activation, int32_t optimizer) {
  if (activation == -1 && optimizer == -1) return "amcx_mlp_train_hyper_kernel";
  if (!train_act_ok(activation) || (optimizer != AMCX_OPT_RMSPROP && optimizer != AMCX_OPT_ADAM)) return nullptr;
  return for_train_kernel(activation, optimizer, [](auto k) { return decltype(k)::name(); });
}

int amcx_mlp_train_f32(const float* x_dev, int64_t n_rows, int64_t row_stride, int32_t n_cols, const int32_t* cols_host, int32_t n_sel,
                       const double* mean_dev, const double* scale_dev, const int32_t* y_dev, const int32_t* idx_dev, int64_t n_idx,
                       int64_t idx_model_stride, const int32_t* widths_host, int32_t n_linear, int32_t activation, uint32_t bn_mask,
                       int32_t optimizer, int32_t batch, int32_t n_models, float* state_dev, int64_t* steps_dev, float* ws_dev,
                       const float* lr_host, const uint32_t* drop_threshold_host, const float* keep_scale_host, const uint64_t* seed_host,
                       int64_t step0, int32_t n_steps, double* history_dev, void* hip_stream) {
  amcx::SelectCols sel;
  if (!mlp_rows_ok(n_rows, row_stride, n_cols, cols_host, n_sel, mean_dev, scale_dev, widths_host, n_linear, &sel)) return AMCX_EINVAL;
  if (!train_act_ok(activation) || !train_shape_ok(widths_host, n_linear, bn_mask, optimizer)) return AMCX_EINVAL;
  if (batch < 2 || batch > amcx::kTrainMaxBatch || n_models < 1 || n_steps < 0 || step0 < 0 || n_idx < 0 || n_idx > 0x7fffffffLL ||
      idx_model_stride < 0 || (idx_model_stride != 0 && idx_model_stride < n_idx) || step0 > 0x7fffffffLL)
    return AMCX_EINVAL;
  if (n_idx % batch == 1) return AMCX_EINVAL;                        // a batch of one row: BatchNorm has no variance of it
  if (n_steps > 0 && (step0 * batch >= n_idx || (step0 + n_steps - 1) * batch >= n_idx)) return AMCX_EINVAL;
  if (lr_host == nullptr || drop_threshold_host == nullptr || keep_scale_host == nullptr || seed_host == nullptr) return AMCX_EINVAL;
  for (int m = 0; m < n_models; ++m)
    if (!finite32(lr_host[m]) || !finite32(keep_scale_host[m])) return AMCX_EINVAL;
  if (n_steps == 0 || n_rows == 0) return AMCX_OK;
  if (!ptrs_ok({{x_dev, 3u, true}, {mean_dev, 7u, false}, {scale_dev, 7u, false}, {y_dev, 3u, true}, {idx_dev, 3u, true},
                {state_dev, 3u, true}, {steps_dev, 7u, true}, {ws_dev, 15u, true}, {history_dev, 7u, true}}))
    return AMCX_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const amcx::MlpShape shape = mlp_shape(widths_host, n_linear, activation);
  const int64_t ws_floats = amcx::train_ws_floats(n_linear, batch);
  for (int first = 0; first < n_models; first += amcx::kTrainUploadModels) {
    const int n = n_models - first < amcx::kTrainUploadModels ? n_models - first : amcx::kTrainUploadModels;
    amcx::TrainHyperChunk h = {};
    for (int i = 0; i < n; ++i) {
      h.lr[i] = lr_host[first + i];
      h.thr[i] = drop_threshold_host[first + i];
      h.keep[i] = keep_scale_host[first + i];
      h.seed_lo[i] = (unsigned)(seed_host[first + i] & 0xffffffffull);
      h.seed_hi[i] = (unsigned)(seed_host[first + i] >> 32);
    }
    const hipError_t e = amcx::launch(amcx::amcx_mlp_train_hyper_kernel, 1, amcx::kTrainUploadModels, 0, st, h, n, ws_dev, ws_floats, first);
    if (e != hipSuccess) return hip_fail(e, "training hyperparameter kernel launch");
  }
  const hipError_t e = for_train_kernel(activation, optimizer, [&](auto k) {
    constexpr auto kern = decltype(k)::kern;
    if (const hipError_t a = amcx::lds_attr_once<kern>(amcx::train_lds_bytes(amcx::kTrainMaxBatch)); a != hipSuccess) return a;
    return amcx::launch(kern, n_models, amcx::kTrainThreads, (size_t)amcx::train_lds_bytes(batch), st, x_dev, n_rows, row_stride, sel,
                        mean_dev, scale_dev, y_dev, idx_dev, n_idx, idx_model_stride, shape, bn_mask, batch, state_dev,
                        reinterpret_cast<long long*>(steps_dev), ws_dev,
                        step0, n_steps, history_dev);
  });
  if (e != hipSuccess) return hip_fail(e, "training kernel launch");
  return AMCX_OK;
}

// ---- ABI 16.2: the waveform generator (amcx_synth_kernel.h) ---------------------------------------------------------------------
}  // extern "C"

namespace {

// the limits a shape has on its own (the plan's and the entry's first check); the rows, the strides and the groups are the entry's
bool synth_shape_ok(int32_t order, int32_t n_taps, int32_t up, int32_t down) {
  return order >= 0 && order <= amcx::kSynMaxOrder && up >= 1 && up <= amcx::kSynMaxUp && down >= 1 && down <= amcx::kSynMaxDown &&
         n_taps >= 1 && n_taps <= amcx::kSynMaxTaps;
}

}  // namespace

extern "C" {

int amcx_synth_plan(int32_t order, int32_t n_taps, int32_t up, int32_t down, int32_t* tile_outputs, int32_t* lds_bytes,
                    int32_t* max_workgroups) {
  if (!synth_shape_ok(order, n_taps, up, down)) return AMCX_EINVAL;
  const size_t lds = amcx::syn_lds_bytes(n_taps, up, down, order);
  if (tile_outputs != nullptr) *tile_outputs = amcx::syn_tile_outputs(n_taps, up, down);
  if (lds_bytes != nullptr) *lds_bytes = (int32_t)lds;
  if (max_workgroups != nullptr) *max_workgroups = cu_count() * wgs_per_cu(lds, 8);
  return AMCX_OK;
}

int amcx_synth_c64(uint64_t seed, uint64_t row_index0, int64_t sample_index0, int64_t n_rows, int64_t row_samples, int64_t row_stride,
                   const void* table_c64_dev, int32_t order, const float* taps_dev, int32_t n_taps, int32_t up, int32_t down,
                   int32_t tau0, uint64_t phase_step, uint32_t cfo_max, uint32_t flags, const float* sigma_dev,
                   int64_t frames_per_group, void* out_c64_dev, void* hip_stream) {
  if (!synth_shape_ok(order, n_taps, up, down)) return AMCX_EINVAL;
  if (tau0 < 0 || tau0 >= up || (flags & ~(uint32_t)(AMCX_SYNTH_RANDOM_PHASE | AMCX_SYNTH_RANDOM_TIMING)) != 0u) return AMCX_EINVAL;
  if (row_samples < 1 || sample_index0 < 0 || sample_index0 >= (int64_t(1) << 40) || row_samples >= (int64_t(1) << 40) ||
      sample_index0 + row_samples >= (int64_t(1) << 40))
    return AMCX_EINVAL;
  if (n_rows < 0 || row_stride < row_samples || (n_rows > 0 && row_stride > (int64_t(1) << 58) / n_rows) || frames_per_group < 1)
    return AMCX_EINVAL;
  if (n_rows == 0) return AMCX_OK;
  if (!ptrs_ok({{out_c64_dev, 7u, true}, {taps_dev, 3u, true}, {table_c64_dev, 3u, order > 0}, {sigma_dev, 3u, true}}))
    return AMCX_EINVAL;
  amcx::SynArgs a;
  a.seed_lo = (unsigned)(seed & 0xffffffffull);
  a.seed_hi = (unsigned)(seed >> 32);
  a.row_index0 = row_index0;
  a.sample_index0 = sample_index0;
  a.n_rows = n_rows;
  a.row_samples = row_samples;
  a.row_stride = row_stride;
  a.table = static_cast<const float2*>(table_c64_dev);
  a.order = order;
  a.taps = taps_dev;
  a.T = n_taps;
  a.U = up;
  a.V = down;
  a.P = amcx::poly_phase_taps(n_taps, up);
  a.tau0 = tau0;
  a.max_span = amcx::syn_max_span(n_taps, up, down);
  a.phase_step = phase_step;
  a.cfo_max = cfo_max;
  a.flags = flags;
  a.sigma = sigma_dev;
  a.frames_per_group = frames_per_group;
  a.out = static_cast<float2*>(out_c64_dev);
  a.tile = amcx::syn_tile_outputs(n_taps, up, down);
  a.tiles_per_row = (row_samples + a.tile - 1) / a.tile;
  a.n_items = n_rows * a.tiles_per_row;
  const size_t lds = amcx::syn_lds_bytes(n_taps, up, down, order);
  const int64_t grid = amcx::persistent_grid(cu_count(), wgs_per_cu(lds, 8), a.n_items, 1);
  const hipError_t e = amcx::launch(amcx::amcx_synth_c64_kernel, grid, amcx::kSynThreads, lds, static_cast<hipStream_t>(hip_stream), a);
  if (e != hipSuccess) return hip_fail(e, "waveform generator kernel launch");
  return AMCX_OK;
}

const char* amcx_kernel_name_synth(void) { return "amcx_synth_c64_kernel"; }

}  // extern "C"

// ---- ABI 16.2.1: the fading multipath channel (amcx_channel_kernel.h) -----------------------------------------------------------
namespace {

// the limits a shape has on its own (the plan's and the entry's first check)
bool channel_shape_ok(int32_t n_paths, int32_t n_sinusoids, int32_t interp_log2, int32_t max_delay) {
  return n_paths >= 1 && n_paths <= amcx::kChanMaxPaths && n_sinusoids >= 1 && n_sinusoids <= amcx::kChanMaxSinusoids &&
         interp_log2 >= 0 && interp_log2 <= amcx::kChanMaxInterpLog2 && max_delay >= 0 && max_delay <= amcx::kChanMaxDelay;
}

}  // namespace

extern "C" {

int amcx_abi_patch(void) { return AMCX_ABI_PATCH; }

int amcx_channel_plan(int32_t n_paths, int32_t n_sinusoids, int32_t interp_log2, int32_t max_delay, int32_t* tile_outputs,
                      int32_t* lds_bytes) {
  if (!channel_shape_ok(n_paths, n_sinusoids, interp_log2, max_delay)) return AMCX_EINVAL;
  if (tile_outputs != nullptr) *tile_outputs = amcx::chan_tile_outputs(n_paths, interp_log2);
  if (lds_bytes != nullptr) *lds_bytes = (int32_t)amcx::chan_lds_bytes(n_paths, n_sinusoids, interp_log2, max_delay);
  return AMCX_OK;
}

int amcx_channel_c64(uint64_t seed, uint64_t row_index0, int64_t sample_index0, int64_t n_rows, int64_t row_samples,
                     const void* in_c64_dev, int64_t in_row_stride, const void* paths_host, int32_t n_paths, int32_t n_sinusoids,
                     int32_t interp_log2, uint32_t doppler_max, uint32_t flags, const float* sigma_dev, int64_t frames_per_group,
                     void* out_c64_dev, int64_t out_row_stride, void* hip_stream) {
  static_assert(sizeof(amcx::ChanPath) == 16, "the header's path record");
  if (!channel_shape_ok(n_paths, n_sinusoids, interp_log2, 0) || paths_host == nullptr) return AMCX_EINVAL;
  if ((flags & ~(uint32_t)AMCX_CHANNEL_RANDOM_PHASE) != 0u) return AMCX_EINVAL;
  amcx::ChanArgs a = {};
  memcpy(a.paths, paths_host, sizeof(amcx::ChanPath) * (size_t)n_paths);
  int32_t H = 0;
  for (int l = 0; l < n_paths; ++l) {
    if (a.paths[l].delay < 0 || a.paths[l].delay > amcx::kChanMaxDelay) return AMCX_EINVAL;
    if (a.paths[l].delay > H) H = a.paths[l].delay;
  }
  if (row_samples < 1 || sample_index0 < 0 || sample_index0 >= (int64_t(1) << 40) || row_samples >= (int64_t(1) << 40) ||
      sample_index0 + row_samples >= (int64_t(1) << 40))
    return AMCX_EINVAL;
  if (n_rows < 0 || in_row_stride < row_samples + H || out_row_stride < row_samples || frames_per_group < 1 ||
      (n_rows > 0 && (in_row_stride > (int64_t(1) << 58) / n_rows || out_row_stride > (int64_t(1) << 58) / n_rows)))
    return AMCX_EINVAL;
  a.tile = amcx::chan_tile_outputs(n_paths, interp_log2);
  a.tiles_per_row = (row_samples + a.tile - 1) / a.tile;
  if (n_rows > 0 && a.tiles_per_row > (int64_t)0x7fffffff / n_rows) return AMCX_EINVAL;
  if (n_rows == 0) return AMCX_OK;
  if (!ptrs_ok({{in_c64_dev, 7u, true}, {out_c64_dev, 7u, true}, {sigma_dev, 3u, false}})) return AMCX_EINVAL;
  // the kernel reads neighbours of the sample it writes: the two byte ranges must not meet
  const uintptr_t in0 = reinterpret_cast<uintptr_t>(in_c64_dev), out0 = reinterpret_cast<uintptr_t>(out_c64_dev);
  const uintptr_t in1 = in0 + 8u * (uintptr_t)((n_rows - 1) * in_row_stride + row_samples + H);
  const uintptr_t out1 = out0 + 8u * (uintptr_t)((n_rows - 1) * out_row_stride + row_samples);
  if (in0 < out1 && out0 < in1) return AMCX_EINVAL;
  a.seed_lo = (unsigned)(seed & 0xffffffffull);
  a.seed_hi = (unsigned)(seed >> 32);
  a.row_index0 = row_index0;
  a.sample_index0 = sample_index0;
  a.n_rows = n_rows;
  a.row_samples = row_samples;
  a.in_stride = in_row_stride;
  a.out_stride = out_row_stride;
  a.in = static_cast<const float2*>(in_c64_dev);
  a.L = n_paths;
  a.S = n_sinusoids;
  a.b = interp_log2;
  a.H = H;
  a.doppler_max = doppler_max;
  a.flags = flags;
  a.sigma = sigma_dev;
  a.frames_per_group = frames_per_group;
  a.out = static_cast<float2*>(out_c64_dev);
  a.n_items = n_rows * a.tiles_per_row;
  // a plain grid, one workgroup per (row, tile): lines of at most 2^16 workgroups, the last one cut by the kernel
  const int64_t gx = a.n_items < 65536 ? a.n_items : 65536, gy = (a.n_items + gx - 1) / gx;
  const size_t lds = amcx::chan_lds_bytes(n_paths, n_sinusoids, interp_log2, H);
  const hipError_t e = amcx::launch(amcx::amcx_channel_c64_kernel, dim3((unsigned)gx, (unsigned)gy), amcx::kChanThreads, lds,
                                    static_cast<hipStream_t>(hip_stream), a);
  if (e != hipSuccess) return hip_fail(e, "channel kernel launch");
  return AMCX_OK;
}

const char* amcx_kernel_name_channel(void) { return "amcx_channel_c64_kernel"; }

}  // extern "C"

// ---- ABI 16.2.2: the continuous-phase generator (amcx_synth_cpm_kernel.h) -------------------------------------------------------
namespace {

struct CpmPlan {
  int tile, segments;
  int64_t tiles_per_row, tiles_per_seg;
};

// the tiles of a row and their cut into segments; `asked` 0: 1 where the rows alone fill the device, else about two workgroups per
// CU, never more than the row's tiles or 64.  The segments are recounted from their length, so that none is empty.
CpmPlan cpm_plan(int32_t n_taps, int32_t up, int32_t down, int64_t n_rows, int64_t row_samples, int32_t asked) {
  CpmPlan p;
  p.tile = amcx::syn_tile_outputs(n_taps, up, down);
  p.tiles_per_row = (row_samples + p.tile - 1) / p.tile;
  int64_t want = asked;
  if (asked == 0) {
    const int64_t target = 2 * (int64_t)cu_count();
    want = n_rows < 1 || n_rows >= target ? 1 : (target + n_rows - 1) / n_rows;
  }
  if (want > amcx::kCpmMaxSegments) want = amcx::kCpmMaxSegments;
  if (want > p.tiles_per_row) want = p.tiles_per_row;
  p.tiles_per_seg = (p.tiles_per_row + want - 1) / want;
  p.segments = (int)((p.tiles_per_row + p.tiles_per_seg - 1) / p.tiles_per_seg);
  return p;
}

bool cpm_samples_ok(int64_t sample_index0, int64_t row_samples) {
  return row_samples >= 1 && sample_index0 >= 0 && sample_index0 < (int64_t(1) << 40) && row_samples < (int64_t(1) << 40) &&
         sample_index0 + row_samples < (int64_t(1) << 40);
}

}  // namespace

extern "C" {

int amcx_synth_cpm_plan(int32_t n_taps, int32_t up, int32_t down, int64_t n_rows, int64_t row_samples, int32_t* tile_outputs,
                        int32_t* lds_bytes, int32_t* segments) {
  if (!synth_shape_ok(2, n_taps, up, down) || !cpm_samples_ok(0, row_samples) || n_rows < 0) return AMCX_EINVAL;
  const CpmPlan p = cpm_plan(n_taps, up, down, n_rows, row_samples, 0);
  if (tile_outputs != nullptr) *tile_outputs = p.tile;
  if (lds_bytes != nullptr) *lds_bytes = (int32_t)amcx::cpm_lds_bytes(n_taps, up, down);
  if (segments != nullptr) *segments = p.segments;
  return AMCX_OK;
}

int amcx_synth_cpm_c64(uint64_t seed, uint64_t row_index0, int64_t sample_index0, int64_t n_rows, int64_t row_samples,
                       int64_t row_stride, int32_t order, const uint32_t* phase_taps_dev, int32_t n_taps, uint32_t phase_full,
                       int32_t up, int32_t down, int32_t tau0, uint64_t phase_step, uint32_t cfo_max, uint32_t flags,
                       const float* sigma_dev, int64_t frames_per_group, const uint32_t* acc_in_dev, uint32_t* acc_out_dev,
                       int32_t segments, void* out, void* hip_stream) {
  if (order < 2 || !synth_shape_ok(order, n_taps, up, down)) return AMCX_EINVAL;
  if (tau0 < 0 || tau0 >= up || (flags & ~(uint32_t)(AMCX_SYNTH_RANDOM_PHASE | AMCX_SYNTH_RANDOM_TIMING)) != 0u) return AMCX_EINVAL;
  if (!cpm_samples_ok(sample_index0, row_samples)) return AMCX_EINVAL;
  if (n_rows < 0 || row_stride < row_samples || (n_rows > 0 && row_stride > (int64_t(1) << 58) / n_rows) || frames_per_group < 1)
    return AMCX_EINVAL;
  if (segments < 0 || segments > amcx::kCpmMaxSegments) return AMCX_EINVAL;
  const CpmPlan p = cpm_plan(n_taps, up, down, n_rows, row_samples, segments);
  if (n_rows > 0 && p.segments > (int64_t)0x7fffffff / n_rows) return AMCX_EINVAL;
  if (n_rows == 0) return AMCX_OK;
  if (!ptrs_ok({{out, 7u, true}, {phase_taps_dev, 3u, true}, {sigma_dev, 3u, true}, {acc_in_dev, 3u, sample_index0 > 0},
                {acc_out_dev, 3u, false}}))
    return AMCX_EINVAL;
  if (acc_in_dev != nullptr && acc_out_dev != nullptr) {               // a segment reads a row's word another may have written
    const uintptr_t in0 = reinterpret_cast<uintptr_t>(acc_in_dev), out0 = reinterpret_cast<uintptr_t>(acc_out_dev);
    if (in0 < out0 + 4u * (uintptr_t)n_rows && out0 < in0 + 4u * (uintptr_t)n_rows) return AMCX_EINVAL;
  }
  amcx::CpmArgs a;
  a.seed_lo = (unsigned)(seed & 0xffffffffull);
  a.seed_hi = (unsigned)(seed >> 32);
  a.row_index0 = row_index0;
  a.sample_index0 = sample_index0;
  a.n_rows = n_rows;
  a.row_samples = row_samples;
  a.row_stride = row_stride;
  a.order = order;
  a.taps = phase_taps_dev;
  a.phase_full = phase_full;
  a.T = n_taps;
  a.U = up;
  a.V = down;
  a.P = amcx::poly_phase_taps(n_taps, up);
  a.tau0 = tau0;
  a.max_span = amcx::syn_max_span(n_taps, up, down);
  a.phase_step = phase_step;
  a.cfo_max = cfo_max;
  a.flags = flags;
  a.sigma = sigma_dev;
  a.frames_per_group = frames_per_group;
  a.acc_in = acc_in_dev;
  a.acc_out = acc_out_dev;
  a.out = static_cast<float2*>(out);
  a.tile = p.tile;
  a.segments = p.segments;
  a.tiles_per_row = p.tiles_per_row;
  a.tiles_per_seg = p.tiles_per_seg;
  a.n_items = n_rows * p.segments;
  // a plain grid, one workgroup per (row, segment): lines of at most 2^16 workgroups, the last one cut by the kernel
  const int64_t gx = a.n_items < 65536 ? a.n_items : 65536, gy = (a.n_items + gx - 1) / gx;
  const hipError_t e = amcx::launch(amcx::amcx_synth_cpm_c64_kernel, dim3((unsigned)gx, (unsigned)gy), amcx::kCpmThreads,
                                    amcx::cpm_lds_bytes(n_taps, up, down), static_cast<hipStream_t>(hip_stream), a);
  if (e != hipSuccess) return hip_fail(e, "continuous-phase generator kernel launch");
  return AMCX_OK;
}

const char* amcx_kernel_name_synth_cpm(void) { return "amcx_synth_cpm_c64_kernel"; }

}  // extern "C"

// ---- ABI 16.2.3: blind carrier recovery (amcx_carrier_kernel.h) -----------------------------------------------------------------
namespace {

// log2 of the order, -1 where it is none of 1, 2, 4, 8
int carrier_log2_order(int32_t order) { return order == 1 ? 0 : order == 2 ? 1 : order == 4 ? 2 : order == 8 ? 3 : -1; }

}  // namespace

extern "C" {

int amcx_carrier_plan(int32_t n, int32_t* rows_per_workgroup, int32_t* lds_bytes) {
  if (psd_log2(n) < 0) return AMCX_EINVAL;
  if (rows_per_workgroup != nullptr) *rows_per_workgroup = amcx::kPsdPoints / n;
  if (lds_bytes != nullptr) *lds_bytes = amcx::kCarLdsBytes;
  return AMCX_OK;
}

int amcx_carrier_c64(const void* in_c64_dev, int64_t n_rows, int32_t n, int64_t in_row_stride, int32_t order, int32_t search_bins,
                     uint32_t flags, void* est_dev, void* out_c64_dev, int64_t out_row_stride, void* hip_stream) {
  static_assert(sizeof(amcx::CarrierRecord) == 32, "the header's record");
  static_assert(amcx::kCarLdsBytes <= 65536, "static LDS: no attribute");
  const int lg = psd_log2(n), lm = carrier_log2_order(order);
  if (lg < 0 || lm < 0) return AMCX_EINVAL;
  if (search_bins < 0 || search_bins > n / 2 - 1) return AMCX_EINVAL;
  const uint32_t apply = AMCX_CARRIER_GAIN | AMCX_CARRIER_FREQ | AMCX_CARRIER_PHASE;
  if ((flags & ~(apply | (uint32_t)AMCX_CARRIER_GIVEN)) != 0u) return AMCX_EINVAL;
  if ((flags & AMCX_CARRIER_GIVEN) != 0u && out_c64_dev == nullptr) return AMCX_EINVAL;     // nothing to estimate, nothing to write
  if (!rows_ok(n_rows, in_row_stride, n) || !opt_rows_ok(out_c64_dev, n_rows, out_row_stride, n)) return AMCX_EINVAL;
  const int64_t G = amcx::kPsdPoints / n, n_groups = (n_rows + G - 1) / G;
  if (n_groups > (int64_t)0x7fffffff) return AMCX_EINVAL;
  if (n_rows == 0) return AMCX_OK;
  if (!ptrs_ok({{in_c64_dev, 7u, true}, {est_dev, 7u, true}, {out_c64_dev, 7u, false}})) return AMCX_EINVAL;
  if (out_c64_dev != nullptr) {                                        // a kept row is written where another workgroup may still read
    const uintptr_t in0 = reinterpret_cast<uintptr_t>(in_c64_dev), out0 = reinterpret_cast<uintptr_t>(out_c64_dev);
    const uintptr_t in1 = in0 + 8u * (uintptr_t)((n_rows - 1) * in_row_stride + n);
    const uintptr_t out1 = out0 + 8u * (uintptr_t)((n_rows - 1) * out_row_stride + n);
    if (in0 < out1 && out0 < in1) return AMCX_EINVAL;
  }
  amcx::CarrierArgs a;
  a.in = static_cast<const float2*>(in_c64_dev);
  a.n_rows = n_rows;
  a.in_stride = in_row_stride;
  a.n = n;
  a.lg = lg;
  a.lm = lm;
  a.search = search_bins;
  a.flags = flags;
  a.est = static_cast<amcx::CarrierRecord*>(est_dev);
  a.out = static_cast<float2*>(out_c64_dev);
  a.out_stride = out_row_stride;
  a.n_groups = n_groups;
  // a plain grid, one workgroup per group of rows: lines of at most 2^16 workgroups, the last one cut by the kernel
  const int64_t gx = n_groups < 65536 ? n_groups : 65536, gy = (n_groups + gx - 1) / gx;
  const hipError_t e = amcx::launch(amcx::amcx_carrier_c64_kernel, dim3((unsigned)gx, (unsigned)gy), amcx::kCarThreads, 0,
                                    static_cast<hipStream_t>(hip_stream), a);
  if (e != hipSuccess) return hip_fail(e, "carrier recovery kernel launch");
  return AMCX_OK;
}

const char* amcx_kernel_name_carrier(void) { return "amcx_carrier_c64_kernel"; }

}  // extern "C"
