// The host context of libamcx.so (include/amcx.h, amcx_ctx_*): what a context owns, and the engine that takes a host
// container through it -- staged by the pool of amcx_upload.h, uploaded, computed, copied back (ctx_run_strided ->
// run_small_graph / run_chunked).  No kernels.  amcx.hip includes this BEHIND its feature dispatch: the engine is built on
// run_features, and it names the packing kernels, which have to stay behind the feature kernels (KERNEL ORDER, amcx_launch.h).
//
// Every handle is a member that frees itself, and every buffer moves the context's buffers_generation on when it
// reallocates: a captured graph, whose nodes hold addresses inside the buffers, is replayed only under the generation it
// was captured in (GraphKey).  A new buffer is one line of amcx_ctx and nothing else.
#pragma once

#include "amcx_upload.h"

namespace {      // (as everything of this header but amcx_ctx itself: nothing here is an exported symbol)

struct NoCopy { NoCopy() = default; NoCopy(const NoCopy&) = delete; NoCopy& operator=(const NoCopy&) = delete; };

// Memory of the device (PINNED: of the host) that only grows.  reserve() keeps the address while `bytes` fit; otherwise the
// old block is freed first (hipFree waits for the device: nothing still runs on it), `generation`, where there is one, moves
// on, and bytes + slack are allocated.  AMCX_ENOMEM leaves the buffer empty.  The generation is deliberately coarse: ANY
// buffer's reallocation retires every cached graph, also one that never pointed into it (d_frames), and a failed +25 %
// attempt with its exact-size retry moves it twice.  That costs a capture, never a stale address; a key of addresses
// would save the capture and bring back the field that somebody forgets.
template <bool PINNED>
struct Buffer : NoCopy {
  void* p = nullptr;
  size_t cap = 0;
  uint64_t* generation;
  explicit Buffer(uint64_t* gen = nullptr) : generation(gen) {}
  ~Buffer() { release(); }
  template <class T> T* as() const { return static_cast<T*>(p); }
  void release() { if (p != nullptr) (void)(PINNED ? hipHostFree(p) : hipFree(p)); p = nullptr; cap = 0; }
  int reserve(size_t bytes, size_t slack = 0) {
    if (cap >= bytes) return AMCX_OK;
    release();
    if (generation != nullptr) ++*generation;
    const hipError_t e = PINNED ? hipHostMalloc(&p, bytes + slack, hipHostMallocDefault) : hipMalloc(&p, bytes + slack);
    if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr; return AMCX_ENOMEM; }
    cap = bytes + slack;
    return AMCX_OK;
  }
};
using PinnedBuffer = Buffer<true>;
// Device memory grows to the exact size below 1 MiB; above, by a quarter more, so that a slowly growing batch size does
// not reallocate every call, and to the exact size if that fails.
struct DeviceBuffer : Buffer<false> {
  using Buffer::Buffer;
  int reserve(size_t bytes) {
    if (bytes >= (size_t(1) << 20) && Buffer::reserve(bytes, bytes / 4) == AMCX_OK) return AMCX_OK;
    return Buffer::reserve(bytes);
  }
};

// A non-blocking stream, an event and an instantiated graph: created once (create() on one that exists does nothing),
// destroyed with their owner.
struct Stream : NoCopy {
  hipStream_t s = nullptr;
  ~Stream() { if (s != nullptr) (void)hipStreamDestroy(s); }
  hipError_t create() { return s != nullptr ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
  operator hipStream_t() const { return s; }
};
struct Event : NoCopy {
  hipEvent_t e = nullptr;
  ~Event() { if (e != nullptr) (void)hipEventDestroy(e); }
  hipError_t create(unsigned flags) { return e != nullptr ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
  operator hipEvent_t() const { return e; }
};
struct GraphExec : NoCopy {
  hipGraphExec_t x = nullptr;
  ~GraphExec() { reset(nullptr); }
  void reset(hipGraphExec_t next) { if (x != nullptr) (void)hipGraphExecDestroy(x); x = next; }
};

}  // namespace

// ---- host-buffer entry points over a reusable context --------------------------------------
// The context owns two streams, pinned staging slots and device scratch that only ever grow, so a
// loop of per-frame calls (the reference's usage pattern, features.py:214-232 called once per queue
// item) pays two small copies and the launches, not hipMalloc/hipFree/stream creation per call, and
// a whole container goes up through the staged, overlapped path (ctx_run_strided).
// MEMBER ORDER is destruction order backwards (amcx_ctx_destroy has synchronised both streams before): the streams go
// first, then events, buffers and graphs, and the staging pool is joined last.
// (Hidden: its members are of anonymous-namespace types, and its implicit constructor and destructor would otherwise join
// the library's exported symbols; callers hold it as the opaque amcx_ctx* of include/amcx.h.)
struct __attribute__((visibility("hidden"))) amcx_ctx {
  int device = 0;
  // strided containers (amcx_ctx_features18_strided_host): staging pool, three pinned slots, a second stream
  amcx::Pool pool;
  int threads = 0;                               // 0: not yet sized
  size_t slot_bytes = size_t(32) << 20;
  bool round_on_device = false;
  amcx_upload_stats stats = {};
  // host placement (amcx_upload.h, NumaPlace): the CPUs local to this device; staging threads, the calling thread for the
  // duration of a threaded upload, and with it the pinned slots it allocates, stay on them.  Empty: nothing is bound.
  char pci_bus_id[32] = {0};
  int numa_node = -1;
  std::vector<int> bind_cpus;
  // small row-major calls (a loop of per-frame calculate_features calls): the copy in, the launches and the copy
  // out as ONE instantiated graph per (frames, frame size, variant, element type, buffers), relaunched
  struct GraphKey {
    int64_t frames = 0; int32_t frame_size = 0, variant = 0; bool c128 = false, zero_copy = false;
    bool sc16 = false; float sc16_scale = 0.f;   // the element kind, and the scale the captured kernel node carries as an argument
    int32_t iq8_kind = 0; float iq8_scale = 0.f; // likewise AMCX_SRC_CI8 / _CU8 (0: neither) and the 8-bit scale
    uint64_t generation = 0;             // buffers_generation at capture: every address a captured node holds
    uint32_t mask = AMCX_FEATURES_ALL;   // the feature mask the captured kernels were launched for
    bool operator==(const GraphKey& o) const {
      return frames == o.frames && frame_size == o.frame_size && variant == o.variant && c128 == o.c128 &&
             zero_copy == o.zero_copy && generation == o.generation && mask == o.mask && sc16 == o.sc16 &&
             sc16_scale == o.sc16_scale && iq8_kind == o.iq8_kind && iq8_scale == o.iq8_scale;
    }
  };
  struct SmallGraph { GraphExec exec; GraphKey key; };
  SmallGraph graphs[4];
  int graph_next = 0;               // slot the next capture replaces
  int graph_hits = 0, graph_misses = 0;
  bool graphs_ok = true;            // false: capture failed once, or the calls vary too much for a cache of four
  uint64_t buffers_generation = 0;  // moves on whenever one of the buffers below reallocates
  DeviceBuffer d_out{&buffers_generation};
  DeviceBuffer d_slab{&buffers_generation};     // 2 x slot: uploaded chunks
  DeviceBuffer d_frames{&buffers_generation};   // plane-major sources: the frame-major complex64 image
  DeviceBuffer d_ws{&buffers_generation};       // the any-size path's FFT workspace (frame sizes above 8192, amcx_features18_c64_ws)
  DeviceBuffer d_ring{&buffers_generation};     // the wave kernels' ring of stash rows (RingSource): this context's launches only
  PinnedBuffer pin{&buffers_generation};        // kPinSlots x slot
  PinnedBuffer out_pin{&buffers_generation};    // the result lands in pinned memory first
  Event up_done[3], slab_free[2];
  Stream stream, copy_stream;
  // calls in flight on this context (a context serves one call at a time): the setters below and amcx_ctx_bind_cpus
  // claim it idle, so that no call reads what they replace
  amcx::CallGate gate;
  // amcx_ctx_set_feature_mask: the features every later host-buffer call computes (read once per call)
  std::atomic<uint32_t> feature_mask{AMCX_FEATURES_ALL};
  // amcx_ctx_set_sc16_scale: what an int16 component of an sc16 source is multiplied by (read once per call)
  std::atomic<float> sc16_scale{0x1p-15f};
  // amcx_ctx_set_iq8_scale: the same for a component of an 8-bit source
  std::atomic<float> iq8_scale{0x1p-7f};
};

namespace {

// ---- host-buffer entry points over a reusable context: the helpers ---------------------------------------------------------
// The context's own workspace for a call of `frames` frames (nothing for the frame sizes that need none).  Reserved
// BEFORE any capture begins: a captured kernel node points into it, and an allocation inside a capture is not allowed.
// A context that cannot have it (a failed reserve leaves the buffer empty) runs the workspace-free form.
void ctx_reserve_ws(amcx_ctx* c, int32_t N, int64_t frames, int32_t variant) {
  const int64_t want = amcx_features18_workspace_bytes(N, frames, variant);
  if (want > 0) (void)c->d_ws.reserve((size_t)want);
  // likewise the ring of the wave kernels that take one; without it they run their LDS form
  // (one size per device, whatever the call's frame count)
  const size_t ring = resolve_variant(N, variant) == AMCX_VARIANT_WAVE ? amcx::wave_ring_bytes(N, cu_count()) : 0;
  if (ring > 0) (void)c->d_ring.reserve(ring);
}

// sc16: `rows` are sc16 and the size has a kernel that reads them (sc16_typed); otherwise complex64
int ctx_features(amcx_ctx* c, const void* rows, int64_t frames, int32_t N, float* out, int32_t variant, uint32_t mask,
                 const IntIn* sc16 = nullptr) {
  const int64_t want = amcx_features18_workspace_bytes(N, frames, variant);
  Workspace ws;
  if (want > 0 && c->d_ws.p != nullptr && c->d_ws.cap >= (size_t)want) { ws.dev = c->d_ws.p; ws.bytes = want; }
  RingSource rings;
  rings.own = c->d_ring.as<float>();
  rings.own_bytes = c->d_ring.cap;
  return run_features(rows, frames, N, N, out, AMCX_NUM_FEATURES, c->stream, variant, mask, ws, rings, sc16);
}

struct DeviceGuard {
  int prev = -1;
  hipError_t enter(int dev) {
    hipError_t e = hipGetDevice(&prev);
    if (e != hipSuccess) { prev = -1; return e; }
    return hipSetDevice(dev);
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// ---- strided host containers ----------------------------------------------------------------------
constexpr int kPinSlots = 3;

using amcx::classify_layout;      // amcx_upload.h: which axis is contiguous decides how a container goes up

double wall_now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int strided_prepare(amcx_ctx* c, size_t slot, size_t dslot, size_t frames_bytes, size_t out_bytes, bool threaded) {
  if (c->threads == 0) {
    unsigned hw = std::thread::hardware_concurrency();
    if (!c->bind_cpus.empty()) hw = (unsigned)amcx::allowed_subset(c->bind_cpus).size();   // this device's share of the host
    c->threads = (int)(hw == 0 ? 4 : hw > 8 ? 8 : hw);
  }
  if (threaded) c->pool.resize(c->threads);      // the staging threads start with the first call that has work for them
  AMCX_HIP(c->copy_stream.create());
  for (auto& ev : c->up_done) AMCX_HIP(ev.create(hipEventDisableTiming));
  for (auto& ev : c->slab_free) AMCX_HIP(ev.create(hipEventDisableTiming));
  int rc = c->pin.reserve(kPinSlots * slot);
  if (rc == AMCX_OK) rc = c->out_pin.reserve(out_bytes, out_bytes / 4 + 4096);
  if (rc == AMCX_OK) rc = c->d_slab.reserve(2 * dslot);
  if (rc == AMCX_OK && frames_bytes) rc = c->d_frames.reserve(frames_bytes);
  if (rc == AMCX_OK) rc = c->d_out.reserve(out_bytes);
  return rc;
}

// a staging thread could not read the container's file
int io_fail(int err) {
  snprintf(g_hip_err, sizeof g_hip_err, "reading the container's file: %s", strerror(err));
  return AMCX_EIO;
}

// One call of ctx_run_strided: what its prologue worked out, for run_small_graph and run_chunked.
struct StridedCall {
  amcx::Source src;
  amcx::RunMap map;
  std::atomic<int> io_error{0};
  int64_t S = 0, K = 0, F = 0;
  int32_t N = 0;
  int v = 0;                       // the resolved variant
  uint32_t mask = AMCX_FEATURES_ALL;
  bool rows = false, inner_snr = false, as_c128 = false, threaded = false;
  bool sc16 = false, sc16_typed = false;   // an sc16 source; a kernel of this size reads sc16 (otherwise it is widened on the device)
  bool iq8 = false;                        // an 8-bit source: widened on the device, to sc16 where sc16_typed, else to complex64
  IntIn sc16_in = {1.0f};                  // the scale of either; of an 8-bit source its format too (the kernels see sc16 or complex64)
  size_t esz = 8;                  // staged bytes per element
  int64_t unit = 0, n_units = 0;   // staged elements per chunk unit (a frame / a plane), and how many
  size_t total_staged = 0, slot = 0, dslot = 0;
  float* out_host = nullptr;
  int64_t out_row_stride = 0;
  amcx_upload_stats st = {};
  double t_start = 0, t_loop = 0;
  // uploaded rows that no kernel reads as they lie: convert_rows_on_device
  bool converts() const { return as_c128 || iq8 || (sc16 && !sc16_typed); }
};

// The rows of a device slot converted to complex64 into the room behind the slot: complex128 rounded, sc16 widened (the
// frame sizes and variants that have no sc16 kernel); 8-bit rows widened to sc16 (sc16_typed) or to complex64.
hipError_t convert_rows_on_device(amcx_ctx* c, const StridedCall& q, char* dev, int64_t frames, const void** d_rows) {
  float2* const wide = reinterpret_cast<float2*>(dev + q.slot);
  *d_rows = wide;
  if (q.iq8) return launch_iq8_widen(dev, frames, q.N, q.N, q.sc16_in, q.sc16_typed, wide, c->stream);
  if (q.as_c128)
    return amcx::launch(amcx::amcx_c128_to_c64_kernel, 2048, 256, 0, c->stream, reinterpret_cast<const double2*>(dev), frames,
                        q.N, q.N, wide);
  amcx::Frames fr{nullptr, frames, q.N, nullptr, 0, c->stream, cu_count()};
  fr.iq16 = reinterpret_cast<const amcx::wave::sc16*>(dev);
  fr.scale = q.sc16_in.scale;
  return launch_sc16_widen(fr, q.N, wide);
}

// the feature kernels over the rows of one chunk at `dev`: complex64, complex128 (rounded first), sc16 (read by the
// kernel, or widened first) or 8-bit (widened first, to what the kernel reads)
int chunk_features(amcx_ctx* c, const StridedCall& q, char* dev, int64_t frames, float* out, hipError_t* e) {
  const void* d_rows = dev;
  if (q.converts()) *e = convert_rows_on_device(c, q, dev, frames, &d_rows);
  if (*e != hipSuccess) return AMCX_OK;
  const IntIn as_sc16{q.sc16_in.scale};
  return ctx_features(c, d_rows, frames, q.N, out, q.v, q.mask, q.sc16_typed ? &as_sc16 : nullptr);
}

// the result is in pinned memory: spread it over the caller's row stride, and close the call's statistics
void finish_strided(amcx_ctx* c, StridedCall& q, bool copy_out, double t_tail) {
  if (copy_out) {
    const float* const res = c->out_pin.as<float>();
    if (q.out_row_stride == AMCX_NUM_FEATURES) {
      memcpy(q.out_host, res, sizeof(float) * AMCX_NUM_FEATURES * (size_t)q.F);
    } else {
      for (int64_t g = 0; g < q.F; ++g)
        memcpy(q.out_host + (size_t)g * (size_t)q.out_row_stride, res + (size_t)g * AMCX_NUM_FEATURES,
               sizeof(float) * AMCX_NUM_FEATURES);
    }
  }
  q.st.seconds_tail = wall_now() - t_tail;
  q.st.seconds = wall_now() - q.t_start;
  c->stats = q.st;
}

// ---- small row-major calls: one graph launch ------------------------------------------------------------------
// A per-frame loop (the reference's calculate_features per queue item, features.py:214-232) is launch-bound: copy in,
// one or two conversions / kernels, copy out, a synchronisation -- seven runtime calls around 10 us of
// GPU work.  Captured once per shape into a graph on the compute stream, a call is: stage into the pinned slot,
// hipGraphLaunch, hipStreamSynchronize.  Anything that does not fit (several chunks, planes, staging threads) and any
// failure to capture takes the general path (run_chunked): then this returns false.  True: *rc is the call's result.
// (Every buffer was reserved before this -- strided_prepare, ctx_reserve_ws -- so buffers_generation stands for all the
// addresses the nodes hold; the room behind the slot lies at a distance that the shape alone decides.)
bool run_small_graph(amcx_ctx* c, StridedCall& q, amcx::Pool& inline_pool, int* rc) {
  if (!q.rows || q.threaded || q.total_staged > q.slot || !c->graphs_ok || getenv("AMCX_NO_GRAPH") != nullptr) return false;   // one chunk
  char* pinned = c->pin.as<char>();
  char* dev = c->d_slab.as<char>();
  float* const d_out = c->d_out.as<float>();
  float* const out_pin = c->out_pin.as<float>();
  const size_t bytes = (size_t)q.n_units * (size_t)q.unit * q.esz;
  const size_t out_bytes = sizeof(float) * AMCX_NUM_FEATURES * (size_t)q.F;
  const double t0 = wall_now();
  amcx::stage_runs(inline_pool, pinned, q.src, q.map, 0, q.n_units, q.as_c128);
  q.st.seconds_staging += wall_now() - t0;
  if (q.io_error.load() != 0) { *rc = io_fail(q.io_error.load()); return true; }
  amcx_ctx::GraphKey key;
  key.frames = q.F; key.frame_size = q.N; key.variant = q.v; key.c128 = q.as_c128;
  // a few frames of complex64: the kernels read the pinned slot and write the pinned result themselves (host memory
  // from hipHostMalloc is mapped into the device's address space) -- two copy nodes fewer in the graph
  key.zero_copy = !q.converts() && bytes <= (size_t(64) << 10) && getenv("AMCX_NO_ZERO_COPY") == nullptr;
  key.generation = c->buffers_generation;
  key.mask = q.mask;
  key.sc16 = q.sc16; key.sc16_scale = q.sc16 ? q.sc16_in.scale : 0.f;
  key.iq8_kind = q.iq8 ? q.src.kind : 0; key.iq8_scale = q.iq8 ? q.sc16_in.scale : 0.f;
  amcx_ctx::SmallGraph* g = nullptr;
  for (auto& cand : c->graphs)
    if (cand.exec.x && cand.key == key) g = &cand;
  if (g != nullptr) {
    ++c->graph_hits;
  } else {
    ++c->graph_misses;
    if (c->graph_misses > 64 && c->graph_misses > 4 * c->graph_hits) c->graphs_ok = false;   // shapes keep changing
    amcx_ctx::SmallGraph& slot_g = c->graphs[c->graph_next];
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    int crc = AMCX_OK;
    hipError_t ce = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal);
    if (ce == hipSuccess && key.zero_copy) {
      crc = ctx_features(c, pinned, q.F, q.N, out_pin, q.v, q.mask, q.sc16 ? &q.sc16_in : nullptr);
      ce = hipStreamEndCapture(c->stream, &graph);
    } else if (ce == hipSuccess) {
      ce = hipMemcpyAsync(dev, pinned, bytes, hipMemcpyHostToDevice, c->stream);
      if (ce == hipSuccess) crc = chunk_features(c, q, dev, q.F, d_out, &ce);
      if (ce == hipSuccess && crc == AMCX_OK)
        ce = hipMemcpyAsync(out_pin, d_out, out_bytes, hipMemcpyDeviceToHost, c->stream);
      const hipError_t ee = hipStreamEndCapture(c->stream, &graph);      // always ends the capture
      if (ce == hipSuccess) ce = ee;
    }
    if (ce == hipSuccess && crc == AMCX_OK && graph != nullptr) ce = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (graph != nullptr) (void)hipGraphDestroy(graph);
    if (ce != hipSuccess || crc != AMCX_OK || exec == nullptr) {
      (void)hipGetLastError();
      c->graphs_ok = false;                 // the general path takes this call and every later one
      return false;
    }
    slot_g.exec.reset(exec);
    slot_g.key = key;
    c->graph_next = (c->graph_next + 1) % 4;
    g = &slot_g;
  }
  q.st.seconds_prepare = q.t_loop - q.t_start;
  const double t_tail = wall_now();
  const hipError_t e = hipGraphLaunch(g->exec.x, c->stream);
  const hipError_t e2 = hipStreamSynchronize(c->stream);
  if (e != hipSuccess || e2 != hipSuccess) {
    *rc = hip_fail(e != hipSuccess ? e : e2, "amcx_ctx_features18 (graph launch)");
    return true;
  }
  q.st.pcie_bytes = (int64_t)bytes; q.st.chunks = 1;
  finish_strided(c, q, true, t_tail);
  *rc = AMCX_OK;
  return true;
}

// ---- the general path: chunks staged by the pool, uploaded on the copy stream, computed on the compute stream ------------
int run_chunked(amcx_ctx* c, StridedCall& q, amcx::Pool& pool) {
  amcx_upload_stats& st = q.st;
  const int64_t F = q.F, unit = q.unit, n_units = q.n_units;
  const int32_t N = q.N;
  const size_t esz = q.esz, slot = q.slot;
  float* const d_out = c->d_out.as<float>();
  int rc = AMCX_OK;
  hipError_t e = hipSuccess;
  const int64_t units_per_slot = (int64_t)(slot / ((size_t)unit * esz));
  int64_t u = 0;
  for (int ch = 0; u < n_units && rc == AMCX_OK; ++ch) {
    // the first chunks are small so that the link starts early and staging overlaps it from the start:
    // 2, 2, 4, 4, 8, 8 ... MiB staged, up to whole slots (a 16 MB modulation of BASELINE configs[0] is five chunks)
    int64_t take = units_per_slot;
    if (ch < 12) {
      const int64_t ramp = (int64_t)((size_t(2) << 20 << (ch / 2)) / ((size_t)unit * esz));
      if (ramp < take) take = ramp;
    }
    if (take < 1) take = 1;
    if (take > n_units - u) take = n_units - u;
    const int ps = ch % kPinSlots, ds = ch & 1;
    char* pinned = c->pin.as<char>() + (size_t)ps * slot;
    char* dev = c->d_slab.as<char>() + (size_t)ds * q.dslot;
    const size_t bytes = (size_t)take * (size_t)unit * esz;
    if (ch >= kPinSlots) {                                  // the upload that last read this pinned slot is done
      const double t0 = wall_now();
      e = hipEventSynchronize(c->up_done[ps]);
      st.seconds_waiting += wall_now() - t0;
      if (e != hipSuccess) break;
    }
    {
      const double t0 = wall_now();
      // rows: run = frame g; planes: a plane is map.cnt_b runs
      const int64_t per_unit = q.rows ? 1 : q.map.cnt_b;
      amcx::stage_runs(pool, pinned, q.src, q.map, u * per_unit, (u + take) * per_unit, q.as_c128);
      st.seconds_staging += wall_now() - t0;
      if (q.io_error.load() != 0) {                        // nothing of this chunk is queued; what is in flight is drained below
        rc = io_fail(q.io_error.load());
        break;
      }
    }
    if (ch >= 2) { e = hipStreamWaitEvent(c->copy_stream, c->slab_free[ds], 0); if (e != hipSuccess) break; }
    e = hipMemcpyAsync(dev, pinned, bytes, hipMemcpyHostToDevice, c->copy_stream);
    if (e != hipSuccess) break;
    e = hipEventRecord(c->up_done[ps], c->copy_stream);
    if (e != hipSuccess) break;
    e = hipStreamWaitEvent(c->stream, c->up_done[ps], 0);
    if (e != hipSuccess) break;
    st.pcie_bytes += (int64_t)bytes;
    if (q.rows) {
      rc = chunk_features(c, q, dev, take, d_out + (size_t)u * AMCX_NUM_FEATURES, &e);
      if (e != hipSuccess) break;
    } else {
      float2* frames = c->d_frames.as<float2>();
      const int S = (int)q.S, inner = q.inner_snr ? 1 : 0;
      e = q.as_c128 ? amcx::launch_pack_planes(reinterpret_cast<const double2*>(dev), (int)take, (long long)F, (long long)F,
                                               S, (long long)q.K, inner, frames, (long long)N, (int)u, c->stream)
                    : amcx::launch_pack_planes(reinterpret_cast<const float2*>(dev), (int)take, (long long)F, (long long)F,
                                               S, (long long)q.K, inner, frames, (long long)N, (int)u, c->stream);
      if (e != hipSuccess) break;
    }
    if (rc != AMCX_OK) break;
    e = hipEventRecord(c->slab_free[ds], c->stream);
    if (e != hipSuccess) break;
    u += take;
    st.chunks = ch + 1;
  }
  if (rc == AMCX_OK && e == hipSuccess && !q.rows)
    rc = ctx_features(c, c->d_frames.p, F, N, d_out, q.v, q.mask);
  const double t_tail = wall_now();
  st.seconds_prepare = q.t_loop - q.t_start;
  // the result comes back into pinned memory (a copy into the caller's pageable rows would be staged by the
  // runtime, ~100 us for 72 KB) and is spread over the caller's row stride by the host
  if (rc == AMCX_OK && e == hipSuccess)
    e = hipMemcpyAsync(c->out_pin.p, d_out, sizeof(float) * AMCX_NUM_FEATURES * (size_t)F, hipMemcpyDeviceToHost, c->stream);
  if (rc == AMCX_OK && e != hipSuccess) rc = hip_fail(e, "amcx_ctx_features18_strided_host");
  // success or not, nothing of this call is in flight when it returns (every upload is ordered before the
  // compute stream's last kernel by an event, so on success that stream alone says so)
  hipError_t e2 = hipStreamSynchronize(c->stream);
  hipError_t e1 = (rc == AMCX_OK && e2 == hipSuccess) ? hipSuccess : hipStreamSynchronize(c->copy_stream);
  if (rc == AMCX_OK && (e1 != hipSuccess || e2 != hipSuccess))
    rc = hip_fail(e1 != hipSuccess ? e1 : e2, "amcx_ctx_features18_strided_host (sync)");
  finish_strided(c, q, rc == AMCX_OK, t_tail);
  return rc;
}

// src: amcx::Source::memory or ::file; src.kind is checked here, src.io_error is set here
int ctx_run_strided(amcx_ctx* c, amcx::Source src, int64_t S, int64_t K,
                    int32_t N, int64_t ss, int64_t sk, int64_t sn, float* out_host, int64_t out_row_stride,
                    int32_t variant) {
  if (c == nullptr) return AMCX_EINVAL;
  const int32_t kind = src.kind;
  if (S < 0 || K < 0 || ss < 0 || sk < 0 || sn < 0 || out_row_stride < AMCX_NUM_FEATURES ||
      !amcx::src_kind_ok(kind))
    return AMCX_EINVAL;
  const int v = resolve_variant(N, variant);
  if (v < 0) return v;
  if (amcx::src_as_it_lies(kind) && sn != 1) return AMCX_ENOTSUP;   // sc16, ci8, cu8: row layouts only
  if (S == 0 || K == 0) return AMCX_OK;
  if (S > (int64_t(1) << 40) / K) return AMCX_EINVAL;
  if ((src.fd < 0 && src.re == nullptr) || (src.fd >= 0 && src.re_off < 0) || out_host == nullptr) return AMCX_EINVAL;
  const amcx::CallGate::Token in_call = c->gate.enter();
  StridedCall q;
  q.mask = c->feature_mask.load(std::memory_order_acquire);
  src.io_error = &q.io_error;
  q.src = src;
  q.S = S; q.K = K; q.N = N; q.v = v; q.out_host = out_host; q.out_row_stride = out_row_stride;
  const int64_t F = q.F = S * K;
  if (!classify_layout(S, K, N, ss, sk, sn, &q.rows, &q.inner_snr, &q.map)) return AMCX_ENOTSUP;
  const bool rows = q.rows;
  if (!rows && S > 0x7fffffffLL) return AMCX_EINVAL;             // the transposition kernel indexes the snr axis with an int
  const bool as_c128 = q.as_c128 = c->round_on_device && kind == AMCX_SRC_C128;
  q.sc16 = kind == AMCX_SRC_SC16;
  q.iq8 = amcx::src_iq8(kind);
  q.sc16_typed = (q.sc16 || q.iq8) && sc16_typed(N, v);
  q.sc16_in.scale = (q.iq8 ? c->iq8_scale : c->sc16_scale).load(std::memory_order_acquire);
  if (q.iq8) q.sc16_in.iq8 = kind == AMCX_SRC_CU8 ? AMCX_IQ8_CU8 : AMCX_IQ8_CI8;
  const size_t esz = q.esz = amcx::staged_elem_bytes(kind, as_c128);
  const size_t src_esz = kind == AMCX_SRC_C64 ? 8 : kind == AMCX_SRC_C128 ? 16 : kind == AMCX_SRC_F32_SPLIT ? 4
                         : kind == AMCX_SRC_SC16 ? 4 : q.iq8 ? 2 : 8;
  const int64_t unit = q.unit = rows ? N : F;             // staged elements per chunk unit (a frame / a plane)
  const int64_t n_units = q.n_units = rows ? F : N;
  size_t slot = c->slot_bytes;
  const size_t total_staged = q.total_staged = (size_t)unit * esz * (size_t)n_units;
  if (slot > total_staged) slot = total_staged;                   // a per-frame call pins kilobytes, not 3 x 32 MiB
  if (slot < (size_t)unit * esz) slot = (size_t)unit * esz;       // a slot holds at least one frame / one plane
  if (slot > (size_t(4) << 30)) return AMCX_ENOMEM;               // > 4 GiB per plane: split the call by snr
  slot = (slot + 4095) & ~size_t(4095);
  q.slot = slot;

  DeviceGuard guard;
  AMCX_HIP(guard.enter(c->device));
  q.t_start = wall_now();
  // rows of complex128 rounded on the device: each device slot is followed by room for its rounded rows
  // ... rows of sc16 widened on the device by room for twice their bytes, 8-bit rows by twice (sc16) or four times (complex64)
  q.dslot = (rows && as_c128) ? slot + slot / 2 : q.iq8 ? (q.sc16_typed ? 3 : 5) * slot : (q.sc16 && !q.sc16_typed) ? 3 * slot : slot;
  const bool threaded = q.threaded = total_staged >= (size_t(1) << 20);   // below 1 MiB a condition-variable wake costs more than the copy
  // an upload worth its staging threads runs on the device's own socket, this thread included: it stages, and the pinned
  // slots strided_prepare may allocate are placed where it runs (a per-frame call is not worth two affinity system calls)
  static const std::vector<int> kNoCpus;
  amcx::AffinityGuard on_local_cpus(threaded ? c->bind_cpus : kNoCpus);
  int rc = strided_prepare(c, slot, q.dslot, rows ? 0 : (size_t)F * N * 8, sizeof(float) * AMCX_NUM_FEATURES * (size_t)F,
                           threaded);
  if (rc != AMCX_OK) return rc;
  ctx_reserve_ws(c, N, F, v);                                      // workspace and ring, before any capture below
  amcx::Pool inline_pool;                                          // size 1: stage_runs runs on the caller
  amcx::Pool& pool = threaded ? c->pool : inline_pool;
  amcx_upload_stats& st = q.st;
  st.frames = F; st.threads = pool.size(); st.plane_major = rows ? 0 : 1; st.from_file = src.fd >= 0 ? 1 : 0;
  st.source_bytes = F * (int64_t)N * (int64_t)src_esz * ((kind >= AMCX_SRC_F32_SPLIT && src.has_im()) ? 2 : 1);
  q.t_loop = wall_now();
  if (run_small_graph(c, q, pool, &rc)) return rc;
  return run_chunked(c, q, pool);
}

// the row-major host entries (amcx_ctx_features18_c64_host / _c128_host and their one-shot forms): a single-snr
// container whose frames are row_stride_elems apart -- the row path of the strided engine
int ctx_run(amcx_ctx* c, const void* iq_host, int32_t kind, int64_t n_frames, int32_t frame_size,
            int64_t row_stride_elems, float* out_host, int64_t out_row_stride, int32_t variant) {
  if (c == nullptr) return AMCX_EINVAL;
  if (n_frames < 0 || row_stride_elems < frame_size || out_row_stride < AMCX_NUM_FEATURES) return AMCX_EINVAL;
  return ctx_run_strided(c, amcx::Source::memory(iq_host, nullptr, kind), 1, n_frames, frame_size, 0, row_stride_elems, 1,
                         out_host, out_row_stride, variant);
}

int stage_any(amcx::Source src, int64_t n_snr, int64_t n_frames, int32_t frame_size, int64_t stride_snr, int64_t stride_frame,
              int64_t stride_sample, int64_t first_unit, int64_t n_units, void* dst, int64_t dst_bytes, int32_t threads,
              int32_t* plane_major, int32_t* inner_snr_out) {
  const int32_t kind = src.kind;
  if (n_snr < 0 || n_frames < 0 || stride_snr < 0 || stride_frame < 0 || stride_sample < 0 || first_unit < 0 ||
      n_units < 0 || threads < 0 || threads > 256 || !amcx::src_kind_ok(kind) ||
      frame_size < AMCX_MIN_FRAME_SIZE || frame_size > AMCX_MAX_FRAME_SIZE)
    return AMCX_EINVAL;
  if (n_frames > 0 && n_snr > (int64_t(1) << 40) / n_frames) return AMCX_EINVAL;
  bool rows = false, inner_snr = false;
  amcx::RunMap map;
  if (!classify_layout(n_snr, n_frames, frame_size, stride_snr, stride_frame, stride_sample, &rows, &inner_snr, &map))
    return AMCX_ENOTSUP;
  if (amcx::src_as_it_lies(kind) && !rows) return AMCX_ENOTSUP;    // sc16, ci8, cu8: row layouts only
  if (plane_major) *plane_major = rows ? 0 : 1;
  if (inner_snr_out) *inner_snr_out = inner_snr ? 1 : 0;
  const int64_t F = n_snr * n_frames, unit = rows ? frame_size : F, total_units = rows ? F : frame_size;
  if (first_unit + n_units > total_units) return AMCX_EINVAL;
  if (n_units == 0 || unit == 0) return AMCX_OK;
  if ((src.fd < 0 && src.re == nullptr) || dst == nullptr ||
      dst_bytes < n_units * unit * (int64_t)amcx::staged_elem_bytes(kind, false))
    return AMCX_EINVAL;
  std::atomic<int> io_error{0};
  src.io_error = &io_error;
  amcx::Pool pool;
  pool.resize(threads < 1 ? 1 : threads);
  const int64_t per_unit = rows ? 1 : map.cnt_b;
  amcx::stage_runs(pool, static_cast<char*>(dst), src, map, first_unit * per_unit, (first_unit + n_units) * per_unit, false);
  if (io_error.load() != 0) return io_fail(io_error.load());
  return AMCX_OK;
}

// one-shot forms: a context for the duration of the call
int one_shot(const void* iq_host, bool is_c128, int64_t n_frames, int32_t frame_size, int64_t row_stride_elems,
             float* out_host, int64_t out_row_stride, int32_t device, int32_t variant) {
  // argument errors are reported before a device is looked for (tests/test_host_cpu.py runs without one)
  if (n_frames < 0 || row_stride_elems < frame_size || out_row_stride < AMCX_NUM_FEATURES)
    return AMCX_EINVAL;
  const int v = resolve_variant(frame_size, variant);
  if (v < 0) return v;
  if (n_frames == 0) return AMCX_OK;
  if (iq_host == nullptr || out_host == nullptr) return AMCX_EINVAL;
  amcx_ctx* c = nullptr;
  int rc = amcx_ctx_create(device, &c);
  if (rc != AMCX_OK) return rc;
  rc = ctx_run(c, iq_host, is_c128 ? AMCX_SRC_C128 : AMCX_SRC_C64, n_frames, frame_size, row_stride_elems, out_host, out_row_stride, v);
  (void)amcx_ctx_destroy(c);
  return rc;
}

}  // namespace
