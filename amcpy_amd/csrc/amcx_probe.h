// The two probes of libamcx.so (include/amcx.h: amcx_probe_fma_rate, amcx_probe_read_bw): what the board does at the
// instruction-issue and at the HBM-read ceiling, for bench.py's roofline.  amcx.hip includes this behind every kernel header:
// plain kernels lie in .text in the order of their definitions (amcx_sc16_kernels.h), and these two were always the last.
#pragma once

namespace {

// The instruction-issue ceiling under the board's power cap: 16 wavefronts per CU (4 per SIMD, the N = 2048 kernel's
// occupancy), each running `iters` trips of 32 independent v_fma_f32 (8 chains x 4) on registers -- no memory traffic.
// Lane 0 of every wave leaves its shader-clock cycles and its 100 MHz real-time ticks, from which the clock follows.
__global__ __launch_bounds__(1024) void amcx_probe_fma_kernel(int iters, float* sink, unsigned long long* ticks) {
  float a0 = (float)threadIdx.x, a1 = a0 + 1.f, a2 = a0 + 2.f, a3 = a0 + 3.f, a4 = a0 + 4.f, a5 = a0 + 5.f,
        a6 = a0 + 6.f, a7 = a0 + 7.f;
  const float b0 = 1.0001f, b1 = 0.9999f;
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      asm volatile(
          "v_fma_f32 %0, %0, %8, %9\n v_fma_f32 %1, %1, %8, %9\n v_fma_f32 %2, %2, %8, %9\n v_fma_f32 %3, %3, %8, %9\n"
          "v_fma_f32 %4, %4, %8, %9\n v_fma_f32 %5, %5, %8, %9\n v_fma_f32 %6, %6, %8, %9\n v_fma_f32 %7, %7, %8, %9\n"
          : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b0), "v"(b1));
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  const unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
  const float s = ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7));
  if (s == 12345.678f) sink[0] = s;                       // keeps the chains alive; never true in practice
  if ((threadIdx.x & 63) == 0) {
    const long long w = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    ticks[2 * w] = t1 - t0;
    ticks[2 * w + 1] = r1 - r0;
  }
}

__global__ __launch_bounds__(256) void amcx_probe_read_kernel(const float4* __restrict__ src,
                                                             long long n_vec, float* partial) {
  typedef float v4f __attribute__((ext_vector_type(4)));
  float acc = 0.f;
  const long long stride = (long long)gridDim.x * blockDim.x;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  // four independent 16-byte loads in flight per lane and iteration
  for (; i + 3 * stride < n_vec; i += 4 * stride) {
    const v4f a = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(src + i));
    const v4f b = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(src + i + stride));
    const v4f c = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(src + i + 2 * stride));
    const v4f d = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(src + i + 3 * stride));
    acc += ((a.x + a.y) + (a.z + a.w)) + ((b.x + b.y) + (b.z + b.w)) + ((c.x + c.y) + (c.z + c.w)) +
           ((d.x + d.y) + (d.z + d.w));
  }
  for (; i < n_vec; i += stride) {
    const float4 v = src[i];
    acc += (v.x + v.y) + (v.z + v.w);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
  __shared__ float s[4];
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (s[0] + s[1]) + (s[2] + s[3]);
}

}  // namespace

extern "C" {

int amcx_probe_fma_rate(double seconds, void* hip_stream, double* wave_instr_per_s, double* clock_ghz) {
  if (!(seconds > 0.0) || seconds > 60.0 || wave_instr_per_s == nullptr) return AMCX_EINVAL;
  *wave_instr_per_s = 0.0;
  if (clock_ghz) *clock_ghz = 0.0;
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const int grid = cu_count();
  if (grid <= 0) return AMCX_ENODEV;
  const long long n_waves = (long long)grid * 16;
  constexpr int kIters = 32768;                            // x 32 instructions x 4096 waves: ~5 ms a launch
  DeviceBuffer sink_buf, ticks_buf;
  Event e0, e1, e2;
  hipError_t e = sink_buf.reserve(4) == AMCX_OK && ticks_buf.reserve((size_t)n_waves * 16) == AMCX_OK ? hipSuccess
                                                                                                      : hipErrorOutOfMemory;
  for (Event* ev : {&e0, &e1, &e2})
    if (e == hipSuccess) e = ev->create(hipEventDefault);
  if (e != hipSuccess) return hip_fail(e, "fma probe setup");
  float* const sink = sink_buf.as<float>();
  unsigned long long* const ticks = ticks_buf.as<unsigned long long>();
  // (the one raw launch of the library, amcx_launch.h: the error is asked for once, behind the timed launches)
  auto launch = [&]() { hipLaunchKernelGGL(amcx_probe_fma_kernel, dim3((unsigned)grid), dim3(1024), 0, stream, kIters, sink, ticks); };
  // one launch to learn its length, then `seconds` of back-to-back launches: the first half lets the board's power
  // management settle the clock, the second half is timed
  (void)hipEventRecord(e0, stream);
  launch();
  (void)hipEventRecord(e1, stream);
  e = hipEventSynchronize(e1);
  float one_ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&one_ms, e0, e1);
  if (e != hipSuccess) return hip_fail(e, "fma probe launch");
  if (!(one_ms > 0.01f)) one_ms = 0.01f;
  long long n = (long long)(seconds * 1e3 / 2.0 / one_ms);
  if (n < 1) n = 1;
  if (n > 100000) n = 100000;
  for (long long i = 0; i < n; ++i) launch();
  (void)hipEventRecord(e1, stream);
  for (long long i = 0; i < n; ++i) launch();
  (void)hipEventRecord(e2, stream);
  e = hipEventSynchronize(e2);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e1, e2);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess || !(ms > 0.f)) return hip_fail(e, "fma probe timing");
  *wave_instr_per_s = (double)n * (double)n_waves * (double)kIters * 32.0 / ((double)ms * 1e-3);
  if (clock_ghz == nullptr) return AMCX_OK;
  std::vector<unsigned long long> h((size_t)n_waves * 2);
  e = hipMemcpy(h.data(), ticks, h.size() * 8, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hip_fail(e, "fma probe read-back");
  double cyc = 0.0, real = 0.0;
  for (long long w = 0; w < n_waves; ++w) { cyc += (double)h[(size_t)(2 * w)]; real += (double)h[(size_t)(2 * w + 1)]; }
  if (real > 0.0) *clock_ghz = cyc / (real * 10.0);       // s_memrealtime ticks at 100 MHz
  return AMCX_OK;
}

int amcx_probe_read_bw(const void* src_dev, int64_t n_bytes, float* partial_dev, void* hip_stream) {
  if (src_dev == nullptr || partial_dev == nullptr || n_bytes < 0 || (n_bytes & 15)) return AMCX_EINVAL;
  if (n_bytes == 0) return AMCX_OK;
  const hipError_t e = amcx::launch(amcx_probe_read_kernel, 4096, 256, 0, static_cast<hipStream_t>(hip_stream),
                                    static_cast<const float4*>(src_dev), n_bytes / 16, partial_dev);
  if (e != hipSuccess) return hip_fail(e, "read probe kernel launch");
  return AMCX_OK;
}

}  // extern "C"
