// The kernels that widen 8-bit IQ (include/amcx.h, amcx_features_iq8; ABI 10) on the device: ci8 / cu8 rows -> packed rows of
// sc16 (where the frame size has sc16 kernels: they run next, amcx_sc16_kernels.h) or of complex64 (everywhere else).  No
// feature kernel reads 8-bit samples: the sc16 kernels bought nothing over complex64 on resident data (README, sc16 table),
// a lane's load would halve again, and what 8 bits buy is the link -- 2 bytes per sample cross it, this pass does the rest.
//
// A sample is two bytes, I then Q.  component = (int8)(byte ^ flip): flip 0x00 for ci8 (the bytes are int8), 0x80 for cu8
// (uint8 around the zero level 128).  To sc16 that is sign extension, nothing else; to complex64 it is
// (float)component * scale, ONE float32 multiplication, exactly what amcx_sc16_to_c64_kernel and the sc16 loader do with the
// sign-extended int16 -- so the features of the widened rows equal amcx_features_sc16's on int16(x) bit for bit.
//
// TWO PATHS, THE SAME BYTES.  A work item is 8 consecutive samples of one row (the last item of a row: what is left of it).
//   vector : the lane loads the item's 16 bytes at once and stores 32 (sc16) / 64 (complex64) with 16-byte stores;
//   general: the lane goes through the item one sample per step, 2-byte loads, 4- / 8-byte stores -- any 2-byte-aligned
//            base, any row stride.
// iq8_vector_row is the one predicate: an item takes the vector path iff it is a whole 8 samples and its row starts on 16
// bytes on BOTH sides (then every item of the row does: 16 / 32 / 64 bytes each).  Rows of one launch may differ
// (an odd row stride: every 8th row is aligned), and so do the lanes of one wave then.
//
// KERNEL ORDER (amcx_launch.h): plain kernels, defined in the header amcx.hip includes FIRST, so they stand at the head of
// .text, in front of the sc16 kernels, and every kernel that was there before keeps its distance to every other --
// tools/codeobj_gate.py --kernels, profiles/r14_iq8_codeobj_kernels.txt.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace amcx {

constexpr int kIq8Item = 8;        // samples per work item: 16 source bytes

__device__ __forceinline__ bool iq8_vector_row(const uint8_t* src_row, const void* dst_row) {
  return ((reinterpret_cast<uintptr_t>(src_row) | reinterpret_cast<uintptr_t>(dst_row)) & 15u) == 0;
}

// byte k (0 ... 3) of w, sign-extended
__device__ __forceinline__ int iq8_byte(unsigned w, int k) { return (int)(w << (24 - 8 * k)) >> 24; }

// one sample out: sc16 as it is, complex64 times scale
__device__ __forceinline__ void iq8_put(short2* dst, int i, int q, float) { *dst = make_short2((short)i, (short)q); }
__device__ __forceinline__ void iq8_put(float2* dst, int i, int q, float scale) {
  *dst = make_float2((float)i * scale, (float)q * scale);
}

// the two samples of one source word (flipped already) as two sc16 samples / two complex64 samples
__device__ __forceinline__ uint2 iq8_pair_sc16(unsigned w) {
  return make_uint2(((unsigned)iq8_byte(w, 0) & 0xffffu) | ((unsigned)iq8_byte(w, 1) << 16),
                    ((unsigned)iq8_byte(w, 2) & 0xffffu) | ((unsigned)iq8_byte(w, 3) << 16));
}
__device__ __forceinline__ float4 iq8_pair_c64(unsigned w, float scale) {
  return make_float4((float)iq8_byte(w, 0) * scale, (float)iq8_byte(w, 1) * scale, (float)iq8_byte(w, 2) * scale,
                     (float)iq8_byte(w, 3) * scale);
}

__device__ __forceinline__ void iq8_put_item(short2* dst, uint4 v, float) {
  const uint2 a = iq8_pair_sc16(v.x), b = iq8_pair_sc16(v.y), c = iq8_pair_sc16(v.z), d = iq8_pair_sc16(v.w);
  uint4* const o = reinterpret_cast<uint4*>(dst);
  o[0] = make_uint4(a.x, a.y, b.x, b.y);
  o[1] = make_uint4(c.x, c.y, d.x, d.y);
}
__device__ __forceinline__ void iq8_put_item(float2* dst, uint4 v, float scale) {
  float4* const o = reinterpret_cast<float4*>(dst);
  o[0] = iq8_pair_c64(v.x, scale);
  o[1] = iq8_pair_c64(v.y, scale);
  o[2] = iq8_pair_c64(v.z, scale);
  o[3] = iq8_pair_c64(v.w, scale);
}

// dst[f][n] = sample n of row f, n < N: rows of src are src_stride SAMPLES (2 bytes) apart, rows of dst are packed.  Reads
// the first N samples of every row and nothing else; writes dst[0 .. n_frames * N) and nothing else.
template <class D>
__device__ __forceinline__ void iq8_widen(const uint8_t* __restrict__ src, long long n_frames, int N, long long src_stride,
                                          unsigned flip, float scale, D* __restrict__ dst) {
  const int items = (N + kIq8Item - 1) / kIq8Item;           // per row
  const long long total = n_frames * items;
  const unsigned flip4 = (flip & 0xffu) * 0x01010101u;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long f = i / items;
    const int n0 = (int)(i - f * items) * kIq8Item;
    const uint8_t* const row = src + 2 * f * src_stride;
    D* const out = dst + f * N;
    if (n0 + kIq8Item <= N && iq8_vector_row(row, out)) {
      uint4 v = *reinterpret_cast<const uint4*>(row + 2 * n0);
      v.x ^= flip4; v.y ^= flip4; v.z ^= flip4; v.w ^= flip4;
      iq8_put_item(out + n0, v, scale);
    } else {
      const int n1 = n0 + kIq8Item < N ? n0 + kIq8Item : N;
      for (int n = n0; n < n1; ++n) {
        const unsigned w = *reinterpret_cast<const unsigned short*>(row + 2 * n) ^ flip4;
        iq8_put(out + n, iq8_byte(w, 0), iq8_byte(w, 1), scale);
      }
    }
  }
}

__global__ __launch_bounds__(256) void amcx_iq8_to_sc16_kernel(const uint8_t* __restrict__ src, long long n_frames, int N,
                                                              long long src_stride, unsigned flip,
                                                              short2* __restrict__ dst) {
  iq8_widen(src, n_frames, N, src_stride, flip, 1.0f, dst);
}

__global__ __launch_bounds__(256) void amcx_iq8_to_c64_kernel(const uint8_t* __restrict__ src, long long n_frames, int N,
                                                             long long src_stride, unsigned flip, float scale,
                                                             float2* __restrict__ dst) {
  iq8_widen(src, n_frames, N, src_stride, flip, scale, dst);
}

}  // namespace amcx
