// Occupancy detection on a (channel x frame) grid (include/amcx.h, ABI 14): the power of every cell, a noise floor per frame,
// the occupied cells as a mask and as an ascending row list, and the copy that packs those rows for the feature kernels.
// A CELL is one frame of N complex64 samples of one channel: row r = c K + k of the (C K, N) matrix the filter bank's output
// is cut into.
//
// ROW POWER (amcx_row_power_kernel).  power[r] = sum_{n < N} re^2 + im^2 in float32.  One wavefront per row at a time, rows
// dealt to the waves of a persistent grid.  A lane reads 16 bytes per load: the sample PAIR q = (samples 2 q, 2 q + 1) goes to
// lane q mod 64, in its round i = q / 64; four loads are in flight per lane; every input byte is read once (non-temporal).
//   THE ORDER, which depends on N alone:
//     lane j:  s_j = 0;  for i = 0, 1, ... while q = j + 64 i < floor(N / 2):
//                  s_j = fma(im, im, fma(re, re, s_j)) of sample 2 q, then the same of sample 2 q + 1
//              N odd: the last sample N - 1 is added the same way by lane floor(N / 2) mod 64, after that lane's pairs
//     tree:    6 levels, d = 32, 16, 8, 4, 2, 1:  s_j = s_j + s_{j xor d}   (every lane ends with the same bits: + commutes)
//   A lane that holds no sample contributes +0, which changes no bit of a sum of non-negative terms, NaN or Inf.
//   A row that does not begin on 16 bytes (a base that is only 8-byte aligned, an odd stride) is read as 8-byte-aligned halves
//   of the same pairs into the same registers: the same bits.  (hipcc fuses the two halves into one 16-byte access at 8-byte
//   alignment, which global memory on gfx950 allows; an odd last sample, at a wave-uniform address, comes through a scalar
//   load.)  Nothing outside [row, row + N) is read.
//   Roundings on the longest path from a term to the sum: 4 per pair, ceil(N / 128) pairs per lane at the most, 6 levels:
//   4 ceil(N / 128) + 6 <= B = 4 ceil(N / 128) + 8 (tests/occupancy_ref.py).
//
// DETECTION, four launches on one stream (no workgroup ever waits for another; ordinary vector stores; no atomics):
//   amcx_occupancy_detect_kernel   tiles of 64 frames (lanes walk k: the reads of power[c K + k] coalesce): floor[k] = the
//                                  element of rank `rank` of the C values, NaN last.  The rank is found on the values' ordered
//                                  32-bit keys by bisection, bit 31 down to 0: the largest x with #{key < x} <= rank IS the
//                                  key of that element.  The keys are read once into LDS; every step counts in LDS, the four
//                                  waves a quarter of the channels each.  No sort, any C.
//   amcx_occupancy_count_kernel    blocks of 256 consecutive rows r: occupied = power[r] > threshold * floor[r mod K] (one
//                                  float32 product, one comparison: a NaN is not occupied), the mask, the block's count.
//   amcx_occupancy_scan_kernel     ONE workgroup: the exclusive scan of the block counts in place, the total to *count.
//   amcx_occupancy_scatter_kernel  the same blocks again: rows[offset of the block + rank inside it] = r -- ascending.
//
// ROW GATHER (amcx_gather_rows_kernel).  dst row i = src row index[i]; a wave per row, 16-byte accesses where both rows begin
// on 16 bytes and 8-byte otherwise; an index outside [0, n_src_rows) gives a row of NaN and reads nothing.
//
// KERNEL ORDER (amcx_launch.h): plain kernels in the header amcx.hip includes FIRST, in front of the resampler's: every kernel
// that was there keeps its bytes (tools/codeobj_gate.py --kernels, profiles/r21_occupancy_codeobj_kernels.txt).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace amcx {

constexpr int kOccThreads = 256;
constexpr int kOccWaves = kOccThreads / 64;
constexpr int kOccBlockRows = 256;          // rows of one block of the count / scatter launches: one per thread
constexpr int kOccMaxChannels = 256;
constexpr int kOccTileFrames = 64;          // frames of one tile of the floor launch: one per lane

typedef float occ_v4f __attribute__((ext_vector_type(4)));
typedef float occ_v2f __attribute__((ext_vector_type(2)));

// sample pair q of a row: one 16-byte load, or two 8-byte loads of the same samples
template <bool ALIGNED16>
__device__ __forceinline__ occ_v4f occ_load_pair(const float2* __restrict__ row, int q) {
  if constexpr (ALIGNED16) {
    return __builtin_nontemporal_load(reinterpret_cast<const occ_v4f*>(row) + q);
  } else {
    const occ_v2f a = __builtin_nontemporal_load(reinterpret_cast<const occ_v2f*>(row) + 2 * q);
    const occ_v2f b = __builtin_nontemporal_load(reinterpret_cast<const occ_v2f*>(row) + 2 * q + 1);
    occ_v4f v;
    v.x = a.x; v.y = a.y; v.z = b.x; v.w = b.y;
    return v;
  }
}

__device__ __forceinline__ float occ_add_pair(float s, occ_v4f v) {
  s = __builtin_fmaf(v.y, v.y, __builtin_fmaf(v.x, v.x, s));
  return __builtin_fmaf(v.w, v.w, __builtin_fmaf(v.z, v.z, s));
}

// lane `lane`'s share of a row (THE ORDER above)
template <bool ALIGNED16>
__device__ __forceinline__ float occ_lane_sum(const float2* __restrict__ row, int N, int lane) {
  const int n_pairs = N >> 1;
  float s = 0.0f;
  int q = lane;
  for (; q + 3 * 64 < n_pairs; q += 4 * 64) {               // four loads in flight, added in ascending q
    const occ_v4f a = occ_load_pair<ALIGNED16>(row, q);
    const occ_v4f b = occ_load_pair<ALIGNED16>(row, q + 64);
    const occ_v4f c = occ_load_pair<ALIGNED16>(row, q + 128);
    const occ_v4f d = occ_load_pair<ALIGNED16>(row, q + 192);
    s = occ_add_pair(occ_add_pair(occ_add_pair(occ_add_pair(s, a), b), c), d);
  }
  for (; q < n_pairs; q += 64) s = occ_add_pair(s, occ_load_pair<ALIGNED16>(row, q));
  if ((N & 1) != 0 && lane == (n_pairs & 63)) {              // the odd sample N - 1: its lane's last term
    const occ_v2f a = __builtin_nontemporal_load(reinterpret_cast<const occ_v2f*>(row) + (N - 1));
    s = __builtin_fmaf(a.y, a.y, __builtin_fmaf(a.x, a.x, s));
  }
  return s;
}

// Reads src[r stride .. r stride + N) for r < n_rows, writes power[0 .. n_rows), nothing else.
__global__ __launch_bounds__(kOccThreads) void amcx_row_power_kernel(const float2* __restrict__ src, long long n_rows, int N,
                                                                     long long stride, float* __restrict__ power) {
  const int lane = (int)threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const long long n_waves = (long long)gridDim.x * kOccWaves;
  for (long long r = (long long)blockIdx.x * kOccWaves + wave; r < n_rows; r += n_waves) {
    const float2* const row = src + r * stride;
    float s = (reinterpret_cast<uintptr_t>(row) & 15u) == 0 ? occ_lane_sum<true>(row, N, lane) : occ_lane_sum<false>(row, N, lane);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s = s + __shfl_xor(s, d, 64);
    if (lane == 0) power[r] = s;
  }
}

// a float32's place in ascending order as an unsigned key: -inf ... -0 < +0 ... +inf < every NaN
__device__ __forceinline__ unsigned occ_key(float p) {
  const unsigned u = __float_as_uint(p);
  if (p != p) return 0xFFFFFFFFu;
  return (u & 0x80000000u) != 0 ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float occ_unkey(unsigned key) {
  if (key == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
  return __uint_as_float((key & 0x80000000u) != 0 ? (key & 0x7FFFFFFFu) : ~key);
}

// dynamic LDS of the floor launch: the tile's keys [C][64], then two buffers of the four waves' partial counts
__host__ __device__ __forceinline__ size_t occ_detect_lds_bytes(int C) {
  return (size_t)C * kOccTileFrames * sizeof(unsigned) + (size_t)2 * kOccWaves * kOccTileFrames * sizeof(int);
}

// Reads power[0 .. C K), writes floor_out[0 .. K).  0 <= rank < C; n_tiles = ceil(K / 64); dynamic LDS occ_detect_lds_bytes(C).
// A workgroup takes a TILE of 64 consecutive frames: lane l of every wave stands for frame 64 tile + l, wave w for the channels
// c = w, w + 4, ...  The keys are staged once (global reads coalesce over k, LDS bank = lane: no conflict); every bisection
// step counts a wave's share from LDS and sums the four shares through LDS -- one barrier per step, the partials double-buffered.
__global__ __launch_bounds__(kOccThreads) void amcx_occupancy_detect_kernel(const float* __restrict__ power, int C, long long K,
                                                                            int rank, float* __restrict__ floor_out,
                                                                            long long n_tiles) {
  extern __shared__ __attribute__((aligned(16))) unsigned occ_lds[];
  unsigned* const keys = occ_lds;
  int* const part = reinterpret_cast<int*>(occ_lds + (size_t)C * kOccTileFrames);
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long k = tile * kOccTileFrames + lane;
    const bool live = k < K;
    for (int c = wave; c < C; c += kOccWaves) keys[c * kOccTileFrames + lane] = live ? occ_key(power[(long long)c * K + k]) : 0xFFFFFFFFu;
    __syncthreads();
    unsigned ans = 0;
    for (int bit = 31; bit >= 0; --bit) {
      const unsigned cand = ans | (1u << bit);
      int below = 0;
      for (int c = wave; c < C; c += kOccWaves) below += keys[c * kOccTileFrames + lane] < cand ? 1 : 0;
      int* const mine = part + (bit & 1) * (kOccWaves * kOccTileFrames);
      mine[wave * kOccTileFrames + lane] = below;
      __syncthreads();
      const int total = (mine[lane] + mine[kOccTileFrames + lane]) + (mine[2 * kOccTileFrames + lane] + mine[3 * kOccTileFrames + lane]);
      if (total <= rank) ans = cand;                                // (every wave decides the same: the same four partials)
    }
    if (wave == 0 && live) floor_out[k] = occ_unkey(ans);
    __syncthreads();                                                // the next tile's keys overwrite what was just counted
  }
}

__device__ __forceinline__ bool occ_occupied(const float* __restrict__ power, const float* __restrict__ floor_k, unsigned K,
                                             float threshold, long long r) {
  return power[r] > threshold * floor_k[(unsigned)r % K];
}

// Block b holds the rows [256 b, 256 b + 256) below n_cells: mask[r] where wanted, counts[b] where wanted.
__global__ __launch_bounds__(kOccThreads) void amcx_occupancy_count_kernel(const float* __restrict__ power,
                                                                           const float* __restrict__ floor_k, unsigned K,
                                                                           long long n_cells, float threshold,
                                                                           unsigned char* __restrict__ mask, int* __restrict__ counts,
                                                                           long long n_blocks) {
  __shared__ int wave_sum[kOccWaves];
  const int tid = (int)threadIdx.x;
  for (long long b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const long long r = b * kOccBlockRows + tid;
    bool occ = false;
    if (r < n_cells) {
      occ = occ_occupied(power, floor_k, K, threshold, r);
      if (mask != nullptr) mask[r] = occ ? 1 : 0;
    }
    if (counts == nullptr) continue;
    const unsigned long long bal = __ballot(occ);
    if ((tid & 63) == 0) wave_sum[tid >> 6] = __popcll(bal);
    __syncthreads();
    if (tid == 0) counts[b] = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
    __syncthreads();
  }
}

// ONE workgroup: counts[0 .. n_blocks) -> its exclusive scan, in place; *total = the sum.
__global__ __launch_bounds__(kOccThreads) void amcx_occupancy_scan_kernel(int* __restrict__ counts, long long n_blocks,
                                                                          int* __restrict__ total) {
  __shared__ int wave_tot[kOccWaves];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0;
  for (long long base = 0; base < n_blocks; base += kOccThreads) {
    const long long i = base + tid;
    const int v = i < n_blocks ? counts[i] : 0;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(inc, d, 64);
      if (lane >= d) inc += t;
    }
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kOccWaves; ++w) {
      if (w < wave) before += wave_tot[w];
      all += wave_tot[w];
    }
    if (i < n_blocks) counts[i] = carry + before + (inc - v);
    carry += all;
    __syncthreads();
  }
  if (tid == 0) *total = carry;
}

// offsets: the scanned block counts.  rows[offsets[b] + the rank of r among the block's occupied rows] = r.
__global__ __launch_bounds__(kOccThreads) void amcx_occupancy_scatter_kernel(const float* __restrict__ power,
                                                                             const float* __restrict__ floor_k, unsigned K,
                                                                             long long n_cells, float threshold,
                                                                             const int* __restrict__ offsets, int* __restrict__ rows,
                                                                             long long n_blocks) {
  __shared__ int wave_sum[kOccWaves];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (long long b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const long long r = b * kOccBlockRows + tid;
    const bool occ = r < n_cells && occ_occupied(power, floor_k, K, threshold, r);
    const unsigned long long bal = __ballot(occ);
    if (lane == 0) wave_sum[wave] = __popcll(bal);
    __syncthreads();
    if (occ) {
      int at = offsets[b] + __popcll(bal & ((1ull << lane) - 1ull));
#pragma unroll
      for (int w = 0; w < kOccWaves; ++w)
        if (w < wave) at += wave_sum[w];
      rows[at] = (int)r;
    }
    __syncthreads();
  }
}

// dst[i dst_stride + n] = src[index[i] stride + n], n < N; an index outside [0, n_src_rows): NaN + NaN j, nothing read.
__global__ __launch_bounds__(kOccThreads) void amcx_gather_rows_kernel(const float2* __restrict__ src, long long n_src_rows, int N,
                                                                       long long stride, const int* __restrict__ index,
                                                                       long long n_index, float2* __restrict__ dst,
                                                                       long long dst_stride) {
  const int lane = (int)threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const long long n_waves = (long long)gridDim.x * kOccWaves;
  const int n_pairs = N >> 1;
  const float nan = __uint_as_float(0x7FC00000u);
  for (long long i = (long long)blockIdx.x * kOccWaves + wave; i < n_index; i += n_waves) {
    const long long from = index[i];
    float2* const to = dst + i * dst_stride;
    const bool to16 = (reinterpret_cast<uintptr_t>(to) & 15u) == 0;
    if (from < 0 || from >= n_src_rows) {
      if (to16) {
        for (int q = lane; q < n_pairs; q += 64) reinterpret_cast<float4*>(to)[q] = make_float4(nan, nan, nan, nan);
      } else {
        for (int q = lane; q < n_pairs; q += 64) { to[2 * q] = make_float2(nan, nan); to[2 * q + 1] = make_float2(nan, nan); }
      }
      if ((N & 1) != 0 && lane == 0) to[N - 1] = make_float2(nan, nan);
      continue;
    }
    const float2* const row = src + from * stride;
    if (to16 && (reinterpret_cast<uintptr_t>(row) & 15u) == 0) {
#pragma unroll 4
      for (int q = lane; q < n_pairs; q += 64) reinterpret_cast<float4*>(to)[q] = reinterpret_cast<const float4*>(row)[q];
    } else {
#pragma unroll 4
      for (int q = lane; q < n_pairs; q += 64) {
        const float2 a = row[2 * q], b = row[2 * q + 1];
        to[2 * q] = a;
        to[2 * q + 1] = b;
      }
    }
    if ((N & 1) != 0 && lane == 0) to[N - 1] = row[N - 1];
  }
}

}  // namespace amcx
