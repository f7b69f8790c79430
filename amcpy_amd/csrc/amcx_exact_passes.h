// The arithmetic of the accuracy-first kernels, stated once: amcx_block_kernel.h (N <= 8192, the frame staged in LDS)
// and amcx_stream_kernel.h (8192 < N <= 32768, the frame left in global memory) compute features 2 ... 18 with the SAME
// operations in the same order, and no frame size runs both, so nothing but this header holds them together.  What
// stands here are leaf routines and the BODIES of the passes over a frame; the loops over n stay in each kernel (a loop
// lifted into a function that takes the body changed the six kernels' machine code in every spelling tried).
// No kernel stands here, so including it moves nothing in .text (KERNEL ORDER, amcx_launch.h).
// Every routine is spelled so that the kernels' machine code is what it was with the text written out in place
// (tools/codeobj_gate.py --kernels): where a signature looks odd -- results through references, parameters by
// reference, values taken as the caller's float -- the plainer one changed the order of some kernel's instructions.
//
// Deliberately NOT here, because their arithmetic differs and sharing it would change output bits: the block kernel's
// power-of-two FFT (its table holds (cs, +sn) and its butterfly is written for that), its N <= 64 form (envelope, angle
// and step in fp64) and both kernels' block_sum (4 waves: every thread adds; 16 waves: K threads add, through LDS).
#pragma once

#include "amcx_math.h"

namespace amcx {

// ---- reductions -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Maximum over a workgroup of WAVES waves (barriers inside; scratch: 2 * WAVES floats).  A NaN must survive the
// reduction: fmaxf drops it, so a flag is carried.
template <int WAVES>
__device__ __forceinline__ float workgroup_max(float v, double* scratch) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float bad = (v == v) ? 0.f : 1.f;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    v = __builtin_fmaxf(v, __shfl_xor(v, off, 64));
    bad = __builtin_fmaxf(bad, __shfl_xor(bad, off, 64));
  }
  float* s = reinterpret_cast<float*>(scratch);
  if (lane == 0) { s[wave * 2] = v; s[wave * 2 + 1] = bad; }
  __syncthreads();
  float m = s[0], b = s[1];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) { m = __builtin_fmaxf(m, s[w * 2]); b = __builtin_fmaxf(b, s[w * 2 + 1]); }
  __syncthreads();
  return b > 0.f ? __builtin_nanf("") : m;
}

// ---- the frame's scale ------------------------------------------------------------------------------------------------
// A frame is taken times 2^-ex, ex the even-rounded exponent of its largest component mx (exact; 0 for ordinary data up
// to a factor < 4, and for a frame that holds a NaN, an infinity or nothing above 2^-125), and the finaliser un-scales in
// fp64 through the features' scaling laws: every fp32 intermediate (|x|^2, the spectrum) then stays inside float32 for
// any normal float32 input, as the reference's complex128 evaluation does (features.py:46-58).
__device__ __forceinline__ int frame_exponent(float mx) {
  int ex = 0;
  if (mx >= 0x1p-125f && mx <= 3.4028235e38f) ex = (((__builtin_bit_cast(int, mx) >> 23) & 0xff) - 127) & ~1;
  return ex;
}

// ---- the bodies of the passes over a frame ----------------------------------------------------------------------------
// Pass A: one sample's terms of the 15 mixed-moment sums, in FrameSums' order.
__device__ __forceinline__ void moment_terms(float2 x, double (&m)[15]) {
  const double re = x.x, im = x.y;
  const double A = re * re - im * im, Bh = re * im, P = re * re + im * im;
  const double AA = A * A, BB = Bh * Bh, AP = A * P;
  m[0] += A; m[1] += Bh; m[2] += P;
  const double X4 = AA - 4.0 * BB;
  m[3] += AA; m[4] += X4; m[5] += A * Bh;
  m[6] += AP; m[7] += Bh * P;
  m[8] += AA * A; m[9] += A * BB; m[10] += AA * Bh; m[11] += BB * Bh;
  m[12] += AA * P; m[13] += X4 * P; m[14] += AP * Bh;
}
__device__ __forceinline__ void put_moments(FrameSums& S, const double (&m)[15]) {
  S.sA = m[0]; S.sBh = m[1]; S.sP = m[2]; S.sAA = m[3]; S.sX4 = m[4]; S.sAB = m[5];
  S.sAP = m[6]; S.sBP = m[7]; S.sAAA = m[8]; S.sABB = m[9]; S.sAAB = m[10]; S.sBBB = m[11];
  S.sAAP = m[12]; S.sX4P = m[13]; S.sABP = m[14];
}

// Pass B: one sample's envelope va and angle vth (float, or double where the caller took them in fp64) about the
// envelope's mean mu and the shifts Kt, Ka.  c[5], the first sum of the phase steps, is the caller's.
template <class T>
__device__ __forceinline__ void centred_terms(T va, T vth, double mu, double Kt, double Ka, double (&c)[8]) {
  const double d = (double)va - mu, d2 = d * d;
  c[0] += __builtin_fabs(d); c[1] += d2; c[2] += d2 * d2;
  const double dt = (double)vth - Kt;
  c[3] += dt; c[4] += dt * dt;
  const double da = __builtin_fabs((double)vth) - Ka;
  c[6] += da; c[7] += da * da;
}

// Pass C: one wrapped phase step w about the shift Kw.
__device__ __forceinline__ void step_terms(double w, double Kw, double (&c)[4]) {
  const double d = w - Kw, d2 = d * d;
  c[0] += d; c[1] += d2; c[2] += d2 * d; c[3] += d2 * d2;
}

// ---- complex helpers --------------------------------------------------------------------------------------------------
__device__ __forceinline__ float2 cmul(float2 a, float2 b) {                  // a b
  return make_float2(__builtin_fmaf(a.x, b.x, -(a.y * b.y)), __builtin_fmaf(a.x, b.y, a.y * b.x));
}
__device__ __forceinline__ float2 cmul_conj(float2 a, float2 b) {             // a conj(b)
  return make_float2(__builtin_fmaf(a.x, b.x, a.y * b.y), __builtin_fmaf(a.y, b.x, -(a.x * b.y)));
}

// W^e from two small tables: hi[e >> 6] = W^(64 (e >> 6)) times lo[e & 63] = W^(e & 63)
__device__ __forceinline__ float2 twiddle(const float2* hi, const float2* lo, int e) { return cmul(hi[e >> 6], lo[e & 63]); }

// Radix-2 butterflies on the pair (p, q) with the twiddle w, the results stored to (p_out, q_out), which may be where
// p and q were read.  Forward, decimation in frequency: (p + q, (p - q) w).  Inverse, decimation in time with the
// conjugate twiddle: (p + q conj(w), p - q conj(w)).
__device__ __forceinline__ void butterfly_dif(float2 p, float2 q, float2 w, float2& p_out, float2& q_out) {
  const float2 d = make_float2(p.x - q.x, p.y - q.y);
  p_out = make_float2(p.x + q.x, p.y + q.y);
  q_out = cmul(d, w);
}
__device__ __forceinline__ void butterfly_dit_conj(float2 p, float2 q, float2 w, float2& p_out, float2& q_out) {
  const float2 t = cmul_conj(q, w);
  p_out = make_float2(p.x + t.x, p.y + t.y);
  q_out = make_float2(p.x - t.x, p.y - t.y);
}

// ---- Bluestein's chirp-z form of the DFT ------------------------------------------------------------------------------
//   X_k = w_k sum_n (x_n w_n) conj(w_(k-n)),  w_n = exp(-i pi n^2 / N),
// a circular convolution of length M >= 2N - 1; |w_k| = 1 drops out of a peak.
__host__ __device__ inline int bluestein_length(int n) {          // smallest power of two >= 2n - 1
  int m = 1;
  while (m < 2 * n - 1) m <<= 1;
  return m;
}

// exp(sign * i pi n^2 / N): n^2 mod 2N in integers (n < 32768: n^2 < 2^30), then one sincospi
__device__ __forceinline__ float2 chirp(int n, int N, float sign) {
  const int r = (n * n) % (2 * N);
  float sn, cs;
  sincospif((float)r / (float)N, &sn, &cs);
  return make_float2(cs, sign * sn);
}

// entry n < M of the filter conj(w): it is even in n, so it is wrapped around M, zeros between
// (reference parameters: with n, N, M by value the inlined loop's induction variables come out in another order)
__device__ __forceinline__ float2 chirp_filter(const int& n, const int& N, const int& M) {
  const int d = n < N ? n : (M - n < N ? M - n : -1);
  return d >= 0 ? chirp(d, N, 1.0f) : make_float2(0.f, 0.f);
}

// entry n < N of the convolution's input, a_n = x_n w_n (the caller pads with zeros up to M)
__device__ __forceinline__ float2 chirp_input(float2 x, int n, int N) { return cmul(x, chirp(n, N, -1.0f)); }

}  // namespace amcx
