// Register / LDS building blocks of the hand-written complex FFTs, shared by the AFNO 2-D transforms (afno_fft.hip)
// and the zonal energy spectrum (zonal_spectrum.hip).
//
// Every complex FFT of length N = A * B runs as TWO register passes with one LDS exchange: radix-A butterflies over
// n2 of x[n1 + B n2] (in registers), twiddle w_N^(n1 k2), stored in place; then radix-B over n1 of the B contiguous
// values at B k2 -> X[k2 + A k1].  Radices are 4, 8 or 16 with compile-time twiddles.
#pragma once

#include <hip/hip_runtime.h>

namespace dlwp {
namespace afft {

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return float2{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return float2{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return float2{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ float2 cconj(float2 a) { return float2{a.x, -a.y}; }
// multiply by SIGN * i  (SIGN = -1: the forward kernel's w_4 = -i)
template <int SIGN>
__device__ __forceinline__ float2 mul_si(float2 a) { return SIGN < 0 ? float2{a.y, -a.x} : float2{-a.y, a.x}; }

// w_16^k = exp(SIGN 2 pi i k / 16), k = 0..7 (compile-time constants)
template <int SIGN>
__device__ __forceinline__ float2 w16(int k) {
  constexpr float c1 = 0.92387953251128674f, s1 = 0.38268343236508977f, r2 = 0.70710678118654752f;
  const float cs[8] = {1.f, c1, r2, s1, 0.f, -s1, -r2, -c1};
  const float sn[8] = {0.f, s1, r2, c1, 1.f, c1, r2, s1};
  return float2{cs[k], SIGN * sn[k]};
}

template <int SIGN>
__device__ __forceinline__ void dft4(float2& a0, float2& a1, float2& a2, float2& a3) {
  const float2 t0 = cadd(a0, a2), t1 = csub(a0, a2), t2 = cadd(a1, a3), t3 = mul_si<SIGN>(csub(a1, a3));
  a0 = cadd(t0, t2);
  a2 = csub(t0, t2);
  a1 = cadd(t1, t3);
  a3 = csub(t1, t3);
}
template <int R, int SIGN>
struct Dft;
template <int SIGN>
struct Dft<4, SIGN> {
  static __device__ __forceinline__ void run(float2 (&v)[4]) { dft4<SIGN>(v[0], v[1], v[2], v[3]); }
};
template <int SIGN>
struct Dft<8, SIGN> {
  static __device__ __forceinline__ void run(float2 (&v)[8]) {
    float2 e[4] = {v[0], v[2], v[4], v[6]}, o[4] = {v[1], v[3], v[5], v[7]};
    Dft<4, SIGN>::run(e);
    Dft<4, SIGN>::run(o);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float2 t = cmul(w16<SIGN>(2 * k), o[k]);
      v[k] = cadd(e[k], t);
      v[k + 4] = csub(e[k], t);
    }
  }
};
template <int SIGN>
struct Dft<16, SIGN> {
  static __device__ __forceinline__ void run(float2 (&v)[16]) {
    float2 e[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { e[k] = v[2 * k]; o[k] = v[2 * k + 1]; }
    Dft<8, SIGN>::run(e);
    Dft<8, SIGN>::run(o);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float2 t = cmul(w16<SIGN>(k), o[k]);
      v[k] = cadd(e[k], t);
      v[k + 8] = csub(e[k], t);
    }
  }
};

// `count` FFTs of length N = A * B living in LDS as buf[f * stride + n]; items are dealt f-fastest (bank-conflict free
// for stride = odd number of float2 ... see the callers); tw[j] = exp(-2 pi i j / N), conjugated for SIGN = +1.
// PASS 1 (in place).
template <int A, int B, int SIGN, int NT>
__device__ __forceinline__ void fft_pass1(float2* buf, int stride, int count, const float2* tw, int tid) {
  for (int it = tid; it < count * B; it += NT) {
    const int f = it % count, n1 = it / count;
    float2* p = buf + f * stride + n1;
    float2 v[A];
#pragma unroll
    for (int n2 = 0; n2 < A; ++n2) v[n2] = p[B * n2];
    Dft<A, SIGN>::run(v);
#pragma unroll
    for (int k2 = 0; k2 < A; ++k2) {
      float2 w = tw[n1 * k2];
      if (SIGN > 0) w.y = -w.y;
      p[B * k2] = k2 == 0 ? v[0] : cmul(v[k2], w);
    }
  }
}
// PASS 2: reads the B contiguous values at B k2, leaves X[k2 + A k1] (k1 = 0..B-1) in `v`.
template <int A, int B, int SIGN>
__device__ __forceinline__ void fft_pass2_regs(const float2* row, int k2, float2 (&v)[B]) {
#pragma unroll
  for (int n1 = 0; n1 < B; ++n1) v[n1] = row[B * k2 + n1];
  Dft<B, SIGN>::run(v);
}
// PASS 2 in place: X[k2 + A k1] is stored where its inputs were, at B k2 + k1 -- "scrambled" order; a reader finds
// X[k] at pos<A, B>(k).  No second buffer, no barrier between the reads and the writes of different items.
template <int A, int B>
__device__ __forceinline__ int pos(int k) { return B * (k % A) + k / A; }
template <int A, int B, int SIGN, int NT>
__device__ __forceinline__ void fft_pass2_inplace(float2* buf, int stride, int count, int tid) {
  for (int it = tid; it < count * A; it += NT) {
    float2* row = buf + (it % count) * stride;
    const int k2 = it / count;
    float2 v[B];
    fft_pass2_regs<A, B, SIGN>(row, k2, v);
#pragma unroll
    for (int k1 = 0; k1 < B; ++k1) row[B * k2 + k1] = v[k1];
  }
}

}  // namespace afft
}  // namespace dlwp
