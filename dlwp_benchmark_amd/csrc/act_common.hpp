// The pointwise activations of the U-Net family (codes 0 identity, 1 exact-erf GELU, 2 tanh, 3 ReLU, 4 SiLU), their
// derivatives, and the workgroup sum: shared by the convolutions (conv.hip, conv2.hip, conv_mfma.hip: staging and
// epilogues) and groupnorm_bwd.hip (GroupNorm forward and backward).
#pragma once

#include "common.hpp"

namespace dlwp {
namespace actc {

enum Act { ACT_NONE = 0, ACT_GELU = 1, ACT_TANH = 2, ACT_RELU = 3, ACT_SILU = 4 };

__device__ __forceinline__ float apply_act(float v, int act) {
  switch (act) {
    case ACT_GELU: return gelu_erf(v);
    case ACT_TANH: return tanhf(v);
    case ACT_RELU: return fmaxf(v, 0.f);
    case ACT_SILU: return v / (1.f + __expf(-v));
    default: return v;
  }
}

// d gelu / dv = Phi(v) + v phi(v).  Phi comes from the 0.5 erfc(|v| / sqrt2) that gelu_erf evaluates (same polynomial, same
// clamp): Phi(v) = 1 - e for v >= 0, e below.  phi(v) = exp(-v^2 / 2) / sqrt(2 pi).
__device__ __forceinline__ float gelu_erf_grad(float v) {
  const float u = fminf(fabsf(v), DLWP_GELU_UMAX);
  float p = DLWP_GELU_QTOP;
#define DLWP_STEP(c) p = fmaf(p, u, c);
  DLWP_GELU_COEFFS(DLWP_STEP)
#undef DLWP_STEP
  const float e = __builtin_amdgcn_exp2f(fmaf(p, u, -1.0f));  // 0.5 erfc(|v|/sqrt2)
  const float cdf = v >= 0.f ? 1.f - e : e;
  const float pdf = 0.3989422804014327f * __expf(-0.5f * v * v);
  return fmaf(v, pdf, cdf);
}

// act'(v) for the activation codes of apply_act
__device__ __forceinline__ float act_grad(float v, int act) {
  switch (act) {
    case 1: return gelu_erf_grad(v);
    case 2: {
      const float t = tanhf(v);
      return 1.f - t * t;
    }
    case 3: return v > 0.f ? 1.f : 0.f;
    case 4: {
      const float s = 1.f / (1.f + __expf(-v));
      return s * (1.f + v * (1.f - s));
    }
    default: return 1.f;
  }
}

// sum over the workgroup (a multiple of 64 threads, at most 512): xor tree inside each wave, then the waves in ascending
// order.  Every thread returns the total; s_red holds one float per wave.
__device__ __forceinline__ float block_sum(float v, float* s_red, int tid) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
  __syncthreads();
  if ((tid & 63) == 0) s_red[tid >> 6] = v;
  __syncthreads();
  float t = 0.f;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += s_red[w];
  return t;
}

}  // namespace actc
}  // namespace dlwp
