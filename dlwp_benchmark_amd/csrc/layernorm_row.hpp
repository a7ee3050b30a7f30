// One token-major LayerNorm row in registers: the row load and the two statistics sweeps that the forward (norm.hip,
// layernorm_kernel) and the backward (layernorm_bwd.hip) share, so that the backward recomputes mean and rstd with the
// forward's own arithmetic and saves neither.  LPR lanes (16 / 32 / 64) hold a row, NV 16-byte vectors each; lane `sub`
// of the group owns the vectors sub + v * LPR.  Sums run as xor-shuffles inside the lane group, two-pass (mean, then the
// sum of squared deviations) like torch's CPU kernel.
#pragma once

#include <type_traits>

#include "common.hpp"

namespace dlwp {
namespace norm {

// (LPR, NV) of a row of nvec 16-byte vectors: the dispatch table of the forward and the backward.  F is a generic
// callable taking two std::integral_constant arguments.
template <typename F>
static inline int32_t dispatch_row(int nvec, F&& f) {
#define DLWP_ROW(L, N) return f(std::integral_constant<int, L>{}, std::integral_constant<int, N>{})
  if (nvec <= 16) DLWP_ROW(16, 1);
  if (nvec <= 32) DLWP_ROW(32, 1);
  switch ((nvec + 63) / 64) {
    case 1: DLWP_ROW(64, 1);
    case 2: DLWP_ROW(64, 2);
    case 3: DLWP_ROW(64, 3);
    case 4: DLWP_ROW(64, 4);
    case 5: case 6: DLWP_ROW(64, 6);
    default: DLWP_ROW(64, 8);
  }
#undef DLWP_ROW
}

// xv: the lane's slice of row `row` (+ pb, the optional per-channel vector added BEFORE the statistics), zeros where the
// row or the vector does not exist; mean and rstd of the row in every lane of the group.
template <int LPR, int NV>
__device__ __forceinline__ void load_row_stats(const float* __restrict__ x, long long row, bool live, int sub, int nvec, int C,
                                               const f32x4 (&pb)[NV], float inv_c, float eps, f32x4 (&xv)[NV], float& mean,
                                               float& rstd) {
  float s = 0.f;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int iv = sub + v * LPR;
    xv[v] = (live && iv < nvec) ? *reinterpret_cast<const f32x4*>(x + row * C + 4 * iv) + pb[v] : f32x4{0.f, 0.f, 0.f, 0.f};
    s += (xv[v][0] + xv[v][1]) + (xv[v][2] + xv[v][3]);
  }
#pragma unroll
  for (int m = LPR / 2; m >= 1; m >>= 1) s += __shfl_xor(s, m);
  mean = s * inv_c;
  float q = 0.f;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int iv = sub + v * LPR;
    if (iv < nvec) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float dlt = xv[v][k] - mean;
        q = fmaf(dlt, dlt, q);
      }
    }
  }
#pragma unroll
  for (int m = LPR / 2; m >= 1; m >>= 1) q += __shfl_xor(q, m);
  rstd = rsqrtf(q * inv_c + eps);
}

}  // namespace norm
}  // namespace dlwp
