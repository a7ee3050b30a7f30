// What the global-attention forward (global_attn.hip) and backward (global_attn_bwd.hip) share: the workgroup shape and
// the 16-deep contraction chunk of their v_mfma_f32_16x16x4_f32 products.
#pragma once
#include "common.hpp"

namespace dlwp {
namespace gattn {

constexpr int kWaves = 4;        // waves per workgroup; each owns one 16-row tile
constexpr int kRegChunks = 8;    // head_dim <= 128: the wave's own 16 x d operands stay in registers (32 VGPRs each)

// 4 consecutive values [d0, d0 + 4) of one token row, zero beyond d or for a row that does not exist.
// VEC: d % 4 == 0 and the tensor is 16-byte aligned, so the four are all in or all out and one 16-byte load fetches them.
template <bool VEC>
__device__ __forceinline__ f32x4 load4(const float* __restrict__ row, int d0, int d, bool ok) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (VEC) {
    if (ok && d0 < d) v = *reinterpret_cast<const f32x4*>(row + d0);
  } else if (ok) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (d0 + t < d) v[t] = row[d0 + t];
  }
  return v;
}

__device__ __forceinline__ f32x4 mfma4(f32x4 a, f32x4 b, f32x4 acc) {
#pragma unroll
  for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], b[t], acc, 0, 0, 0);
  return acc;
}

}  // namespace gattn
}  // namespace dlwp
