// The activation of GraphCastNet's MLPs (codes 0 identity, 1 ReLU, 2 SiLU) and its derivative: shared by graphcast.hip
// (forward and data gradients) and graphcast_bwd.hip (the weight gradient re-applies it to a saved pre-activation).
#pragma once
#include "common.hpp"

namespace dlwp {
namespace gc {

__device__ __forceinline__ float activate(float v, int act) {
  if (act == 1) return fmaxf(v, 0.f);
  if (act == 2) return v / (1.0f + expf(-v));
  return v;
}

// d act / d z at the pre-activation z, as torch's relu / silu backward: ReLU z > 0; SiLU s (1 + z (1 - s)), s = sigmoid z
__device__ __forceinline__ float activate_grad(float z, int act) {
  if (act == 1) return z > 0.f ? 1.f : 0.f;
  if (act == 2) {
    const float s = 1.0f / (1.0f + expf(-z));
    return s * (1.0f + z * (1.0f - s));
  }
  return 1.f;
}

}  // namespace gc
}  // namespace dlwp
