// The second launch of the convolution weight gradients (conv_wgrad.hip): the K-slices' partial dW / db, which the first launch
// left in the workspace, summed in slice order (layernorm_bwd.hip and bias_act.hip sum their partials with it too).  One writer
// per element and a fixed order: with a slice count that depends on the shape alone the result is bit-identical from run to run.
#pragma once

#include "common.hpp"

namespace dlwp {
namespace wgrad {

// dw[i] = sum over the slices, in index order, of part_w[s][i]; db likewise behind it (n_b = 0: no bias gradient)
static __global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part_w,
                                                                  const float* __restrict__ part_b, float* __restrict__ dw,
                                                                  float* __restrict__ db, long long n_w, int n_b, int slices) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n_w) {
    float v = 0.f;
    for (int s = 0; s < slices; ++s) v += part_w[(long long)s * n_w + i];
    dw[i] = v;
  } else if (i < n_w + n_b) {
    const int c = (int)(i - n_w);
    float v = 0.f;
    for (int s = 0; s < slices; ++s) v += part_b[(long long)s * n_b + c];
    db[c] = v;
  }
}

}  // namespace wgrad
}  // namespace dlwp
