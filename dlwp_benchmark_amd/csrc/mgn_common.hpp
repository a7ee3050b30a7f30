// What the MeshGraphNet forward (mgn.hip) and backward (mgn_bwd.hip) must agree on bit for bit, defined once: the workgroup
// shape, the MLP descriptor, the scalar Linear product and the LayerNorm of a row (the backward recomputes the forward in
// LDS with exactly these), and the host code that fills the descriptor from the C ABI's and raises the LDS limit.
#pragma once
#include "common.hpp"

// namespace mgn: the forward's; mgn_bwd.hip reaches these definitions through it
namespace dlwp {
namespace mgn {

constexpr int kThreads = 256;
constexpr int kWave = 64;

// The pointer and width part of an MLP descriptor as the kernels take it.  mgn::Mlp and mgn_bwd::Mlp derive from it and
// declare `float eps` (and the backward its gradient offsets) themselves: 128 bytes without tail padding, so the fields
// a derived struct adds start where they would in one flat struct.
struct MlpBase {
  int n;                 // Linear count, 2..5
  int dims[6];
  const float* wt[5];    // [dims[l]][dims[l + 1]]
  const float* bias[5];
  const float* g;
  const float* b;
};

__host__ __device__ inline int round4(int x) { return (x + 3) & ~3; }

// out[r][j] = act(bias[j] + sum_k in[r][k] wt[k][j]) for r < R (R % 4 == 0), j < n_out; in / out are LDS tiles.  fp32 FMA
// chain in k order
__device__ __forceinline__ void dense(const float* in, int ldi, int n_in, float* out, int ldo, int n_out,
                                      const float* __restrict__ wt, const float* __restrict__ bias, int R, bool relu) {
  const int pairs = (R >> 2) * n_out;
  for (int p = threadIdx.x; p < pairs; p += kThreads) {
    const int j = p % n_out, r0 = (p / n_out) * 4;
    const float* i0 = in + r0 * ldi;
    const float* i1 = i0 + ldi;
    const float* i2 = i1 + ldi;
    const float* i3 = i2 + ldi;
    const float bj = bias[j];
    float a0 = bj, a1 = bj, a2 = bj, a3 = bj;
    const float* w = wt + j;
    int k = 0;
    for (; k + 4 <= n_in; k += 4) {
      const float w0 = w[(size_t)k * n_out], w1 = w[(size_t)(k + 1) * n_out];
      const float w2 = w[(size_t)(k + 2) * n_out], w3 = w[(size_t)(k + 3) * n_out];
      const float4 x0 = *reinterpret_cast<const float4*>(i0 + k);
      const float4 x1 = *reinterpret_cast<const float4*>(i1 + k);
      const float4 x2 = *reinterpret_cast<const float4*>(i2 + k);
      const float4 x3 = *reinterpret_cast<const float4*>(i3 + k);
      a0 = fmaf(x0.x, w0, a0); a1 = fmaf(x1.x, w0, a1); a2 = fmaf(x2.x, w0, a2); a3 = fmaf(x3.x, w0, a3);
      a0 = fmaf(x0.y, w1, a0); a1 = fmaf(x1.y, w1, a1); a2 = fmaf(x2.y, w1, a2); a3 = fmaf(x3.y, w1, a3);
      a0 = fmaf(x0.z, w2, a0); a1 = fmaf(x1.z, w2, a1); a2 = fmaf(x2.z, w2, a2); a3 = fmaf(x3.z, w2, a3);
      a0 = fmaf(x0.w, w3, a0); a1 = fmaf(x1.w, w3, a1); a2 = fmaf(x2.w, w3, a2); a3 = fmaf(x3.w, w3, a3);
    }
    for (; k < n_in; ++k) {
      const float wk = w[(size_t)k * n_out];
      a0 = fmaf(i0[k], wk, a0); a1 = fmaf(i1[k], wk, a1); a2 = fmaf(i2[k], wk, a2); a3 = fmaf(i3[k], wk, a3);
    }
    if (relu) {
      a0 = fmaxf(a0, 0.f); a1 = fmaxf(a1, 0.f); a2 = fmaxf(a2, 0.f); a3 = fmaxf(a3, 0.f);
    }
    float* o = out + r0 * ldo + j;
    o[0] = a0; o[ldo] = a1; o[2 * ldo] = a2; o[3 * ldo] = a3;
  }
}

// LayerNorm of one row of width d in place (two-pass mean / variance, biased, like torch), one wave
__device__ __forceinline__ void layernorm_row(float* row, int d, const float* __restrict__ g, const float* __restrict__ b,
                                              float eps, int lane) {
  float s = 0.f;
  for (int k = lane; k < d; k += kWave) s += row[k];
  const float mean = wave_sum(s) / (float)d;
  float q = 0.f;
  for (int k = lane; k < d; k += kWave) {
    const float c = row[k] - mean;
    q = fmaf(c, c, q);
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)d + eps);
  for (int k = lane; k < d; k += kWave) row[k] = fmaf((row[k] - mean) * rstd, g[k], b[k]);
}

// host: fill `m` from the C ABI's descriptor and check it against the caller's envelope (input width <= max_in, every
// other width <= max_width).  `who` prefixes and `envelope` ends the caller's error texts.  The caller takes ln_eps and
// checks the gamma / beta pair itself.
static int32_t fill_mlp(const dlwp_mgn_mlp_desc* d, MlpBase& m, int max_in, int max_width, const char* who,
                        const char* envelope) {
  DLWP_REQUIRE(d, DLWP_ERR_INVALID_ARGUMENT, "%s: null MLP descriptor", who);
  DLWP_REQUIRE(d->n_linear >= 2 && d->n_linear <= 5, DLWP_ERR_UNSUPPORTED, "%s: %d Linears (2..5 supported)", who,
               d->n_linear);
  m.n = d->n_linear;
  for (int i = 0; i <= m.n; ++i) {
    m.dims[i] = d->dims[i];
    DLWP_REQUIRE(d->dims[i] > 0, DLWP_ERR_INVALID_ARGUMENT, "%s: width %d of layer %d", who, d->dims[i], i);
    DLWP_REQUIRE(d->dims[i] <= (i == 0 ? max_in : max_width), DLWP_ERR_UNSUPPORTED,
                 "%s: width %d of layer %d is outside the %s", who, d->dims[i], i, envelope);
  }
  for (int i = m.n + 1; i < 6; ++i) m.dims[i] = 0;
  for (int i = 0; i < 5; ++i) {
    m.wt[i] = i < m.n ? d->wt[i] : nullptr;
    m.bias[i] = i < m.n ? d->bias[i] : nullptr;
    if (i < m.n) DLWP_REQUIRE(d->wt[i] && d->bias[i], DLWP_ERR_INVALID_ARGUMENT, "%s: null weight of Linear %d", who, i);
  }
  m.g = d->ln_gamma;
  m.b = d->ln_beta;
  return DLWP_OK;
}

// host: a kernel that asks for more than 64 KiB of dynamic LDS has to be told so once
template <class K>
static int32_t set_lds(K kern, size_t lds) {
  if (lds > 64 * 1024)
    DLWP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return DLWP_OK;
}

}  // namespace mgn
}  // namespace dlwp
