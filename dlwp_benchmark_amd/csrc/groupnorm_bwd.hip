// GroupNorm + activation of the U-Net / ModernUNet family in both directions (reference models/unet/unet.py:739 final_norm
// (+ GELU :761), :887-888 ResidualBlock norms; backward: scripts/train.py:271 `loss.backward()` through them).
//
//   v = xh gamma_c + beta_c,  xh = (x - mean) rstd,  y = act(v),  E = (C / groups) HW
//
// Forward: one workgroup per (sample, group), two-sweep statistics, affine + activation fused into the third sweep.  With a
// non-null `stats` it also writes (mean, rstd) per (sample, group): all that a training step keeps besides x.
//
// Backward, from x, stats, gamma, beta and gy alone (xh, v and gv = gy act'(v) are recomputed):
//   s1[n,c] = sum_hw gv         s2[n,c] = sum_hw gv xh
//   dbeta_c = sum_n s1[n,c]     dgamma_c = sum_n s2[n,c]
//   a[n,g] = sum_{c in g} gamma_c s1[n,c] / E      b[n,g] = sum_{c in g} gamma_c s2[n,c] / E
//   dx = rstd (gv gamma_c - a - xh b)
// The work is split over the N C rows [n][c][HW] of the tensor, not over (sample, group): ResidualBlock uses one group, and
// a grid of N workgroups would leave most of the chip idle.  Three launches:
//   rowsum   s1, s2 of every row into the workspace [2][N C]
//   dparam   dgamma / dbeta: per channel the serial sum over n in ascending order (the loads go through LDS in chunks)
//   dx       every workgroup first re-derives a, b of the (sample, group) pairs its rows belong to from the row sums
// A row is handled by G lanes, G the power of two that covers the row in one sweep of 16-byte (vector form) or 4-byte
// (scalar form) loads, at most 64; 256 / G consecutive rows share a workgroup, so a wave reads consecutive memory whatever
// the row length (HW = 4 at the bottom of the U-Net: one lane per row, one 16-byte load each).  Rows longer than 64 loads
// take a whole workgroup (BLOCK form).  The launcher picks the vector form only when HW % 4 == 0 and every tensor pointer is
// 16-byte aligned.  Every sum has a fixed order and one writer (no atomics): a rerun is bitwise identical.
// Traffic: 4 reads + 1 write of the tensor (x and gy in both passes) against a floor of 2 reads + 1 write.
#include "act_common.hpp"

namespace dlwp {
namespace gn {

using actc::act_grad;
using actc::apply_act;
using actc::block_sum;

// one workgroup per (sample, group): elements [n][g * cpg .. (g + 1) * cpg)[HW] are contiguous in NCHW
__global__ __launch_bounds__(256) void groupnorm_act_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float* __restrict__ y,
                                                            float* __restrict__ stats, int C, int HW, int groups, float eps,
                                                            int act) {
  __shared__ float s_red[8];
  const int tid = threadIdx.x;
  const int n = blockIdx.x / groups, g = blockIdx.x % groups;
  const int cpg = C / groups;
  const long long base = ((long long)n * C + (long long)g * cpg) * HW;
  const int E = cpg * HW;
  float s = 0.f;
  for (int i = tid; i < E; i += 256) s += x[base + i];
  const float mean = block_sum(s, s_red, tid) / (float)E;
  float q = 0.f;
  for (int i = tid; i < E; i += 256) {
    const float dlt = x[base + i] - mean;
    q += dlt * dlt;
  }
  const float var = block_sum(q, s_red, tid) / (float)E;      // biased, like torch.nn.GroupNorm
  const float rstd = rsqrtf(var + eps);
  if (stats != nullptr && tid == 0) {
    stats[2 * (long long)blockIdx.x] = mean;
    stats[2 * (long long)blockIdx.x + 1] = rstd;
  }
  for (int i = tid; i < E; i += 256) {
    const int c = g * cpg + i / HW;
    float v = (x[base + i] - mean) * rstd;
    v = v * (gamma ? gamma[c] : 1.f) + (beta ? beta[c] : 0.f);
    y[base + i] = apply_act(v, act);
  }
}

struct BwdP {
  const float* x;      // [N][C][HW]
  const float* stats;  // [N * groups][2]: mean, rstd
  const float* gamma;  // [C] or null
  const float* beta;   // [C] or null
  const float* gy;     // [N][C][HW]
  float* dx;           // [N][C][HW]
  float* ws;           // [2][rows]: s1, s2
  int C, HW, cpg, rows, act;
  int G;               // lanes per row (power of two, <= 64) of the sub-wave forms
  int P;               // lanes per (sample, group) when the dx pass re-derives a, b (power of two, <= 64)
};

template <int V>
__device__ __forceinline__ void load_v(const float* p, float (&o)[V]) {
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
  } else {
    o[0] = *p;
  }
}

template <int V>
__device__ __forceinline__ void store_v(float* p, const float (&o)[V]) {
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
    *p = o[0];
  }
}

// s1, s2 of every row.  V floats per load; BLOCK: one row per workgroup, otherwise p.G lanes per row.
template <int V, bool BLOCK>
__global__ __launch_bounds__(256) void gn_bwd_rowsum_kernel(const BwdP p) {
  __shared__ float s_red[8];
  const int tid = threadIdx.x;
  const int G = BLOCK ? 256 : p.G;
  const int row = (int)blockIdx.x * (256 / G) + tid / G;
  const int lane = tid & (G - 1);
  const bool valid = row < p.rows;
  float s1 = 0.f, s2 = 0.f;
  if (valid) {
    const int c = row % p.C, ng = row / p.cpg;
    const float mean = p.stats[2 * (long long)ng], rstd = p.stats[2 * (long long)ng + 1];
    const float gm = p.gamma ? p.gamma[c] : 1.f, bt = p.beta ? p.beta[c] : 0.f;
    const float* xr = p.x + (long long)row * p.HW;
    const float* gr = p.gy + (long long)row * p.HW;
    for (int i = lane * V; i < p.HW; i += G * V) {
      float xv[V], gv[V];
      load_v<V>(xr + i, xv);
      load_v<V>(gr + i, gv);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float xh = (xv[k] - mean) * rstd;
        const float g = gv[k] * act_grad(xh * gm + bt, p.act);
        s1 += g;
        s2 += g * xh;
      }
    }
  }
  if constexpr (BLOCK) {
    s1 = block_sum(s1, s_red, tid);
    s2 = block_sum(s2, s_red, tid);
  } else {
    for (int m = 1; m < G; m <<= 1) {
      s1 += __shfl_xor(s1, m);
      s2 += __shfl_xor(s2, m);
    }
  }
  if (valid && lane == 0) {
    p.ws[row] = s1;
    p.ws[(long long)p.rows + row] = s2;
  }
}

// dbeta_c = sum_n s1[n][c], dgamma_c = sum_n s2[n][c], n ascending.  A workgroup takes 8 channels; 128 samples at a time go
// through LDS so that the loads run in parallel while the sum itself stays one serial chain per (channel, sum).
__global__ __launch_bounds__(256) void gn_bwd_dparam_kernel(const float* __restrict__ ws, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, int N, int C) {
  constexpr int TC = 8, CN = 128;
  __shared__ float s[2][CN][TC];
  const int tid = threadIdx.x;
  const int c0 = (int)blockIdx.x * TC;
  const int w_me = tid / TC, c_me = tid % TC;      // the summing threads: tid < 2 * TC
  float acc = 0.f;
  for (int n0 = 0; n0 < N; n0 += CN) {
    for (int i = tid; i < 2 * CN * TC; i += 256) {
      const int w = i / (CN * TC), nl = (i / TC) % CN, cl = i % TC;
      const int n = n0 + nl, c = c0 + cl;
      s[w][nl][cl] = (n < N && c < C) ? ws[(long long)w * N * C + (long long)n * C + c] : 0.f;
    }
    __syncthreads();
    if (tid < 2 * TC) {
      const int lim = N - n0 < CN ? N - n0 : CN;
      for (int nl = 0; nl < lim; ++nl) acc += s[w_me][nl][c_me];
    }
    __syncthreads();
  }
  if (tid < 2 * TC && c0 + c_me < C) {
    float* out = w_me ? dgamma : dbeta;
    if (out) out[c0 + c_me] = acc;
  }
}

// dx = rstd (gv gamma_c - a - xh b).  The workgroup's rows lie in the (sample, group) pairs ng_lo .. ng_lo + count - 1
// (ng = row / cpg); a, b of each are summed by p.P lanes from the row sums, then every row proceeds as in the first pass.
template <int V, bool BLOCK>
__global__ __launch_bounds__(256) void gn_bwd_dx_kernel(const BwdP p) {
  __shared__ float s_a[256], s_b[256];          // count <= rows per workgroup <= 256
  const int tid = threadIdx.x;
  const int G = BLOCK ? 256 : p.G;
  const int rpb = 256 / G;
  const int row0 = (int)blockIdx.x * rpb;
  const int row_end = row0 + rpb < p.rows ? row0 + rpb : p.rows;
  const int ng_lo = row0 / p.cpg;
  const int count = (row_end - 1) / p.cpg - ng_lo + 1;
  const float E = (float)((long long)p.cpg * p.HW);
  for (int j0 = 0; j0 < count; j0 += 256 / p.P) {
    const int j = j0 + tid / p.P, pl = tid & (p.P - 1);
    float a = 0.f, b = 0.f;
    if (j < count) {
      const int r0 = (ng_lo + j) * p.cpg;       // first row of the pair; its channel is r0 % C
      const int ch0 = r0 % p.C;
      for (int k = pl; k < p.cpg; k += p.P) {
        const float gm = p.gamma ? p.gamma[ch0 + k] : 1.f;
        a += gm * p.ws[r0 + k];
        b += gm * p.ws[(long long)p.rows + r0 + k];
      }
    }
    for (int m = 1; m < p.P; m <<= 1) {
      a += __shfl_xor(a, m);
      b += __shfl_xor(b, m);
    }
    if (j < count && pl == 0) {
      s_a[j] = a / E;
      s_b[j] = b / E;
    }
  }
  __syncthreads();
  const int row = row0 + tid / G;
  const int lane = tid & (G - 1);
  if (row >= p.rows) return;
  const int c = row % p.C, ng = row / p.cpg;
  const float mean = p.stats[2 * (long long)ng], rstd = p.stats[2 * (long long)ng + 1];
  const float gm = p.gamma ? p.gamma[c] : 1.f, bt = p.beta ? p.beta[c] : 0.f;
  const float a = s_a[ng - ng_lo], b = s_b[ng - ng_lo];
  const float* xr = p.x + (long long)row * p.HW;
  const float* gr = p.gy + (long long)row * p.HW;
  float* dr = p.dx + (long long)row * p.HW;
  for (int i = lane * V; i < p.HW; i += G * V) {
    float xv[V], gv[V], dv[V];
    load_v<V>(xr + i, xv);
    load_v<V>(gr + i, gv);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float xh = (xv[k] - mean) * rstd;
      const float g = gv[k] * act_grad(xh * gm + bt, p.act);
      dv[k] = rstd * (g * gm - a - xh * b);
    }
    store_v<V>(dr + i, dv);
  }
}

static int pow2_at_least(long long v, int cap) {
  int g = 1;
  while (g < cap && g < v) g <<= 1;
  return g;
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int V, bool BLOCK>
static void launch_bwd(const BwdP& p, bool want_dx, hipStream_t s) {
  const int rpb = BLOCK ? 1 : 256 / p.G;
  const unsigned grid = (unsigned)((p.rows + rpb - 1) / rpb);
  hipLaunchKernelGGL((gn_bwd_rowsum_kernel<V, BLOCK>), dim3(grid), dim3(256), 0, s, p);
  if (want_dx) hipLaunchKernelGGL((gn_bwd_dx_kernel<V, BLOCK>), dim3(grid), dim3(256), 0, s, p);
}

}  // namespace gn
}  // namespace dlwp

using namespace dlwp;

static int32_t groupnorm_forward(const float* x, const float* gamma, const float* beta, float* y, float* stats, int32_t batch,
                                 int32_t channels, int32_t hw, int32_t groups, float eps, int32_t act, void* stream) {
  DLWP_REQUIRE(x && y, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(batch > 0 && channels > 0 && hw > 0 && groups > 0 && channels % groups == 0, DLWP_ERR_INVALID_ARGUMENT,
               "bad shape: %d channels in %d groups", channels, groups);
  DLWP_REQUIRE(act >= 0 && act <= 4, DLWP_ERR_INVALID_ARGUMENT, "unknown activation %d", act);
  DLWP_REQUIRE((long long)(channels / groups) * hw < (1ll << 31), DLWP_ERR_UNSUPPORTED, "group too large");
  DLWP_REQUIRE((long long)batch * groups < (1ll << 31), DLWP_ERR_UNSUPPORTED, "too many (sample, group) pairs");
  hipLaunchKernelGGL(gn::groupnorm_act_kernel, dim3((unsigned)(batch * groups)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), x, gamma, beta, y, stats, channels, hw, groups, eps, act);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" int32_t dlwp_groupnorm_act_f32(const float* x, const float* gamma, const float* beta, float* y, int32_t batch,
                                          int32_t channels, int32_t hw, int32_t groups, float eps, int32_t act, void* stream) {
  return groupnorm_forward(x, gamma, beta, y, nullptr, batch, channels, hw, groups, eps, act, stream);
}

extern "C" int32_t dlwp_groupnorm_act_fwd_stats_f32(const float* x, const float* gamma, const float* beta, float* y,
                                                    float* stats, int32_t batch, int32_t channels, int32_t hw, int32_t groups,
                                                    float eps, int32_t act, void* stream) {
  DLWP_REQUIRE(stats, DLWP_ERR_INVALID_ARGUMENT, "null stats");
  return groupnorm_forward(x, gamma, beta, y, stats, batch, channels, hw, groups, eps, act, stream);
}

extern "C" size_t dlwp_groupnorm_act_bwd_workspace_bytes(int32_t batch, int32_t channels) {
  if (batch <= 0 || channels <= 0) return 0;
  return (size_t)2 * (size_t)batch * (size_t)channels * sizeof(float);
}

extern "C" int32_t dlwp_groupnorm_act_bwd_f32(const float* x, const float* stats, const float* gamma, const float* beta,
                                              const float* gy, float* dx, float* dgamma, float* dbeta, void* workspace,
                                              int32_t batch, int32_t channels, int32_t hw, int32_t groups, int32_t act,
                                              void* stream) {
  DLWP_REQUIRE(x && stats && gy && workspace, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(batch > 0 && channels > 0 && hw > 0 && groups > 0 && channels % groups == 0, DLWP_ERR_INVALID_ARGUMENT,
               "bad shape: %d channels in %d groups", channels, groups);
  DLWP_REQUIRE(act >= 0 && act <= 4, DLWP_ERR_INVALID_ARGUMENT, "unknown activation %d", act);
  DLWP_REQUIRE((long long)(channels / groups) * hw < (1ll << 31), DLWP_ERR_UNSUPPORTED, "group too large");
  DLWP_REQUIRE((long long)batch * channels <= (1ll << 30) && hw <= (1 << 30), DLWP_ERR_UNSUPPORTED, "tensor too large");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  gn::BwdP p;
  p.x = x; p.stats = stats; p.gamma = gamma; p.beta = beta; p.gy = gy; p.dx = dx;
  p.ws = static_cast<float*>(workspace);
  p.C = channels; p.HW = hw; p.cpg = channels / groups; p.rows = batch * channels; p.act = act;
  const bool vec = hw % 4 == 0 && gn::aligned16(x) && gn::aligned16(gy) && gn::aligned16(dx);
  const int loads = vec ? hw / 4 : hw;           // per row
  p.G = gn::pow2_at_least(loads, 64);
  p.P = gn::pow2_at_least(p.cpg, 64);
  const bool block = loads > 64;
  if (vec && block) gn::launch_bwd<4, true>(p, dx != nullptr, s);
  else if (vec) gn::launch_bwd<4, false>(p, dx != nullptr, s);
  else if (block) gn::launch_bwd<1, true>(p, dx != nullptr, s);
  else gn::launch_bwd<1, false>(p, dx != nullptr, s);
  if (dgamma || dbeta)
    hipLaunchKernelGGL(gn::gn_bwd_dparam_kernel, dim3((unsigned)((channels + 7) / 8)), dim3(256), 0, s, p.ws, dgamma, dbeta,
                       batch, channels);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}
