// The pointwise part of a Linear's training step (y = act(x W^T + b) + resid: the nn.Linear layers of
// swin_transformer.py:21-39, :107-120, panguweather.py:176-211 and fourcastnet.py:40-53 under the `loss.backward()` of
// scripts/train.py:271), around the GEMMs of linear.hip:
//
//   dlwp_act_f32           h = act(z): the activation as a launch of its own, for a forward that must keep z.  The same
//                          gelu_erf arithmetic as the GEMM epilogue of dlwp_linear_f32, so h is what inference stores.
//   dlwp_bias_act_bwd_f32  gz = gy act'(z) and db_n = sum_rows gz in one pass over gy (and z).
//
// The column sum follows layernorm_bwd.hip: a thread owns one 16-byte column vector and adds its rows in ascending order;
// the row groups of a workgroup are added through LDS in group order; the workgroups' partials [P][N] are summed in index
// order by wgrad::wgrad_reduce_kernel -- above FOLD partials in two launches, [P / FOLD][FOLD N] over its first index and
// then [FOLD][N], because that kernel is one serial chain per output element.  One writer per element, no atomics: a rerun
// is bitwise identical.
#include "act_common.hpp"
#include "wgrad_reduce.hpp"

namespace dlwp {
namespace bact {

using actc::act_grad;
using actc::apply_act;

__global__ __launch_bounds__(256) void act_kernel(const float* __restrict__ z, float* __restrict__ h, long long nvec, int act) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += stride) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(z + 4 * i);
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = apply_act(v[k], act);
    *reinterpret_cast<f32x4*>(h + 4 * i) = o;
  }
}

// how the [rows][N] tensor is cut: cw lanes (a power of two, at most 64) side by side on consecutive column vectors,
// 256 / cw row groups per workgroup, cblocks workgroups across the columns, P down the rows (grid-stride)
struct Cut {
  int cw, cblocks, P;
};
constexpr int FOLD = 16;   // partials the second reduce launch sums; above FOLD, P is a multiple of it

static Cut cut_for(int64_t rows, int32_t n) {
  const int nvec = n / 4;
  Cut c;
  c.cw = 1;
  while (c.cw < 64 && c.cw < nvec) c.cw <<= 1;
  c.cblocks = (nvec + c.cw - 1) / c.cw;
  const int rpb = 256 / c.cw;
  long long p = (rows + rpb - 1) / rpb;
  const long long cap = 1024 / c.cblocks < 1 ? 1 : (1024 / c.cblocks > 256 ? 256 : 1024 / c.cblocks);
  c.P = (int)(p < cap ? p : cap);
  if (c.P > FOLD) c.P = c.P / FOLD * FOLD;
  return c;
}

// gz and gy may be the same tensor (no __restrict__): a thread reads an element before it writes it
template <bool ACT>
__global__ __launch_bounds__(256) void bias_act_bwd_kernel(const float* gy, const float* __restrict__ z, float* gz,
                                                           float* __restrict__ ws, long long rows, int N, int act, int cw,
                                                           int cblocks) {
  __shared__ f32x4 s_part[256];
  const int tid = threadIdx.x;
  const int nvec = N >> 2;
  const int rpb = 256 / cw;
  const int cb = (int)(blockIdx.x % cblocks), pb = (int)(blockIdx.x / cblocks), P = (int)(gridDim.x / cblocks);
  const int cv = cb * cw + (tid & (cw - 1));
  const int rg = tid / cw;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (cv < nvec) {
    for (long long row = (long long)pb * rpb + rg; row < rows; row += (long long)P * rpb) {
      const long long o = row * N + 4 * cv;
      f32x4 g = *reinterpret_cast<const f32x4*>(gy + o);
      if constexpr (ACT) {
        const f32x4 zv = *reinterpret_cast<const f32x4*>(z + o);
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] *= act_grad(zv[k], act);
        *reinterpret_cast<f32x4*>(gz + o) = g;
      }
      acc += g;
    }
  }
  if (ws == nullptr) return;
  s_part[tid] = acc;
  __syncthreads();
  if (tid < cw && cv < nvec) {
    f32x4 t = s_part[tid];
    for (int j = 1; j < rpb; ++j) t += s_part[j * cw + tid];
    *reinterpret_cast<f32x4*>(ws + (long long)pb * N + 4 * cv) = t;
  }
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace bact
}  // namespace dlwp

using namespace dlwp;

extern "C" int32_t dlwp_act_f32(const float* z, float* h, int64_t n, int32_t act, void* stream) {
  DLWP_REQUIRE(z && h, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(n > 0, DLWP_ERR_INVALID_ARGUMENT, "bad size");
  DLWP_REQUIRE(act >= 0 && act <= 4, DLWP_ERR_INVALID_ARGUMENT, "unknown activation %d", act);
  DLWP_REQUIRE(n % 4 == 0 && bact::aligned16(z) && bact::aligned16(h), DLWP_ERR_UNSUPPORTED,
               "act: the size must be a multiple of 4 and z, h 16-byte aligned");
  const long long nvec = n / 4;
  long long blocks = (nvec + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(bact::act_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), z, h, nvec,
                     act);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" size_t dlwp_bias_act_bwd_workspace_bytes(int64_t rows, int32_t n) {
  if (rows <= 0 || n <= 0 || n % 4 != 0) return 0;
  const int P = bact::cut_for(rows, n).P;      // the partials [P][n] and, above FOLD of them, the folded sums [FOLD][n]
  return (size_t)(P + (P > bact::FOLD ? bact::FOLD : 0)) * (size_t)n * sizeof(float);
}

extern "C" int32_t dlwp_bias_act_bwd_f32(const float* gy, const float* z, float* gz, float* db, void* workspace,
                                         size_t workspace_bytes, int64_t rows, int32_t n, int32_t act, void* stream) {
  DLWP_REQUIRE(gy, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(rows > 0 && n > 0, DLWP_ERR_INVALID_ARGUMENT, "bad shape");
  DLWP_REQUIRE(act >= 0 && act <= 4, DLWP_ERR_INVALID_ARGUMENT, "unknown activation %d", act);
  DLWP_REQUIRE(act == 0 || (z && gz), DLWP_ERR_INVALID_ARGUMENT, "an activation needs z and gz");
  DLWP_REQUIRE(!db || workspace, DLWP_ERR_INVALID_ARGUMENT, "null workspace");
  DLWP_REQUIRE(n % 4 == 0, DLWP_ERR_UNSUPPORTED, "width %d: must be a multiple of 4", n);
  DLWP_REQUIRE(bact::aligned16(gy) && (act == 0 || (bact::aligned16(z) && bact::aligned16(gz))) &&
                   (!db || bact::aligned16(workspace)),
               DLWP_ERR_UNSUPPORTED, "gy, z, gz and the workspace must be 16-byte aligned");
  DLWP_REQUIRE(!db || workspace_bytes >= dlwp_bias_act_bwd_workspace_bytes(rows, n), DLWP_ERR_WORKSPACE,
               "workspace of %zu bytes, %zu needed", workspace_bytes, dlwp_bias_act_bwd_workspace_bytes(rows, n));
  if (act == 0 && !db) return DLWP_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bact::Cut c = bact::cut_for(rows, n);
  float* ws = db ? static_cast<float*>(workspace) : nullptr;
  const dim3 grid((unsigned)(c.cblocks * c.P));
  if (act != 0)
    hipLaunchKernelGGL((bact::bias_act_bwd_kernel<true>), grid, dim3(256), 0, s, gy, z, gz, ws, (long long)rows, n, act, c.cw,
                       c.cblocks);
  else
    hipLaunchKernelGGL((bact::bias_act_bwd_kernel<false>), grid, dim3(256), 0, s, gy, z, gz, ws, (long long)rows, n, act, c.cw,
                       c.cblocks);
  if (db) {
    int P = c.P;
    const float* part = ws;
    if (P > bact::FOLD) {
      const long long wide = (long long)bact::FOLD * n;
      float* fold = ws + (long long)P * n;
      hipLaunchKernelGGL(wgrad::wgrad_reduce_kernel, dim3((unsigned)((wide + 255) / 256)), dim3(256), 0, s, part,
                         (const float*)nullptr, fold, (float*)nullptr, wide, 0, P / bact::FOLD);
      part = fold;
      P = bact::FOLD;
    }
    hipLaunchKernelGGL(wgrad::wgrad_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, (const float*)nullptr,
                       db, (float*)nullptr, (long long)n, 0, P);
  }
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}
