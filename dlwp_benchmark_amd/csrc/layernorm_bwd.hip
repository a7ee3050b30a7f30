// LayerNorm backward over the last (channel) dimension of token-major tensors: the `loss.backward()` of scripts/train.py:271
// through the nn.LayerNorm layers of the token backbones (fourcastnet.py:180-193; swin_transformer.py:213,262;
// panguweather.py:281,321).  For y = LayerNorm_C(x) gamma + beta, x and gy [rows][C]:
//
//   xh = (x - mean) rstd      g = gy gamma      a = mean_C(g)      b = mean_C(g xh)
//   dx = rstd (g - a - xh b)  dgamma_c = sum_rows gy xh            dbeta_c = sum_rows gy
//
// A row is at most 8 KB and lives in registers, in the forward's row-to-lane mapping (layernorm_row.hpp: 16 / 32 / 64 lanes
// per row, NV 16-byte vectors per lane, grid-stride over the rows).  mean and rstd are recomputed from x with the forward's
// own two sweeps, so a training step saves neither; one pass reads x and gy once and writes dx once (the 2 reads + 1 write
// floor).
//
// Launch 1 (layernorm_bwd_kernel): dx, and per lane the slice of sum gy xh and sum gy over all rows its lane group takes, in
//   ascending row order.  The lane groups of a workgroup then add their slices through LDS in group order (= ascending first
//   row) and the first group writes the workgroup's partial: workspace [2][P][C] (dgamma partials, then dbeta partials), P
//   workgroups.  P depends on (rows, C) alone; it is at most MAX_PARTIALS and P C at most MAX_PARTIAL_FLOATS (a workspace of
//   4.5 MB at the most).
// Launch 2 (wgrad::wgrad_reduce_kernel): dgamma / dbeta = the P partials summed in index order.  wgrad_reduce_kernel is one
//   serial chain per output element, so above FOLD partials P is a multiple of FOLD and the sum takes the kernel twice:
//   [P / FOLD][FOLD C] over its first index into [FOLD][C] behind the partials, then that over FOLD -- two chains of at
//   most 64 instead of one of 2048, the first FOLD C elements wide.
// One writer per element, no atomics, fixed orders: a rerun is bitwise identical.
#include "layernorm_row.hpp"
#include "wgrad_reduce.hpp"

namespace dlwp {
namespace lnb {

constexpr int MAX_PARTIALS = 2048;     // workgroups of launch 1 when it accumulates dgamma / dbeta (eight per compute unit)
constexpr long long MAX_PARTIAL_FLOATS = 1 << 19;   // P C at the most
constexpr int FOLD = 32;               // partials the second reduce launch sums; above FOLD, P is a multiple of it
constexpr int MAX_BLOCKS_DX = 256 * 16;  // without partials: the forward's grid

using norm::load_row_stats;

template <int LPR, int NV>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ gy, float* __restrict__ dx,
                                                            float* __restrict__ ws, long long rows, int C, float eps) {
  __shared__ f32x4 s_part[2 * NV * 256];           // [dgamma | dbeta][NV][thread]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int sub = lane % LPR;                        // position inside the row's lane group
  constexpr int RPW = 64 / LPR;                      // rows per wave
  const long long wave_id = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long nwave = ((long long)gridDim.x * blockDim.x) >> 6;
  const int nvec = C >> 2;
  const bool want_dx = dx != nullptr, want_part = ws != nullptr;
  f32x4 gm[NV], nopre[NV], dg[NV], db[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int iv = sub + v * LPR;
    gm[v] = iv < nvec ? *reinterpret_cast<const f32x4*>(gamma + 4 * iv) : f32x4{0.f, 0.f, 0.f, 0.f};
    nopre[v] = dg[v] = db[v] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float inv_c = 1.0f / (float)C;
  for (long long r0 = wave_id * RPW; r0 < rows; r0 += nwave * RPW) {
    const long long row = r0 + lane / LPR;
    const bool live = row < rows;
    f32x4 xv[NV], gv[NV];
    float mean, rstd;
#pragma unroll
    for (int v = 0; v < NV; ++v) {                   // issued before the statistics: both loads of the row are in flight
      const int iv = sub + v * LPR;
      gv[v] = (live && iv < nvec) ? *reinterpret_cast<const f32x4*>(gy + row * C + 4 * iv) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    load_row_stats<LPR, NV>(x, row, live, sub, nvec, C, nopre, inv_c, eps, xv, mean, rstd);
    // xh in place of x.  A dead row or vector has gy = 0 and gamma = 0: it adds nothing below.
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int k = 0; k < 4; ++k) xv[v][k] = (xv[v][k] - mean) * rstd;
    if (want_part) {
#pragma unroll
      for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          dg[v][k] = fmaf(gv[v][k], xv[v][k], dg[v][k]);
          db[v][k] += gv[v][k];
        }
    }
    if (want_dx) {
      float sa = 0.f, sb = 0.f;
#pragma unroll
      for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          gv[v][k] *= gm[v][k];                      // g
          sa += gv[v][k];
          sb = fmaf(gv[v][k], xv[v][k], sb);
        }
#pragma unroll
      for (int m = LPR / 2; m >= 1; m >>= 1) {
        sa += __shfl_xor(sa, m);
        sb += __shfl_xor(sb, m);
      }
      const float a = sa * inv_c, b = sb * inv_c;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const int iv = sub + v * LPR;
        if (live && iv < nvec) {
          f32x4 o;
#pragma unroll
          for (int k = 0; k < 4; ++k) o[k] = rstd * ((gv[v][k] - a) - xv[v][k] * b);
          *reinterpret_cast<f32x4*>(dx + row * C + 4 * iv) = o;
        }
      }
    }
  }
  if (!want_part) return;
  // the workgroup's 256 / LPR lane groups, group tid / LPR first: it holds the workgroup's lowest rows of every sweep
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    s_part[v * 256 + tid] = dg[v];
    s_part[(NV + v) * 256 + tid] = db[v];
  }
  __syncthreads();
  if (tid < LPR) {
    const long long P = gridDim.x;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int iv = tid + v * LPR;
      if (iv < nvec) {
        f32x4 sg = s_part[v * 256 + tid], sb = s_part[(NV + v) * 256 + tid];
        for (int g = 1; g < 256 / LPR; ++g) {
          sg += s_part[v * 256 + g * LPR + tid];
          sb += s_part[(NV + v) * 256 + g * LPR + tid];
        }
        *reinterpret_cast<f32x4*>(ws + (long long)blockIdx.x * C + 4 * iv) = sg;
        *reinterpret_cast<f32x4*>(ws + (P + blockIdx.x) * C + 4 * iv) = sb;
      }
    }
  }
}

static bool in_envelope(int64_t rows, int32_t channels) {
  return rows > 0 && channels > 0 && channels % 4 == 0 && channels <= 2048;
}

// workgroups that cover the rows once, before any cap
static long long blocks_for(int64_t rows, int32_t channels) {
  const int nvec = channels / 4;
  const int lpr = nvec <= 16 ? 16 : nvec <= 32 ? 32 : 64;
  const long long waves = (rows + 64 / lpr - 1) / (64 / lpr);
  return (waves + 3) / 4;
}

static int partials(int64_t rows, int32_t channels) {
  long long p = blocks_for(rows, channels);
  if (p > MAX_PARTIALS) p = MAX_PARTIALS;
  if (p * channels > MAX_PARTIAL_FLOATS) p = MAX_PARTIAL_FLOATS / channels;   // >= 256
  return (int)(p > FOLD ? p / FOLD * FOLD : p);
}

// floats of the workspace: the partials [2][P][C] and, above FOLD of them, the folded sums [2][FOLD][C]
static size_t workspace_floats(int P, int32_t channels) {
  return (size_t)2 * (size_t)(P + (P > FOLD ? FOLD : 0)) * (size_t)channels;
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace lnb
}  // namespace dlwp

using namespace dlwp;

extern "C" int32_t dlwp_layernorm_bwd_partials(int64_t rows, int32_t channels) {
  return lnb::in_envelope(rows, channels) ? lnb::partials(rows, channels) : 0;
}

extern "C" size_t dlwp_layernorm_bwd_workspace_bytes(int64_t rows, int32_t channels) {
  if (!lnb::in_envelope(rows, channels)) return 0;
  return lnb::workspace_floats(lnb::partials(rows, channels), channels) * sizeof(float);
}

extern "C" int32_t dlwp_layernorm_bwd_f32(const float* x, const float* gamma, const float* gy, float* dx, float* dgamma,
                                          float* dbeta, void* workspace, size_t workspace_bytes, int64_t rows,
                                          int32_t channels, float eps, void* stream) {
  DLWP_REQUIRE(x && gamma && gy, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(rows > 0 && channels > 0, DLWP_ERR_INVALID_ARGUMENT, "bad shape");
  const bool want_part = dgamma != nullptr || dbeta != nullptr;
  DLWP_REQUIRE(!want_part || workspace, DLWP_ERR_INVALID_ARGUMENT, "null workspace");
  DLWP_REQUIRE(channels % 4 == 0 && channels <= 2048, DLWP_ERR_UNSUPPORTED,
               "channels %d: must be a multiple of 4 and <= 2048", channels);
  DLWP_REQUIRE(lnb::aligned16(x) && lnb::aligned16(gy) && lnb::aligned16(dx) && lnb::aligned16(gamma) &&
                   (!want_part || lnb::aligned16(workspace)),
               DLWP_ERR_UNSUPPORTED, "x, gamma, gy, dx and the workspace must be 16-byte aligned");
  DLWP_REQUIRE(!want_part || workspace_bytes >= dlwp_layernorm_bwd_workspace_bytes(rows, channels), DLWP_ERR_WORKSPACE,
               "workspace of %zu bytes, %zu needed", workspace_bytes, dlwp_layernorm_bwd_workspace_bytes(rows, channels));
  if (!dx && !want_part) return DLWP_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* ws = want_part ? static_cast<float*>(workspace) : nullptr;
  // with partials the grid IS the partial count the workspace was sized for (grid-stride over the rows either way)
  long long blocks = want_part ? lnb::partials(rows, channels) : lnb::blocks_for(rows, channels);
  if (blocks > lnb::MAX_BLOCKS_DX) blocks = lnb::MAX_BLOCKS_DX;
  const int32_t rc = norm::dispatch_row(channels / 4, [&](auto lpr, auto nv) -> int32_t {
    hipLaunchKernelGGL((lnb::layernorm_bwd_kernel<decltype(lpr)::value, decltype(nv)::value>), dim3((unsigned)blocks), dim3(256), 0,
                       s, x, gamma, gy, dx, ws, (long long)rows, channels, eps);
    return DLWP_OK;
  });
  if (rc != DLWP_OK) return rc;
  if (want_part) {
    int P = (int)blocks;
    const float* part_g = ws;
    const float* part_b = ws + (long long)P * channels;
    if (P > lnb::FOLD) {
      const int wide = lnb::FOLD * channels;          // <= 65536
      float* fold_g = ws + 2ll * P * channels;
      float* fold_b = fold_g + wide;
      hipLaunchKernelGGL(wgrad::wgrad_reduce_kernel, dim3((unsigned)((2 * wide + 255) / 256)), dim3(256), 0, s, part_g, part_b,
                         fold_g, fold_b, (long long)wide, wide, P / lnb::FOLD);
      part_g = fold_g;
      part_b = fold_b;
      P = lnb::FOLD;
    }
    const long long n_w = dgamma ? channels : 0;
    const int n_b = dbeta ? channels : 0;
    hipLaunchKernelGGL(wgrad::wgrad_reduce_kernel, dim3((unsigned)((n_w + n_b + 255) / 256)), dim3(256), 0, s, part_g, part_b,
                       dgamma, dbeta, n_w, n_b, P);
  }
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}
