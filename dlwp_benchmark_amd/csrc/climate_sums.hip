// Climate sums of a rollout and its targets: the reductions over lead time behind the reference's physical-soundness scores
// (reference scripts/evaluate.py:832-872).  For a chunk out / target [B, K, C, H, W] of K consecutive rollout steps:
//   zonal[q][b][c][h]     += sum_{k < K} sum_{w} x_q[b, k, c, h, w]                         (mean over ("time", "lon"), :839-840)
//   window[q][b][c][h][w] += sum_{win_begin <= k < win_end} x_q[b, k, c, h, w]              (mean over the window's "time", :868-869)
// with q = 0: out, 1: target.  The means, the latitude bands and the roots are the caller's (metrics.SoundnessMetrics).
//
// Ownership.  A row is one (b, c, h): W consecutive floats per step, the steps C H W apart.  A group of G lanes of one wave
// owns a row for the whole call (G = the power of two that covers the row's W / V load units, at most 64: a wave owns 64 / G
// adjacent rows, a workgroup of four waves 256 / G; a workgroup walks the rows with the grid's stride).  The group walks the
// chunk's steps in step order.  In a step lane l adds the units l, l + G, l + 2 G, ... of the row, element by element, onto a
// double that starts at zero; the G partials are added by the xor tree G/2, ..., 2, 1; lane 0 adds the K row sums one after
// another onto the running value it read from `zonal` and writes it back once.  The window sums are element-wise adds in step
// order by the lane that loaded the element: the first NS units of a lane ride in registers between one read and one write
// of `window`, further ones are updated in memory step by step.  Every add is an fp64 add of a converted fp32 value; there
// is no fp32 partial, no atomic and no second writer of any output element.  V, G and the order of every add are functions
// of W alone -- not of K, the pointers or the device -- so the sums of a horizon are bit-identical however it is cut into
// chunks.  out and target are each read exactly once, with or without the window.
#include "common.hpp"

namespace dlwp {
namespace climate {

constexpr int NT = 256;   // four waves: at G = 64 a workgroup owns four rows at a time
constexpr int NS = 2;     // units per lane whose window sums stay in registers (W <= 512 at V = 4)

// one load unit: V consecutive floats.  V = 4 and `aligned`: one 16-byte load; V = 4 on an unaligned view: four 4-byte loads
// of the same elements (the same adds in the same order)
template <int V>
__device__ __forceinline__ void load_unit(const float* __restrict__ p, bool aligned, float (&v)[V]) {
  if constexpr (V == 4) {
    if (aligned) {
      const float4 f = *reinterpret_cast<const float4*>(p);
      v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    } else {
      v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
    }
  } else {
    v[0] = p[0];
  }
}

template <int V>
__global__ __launch_bounds__(NT) void climate_sums_kernel(const float* __restrict__ out, const float* __restrict__ tar,
                                                          double* __restrict__ zonal, double* __restrict__ window,
                                                          long long rows, int K, long long CH, int W, int G, int log2g,
                                                          int win_begin, int win_end, int aligned) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lg = lane & (G - 1), sub = lane >> log2g;
  const int rpw = 64 >> log2g;                                  // rows per wave
  const int n = W / V;                                          // units per row
  const long long step_stride = CH * W;
  const bool win = window != nullptr && win_end > win_begin;
  const bool al = aligned != 0;
  const long long rows_per_sweep = (long long)gridDim.x * (NT / 64) * rpw;
  for (long long row0 = ((long long)blockIdx.x * (NT / 64) + wave) * rpw; row0 < rows; row0 += rows_per_sweep) {
    const long long row = row0 + sub;
    const bool valid = row < rows;                              // lanes of a row past the end load nothing and write nothing
    const long long b = valid ? row / CH : 0;
    const long long off = valid ? (b * K * CH + (row - b * CH)) * W : 0;   // element (b, 0, c, h, 0)
    const float* __restrict__ po = out + off;
    const float* __restrict__ pt = tar + off;
    double* __restrict__ wo = win ? window + row * W : nullptr;
    double* __restrict__ wt = win ? window + (rows + row) * W : nullptr;
    double zo = 0.0, zt = 0.0;
    if (valid && lg == 0) {
      zo = zonal[row];
      zt = zonal[rows + row];
    }
    double ro[NS][V], rt[NS][V];                                // the window sums of this lane's first NS units
    if (win) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int i = lg + s * G;
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const bool on = valid && i < n;
          ro[s][e] = on ? wo[i * V + e] : 0.0;
          rt[s][e] = on ? wt[i * V + e] : 0.0;
        }
      }
    }
    for (int k = 0; k < K; ++k) {
      const float* __restrict__ xo = po + k * step_stride;
      const float* __restrict__ xt = pt + k * step_stride;
      const bool inw = win && k >= win_begin && k < win_end;
      double so = 0.0, st = 0.0;
      if (valid) {
        float vo[NS][V], vt[NS][V];
#pragma unroll
        for (int s = 0; s < NS; ++s) {                          // all loads of the step's first sweeps before their adds
          const int i = lg + s * G;
          if (i < n) {
            load_unit<V>(xo + i * V, al, vo[s]);
            load_unit<V>(xt + i * V, al, vt[s]);
          }
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const int i = lg + s * G;
          if (i < n) {
#pragma unroll
            for (int e = 0; e < V; ++e) {
              const double a = (double)vo[s][e], c = (double)vt[s][e];
              so += a;
              st += c;
              if (inw) {
                ro[s][e] += a;
                rt[s][e] += c;
              }
            }
          }
        }
        for (int i = lg + NS * G; i < n; i += G) {              // rows longer than NS sweeps (only G = 64 gets here)
          float uo[V], ut[V];
          load_unit<V>(xo + i * V, al, uo);
          load_unit<V>(xt + i * V, al, ut);
#pragma unroll
          for (int e = 0; e < V; ++e) {
            const double a = (double)uo[e], c = (double)ut[e];
            so += a;
            st += c;
            if (inw) {
              wo[i * V + e] += a;
              wt[i * V + e] += c;
            }
          }
        }
      }
      for (int o = G >> 1; o > 0; o >>= 1) {                    // fixed tree inside the group; every lane of the wave takes part
        so += __shfl_xor(so, o, 64);
        st += __shfl_xor(st, o, 64);
      }
      zo += so;
      zt += st;
    }
    if (valid && lg == 0) {
      zonal[row] = zo;
      zonal[rows + row] = zt;
    }
    if (win && valid) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int i = lg + s * G;
        if (i < n) {
#pragma unroll
          for (int e = 0; e < V; ++e) {
            wo[i * V + e] = ro[s][e];
            wt[i * V + e] = rt[s][e];
          }
        }
      }
    }
  }
}

}  // namespace climate
}  // namespace dlwp

using namespace dlwp;

extern "C" int32_t dlwp_climate_sums_acc_f32(const float* out_dev, const float* target_dev, double* zonal_dev,
                                             double* window_dev, int32_t batch, int32_t steps, int32_t channels, int32_t height,
                                             int32_t width, int32_t win_begin, int32_t win_end, void* stream) {
  DLWP_REQUIRE(out_dev && target_dev && zonal_dev, DLWP_ERR_INVALID_ARGUMENT, "climate sums: null out, target or zonal");
  DLWP_REQUIRE(batch > 0 && steps > 0 && channels > 0 && height > 0 && width > 0, DLWP_ERR_INVALID_ARGUMENT,
               "climate sums: bad shape [%d, %d, %d, %d, %d]", batch, steps, channels, height, width);
  DLWP_REQUIRE(0 <= win_begin && win_begin <= win_end && win_end <= steps, DLWP_ERR_INVALID_ARGUMENT,
               "climate sums: window [%d, %d) is not within the chunk's %d steps", win_begin, win_end, steps);
  DLWP_REQUIRE((reinterpret_cast<uintptr_t>(out_dev) & 3) == 0 && (reinterpret_cast<uintptr_t>(target_dev) & 3) == 0 &&
                   (reinterpret_cast<uintptr_t>(zonal_dev) & 7) == 0 && (reinterpret_cast<uintptr_t>(window_dev) & 7) == 0,
               DLWP_ERR_INVALID_ARGUMENT, "climate sums: out / target must be 4-byte and the sums 8-byte aligned");
  const long long ch = (long long)channels * height, rows = (long long)batch * ch;
  const int v = width % 4 == 0 ? 4 : 1;                 // the load unit, a function of W alone (see the ownership note)
  const int units = width / v;
  int log2g = 0;
  while ((1 << log2g) < units && log2g < 6) ++log2g;
  const int g = 1 << log2g;
  const long long rows_per_block = (climate::NT / 64) * (64 / g);
  long long blocks = (rows + rows_per_block - 1) / rows_per_block;
  if (blocks > 2048) blocks = 2048;                     // 8 workgroups a CU; more rows are walked with the grid's stride
  const int aligned = v == 4 && (reinterpret_cast<uintptr_t>(out_dev) & 15) == 0 && (reinterpret_cast<uintptr_t>(target_dev) & 15) == 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (v == 4)
    hipLaunchKernelGGL(climate::climate_sums_kernel<4>, dim3((unsigned)blocks), dim3(climate::NT), 0, s, out_dev, target_dev,
                       zonal_dev, window_dev, rows, steps, ch, width, g, log2g, win_begin, win_end, aligned);
  else
    hipLaunchKernelGGL(climate::climate_sums_kernel<1>, dim3((unsigned)blocks), dim3(climate::NT), 0, s, out_dev, target_dev,
                       zonal_dev, window_dev, rows, steps, ch, width, g, log2g, win_begin, win_end, aligned);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}
