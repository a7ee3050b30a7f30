// The device-resident WeatherBench dataset (reference data/datasets/datasets.py:291-453, climatology.py:41,
// scripts/build_baselines.py:64): the fields live on the card as ONE float32 store [T, V, plane] -- time first, the variables
// (levels flattened by the host) next, plane = H W on a lat-lon grid and 12 n n on HEALPix -- and everything the reference
// does per sample on the host with xarray is a gather or a reduction over that store:
//   gather      one launch assembles prescribed / prognostic / target of a batch from a device table of frame indices
//               (__getitem__ + default_collate, :330-416): normalisation, NaN fill, the input noise and the input / target
//               split included; every stored value is read once per window
//   stats       count, sum and squared deviations per variable over a list of frames (compute_statistics, :419-453)
//   group mean  the mean per (group, variable, grid point) over a list of frames with a group id each (the monthly
//               climatology, climatology.py:41)
//   coarsen     k x k block means, NaN skipped (downscale_factor, :303-305); once, when the store is built
//
// Work split.  256 threads per workgroup; a thread owns a UNIT of 4 consecutive plane elements of one row (a row: one plane
// of an output, or one (frame, variable) plane of the store), a workgroup a TILE of 256 units of one row, and the grid --
// capped at MAX_BLOCKS -- walks the tiles with its own stride.  A tile never straddles rows, so everything but the unit
// index is uniform in a workgroup (scalar arithmetic, one 64-bit division per tile, none per element).  A unit is one
// 16-byte load / store where plane % 4 == 0 and the base address is 16-byte aligned (checked per pointer: an unaligned
// output view takes 4-byte stores while the store is still read 16 bytes at a time), and up to four 4-byte accesses of the
// same elements otherwise (and for the ragged last unit of a plane).  Offsets into the store are 64-bit throughout.
//
// Determinism.  No atomics.  The reductions accumulate in fp64 from the first add: a thread adds its elements in ascending
// (tile, element) order, a wave adds its lanes by the xor tree 32, ..., 1, thread 0 adds the four waves in order, and a
// single thread adds the workgroups' partials in workgroup order -- an order fixed by the shape, not by the device.
#include "philox_normal.hpp"

namespace dlwp {
namespace dataset {

constexpr int NT = 256;
constexpr int MAX_BLOCKS = 2048;      // eight workgroups per compute unit
constexpr int STAT_BLOCKS = 128;      // workgroups per variable of a statistics pass (a partial each)

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__device__ __forceinline__ f32x4 load4(const float* __restrict__ p, int live, bool vec) {
  if (vec) return *reinterpret_cast<const f32x4*>(p);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < live) v[k] = p[k];
  return v;
}

__device__ __forceinline__ void store4(float* __restrict__ p, int live, bool vec, f32x4 v) {
  if (vec) {
    *reinterpret_cast<f32x4*>(p) = v;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < live) p[k] = v[k];
  }
}

static unsigned grid_for(long long tiles, int cap) { return (unsigned)(tiles < cap ? (tiles > 0 ? tiles : 1) : cap); }

// ---- gather ---------------------------------------------------------------------------------------------------------------
// a channel table row: {source variable, mean (fp32 bits), std (fp32 bits), replace-NaN-by-0 flag}
struct GatherArgs {
  const float* store;
  const int* frames;        // [B, S + 1]
  const int* items;         // [B]: the noise member of each sample (read only with noise != 0)
  const int4* prog_tab;     // [C]
  const int4* pres_tab;     // [P]
  float* prescribed;        // [B, S, P, plane] or null
  float* prognostic;        // [B, S, C, plane] or null
  float* target;            // [B, S - context, C, plane] or null
  long long T, plane, nq, tpr, rows_prog, tiles;
  int V, B, S, context, C, P, normalize;
  float noise;
  uint64_t seed, q0;
};

// the normals of the elements e .. e + 3 of stream `member` (element e has the stream index 4 q0 + e)
__device__ __forceinline__ f32x4 noise4(uint64_t seed, uint32_t member, uint64_t q0, long long e, int live, bool one_block) {
  if (one_block) return philox::normal4(seed, member, q0 + (uint64_t)(e >> 2));
  f32x4 r = {0.f, 0.f, 0.f, 0.f}, z = r;
  long long have = -1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < live) {
      const long long blk = (e + k) >> 2;
      if (blk != have) {
        z = philox::normal4(seed, member, q0 + (uint64_t)blk);
        have = blk;
      }
      const int lane = (int)((e + k) & 3);
      r[k] = lane == 0 ? z[0] : lane == 1 ? z[1] : lane == 2 ? z[2] : z[3];
    }
  }
  return r;
}

__global__ __launch_bounds__(NT) void gather_kernel(const GatherArgs a) {
  const bool plane4 = (a.plane & 3) == 0;
  const bool vin = plane4 && aligned16(a.store);
  const bool vpres = plane4 && aligned16(a.prescribed), vprog = plane4 && aligned16(a.prognostic),
             vtar = plane4 && aligned16(a.target);
  const int S1 = a.S + 1;
  for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const long long row = tile / a.tpr;
    const long long q = (tile - row * a.tpr) * NT + threadIdx.x;
    if (q >= a.nq) continue;
    const long long p0 = 4 * q;
    const int live = a.plane - p0 < 4 ? (int)(a.plane - p0) : 4;
    const bool full = live == 4;
    const bool is_prog = row < a.rows_prog;
    int b, j, c;
    if (is_prog) {
      const long long r = row;
      b = (int)(r / ((long long)S1 * a.C));
      const int rem = (int)(r - (long long)b * S1 * a.C);
      j = rem / a.C;
      c = rem - j * a.C;
    } else {
      const long long r = row - a.rows_prog;
      b = (int)(r / ((long long)a.S * a.P));
      const int rem = (int)(r - (long long)b * a.S * a.P);
      j = rem / a.P;
      c = rem - j * a.P;
    }
    const bool to_prog = is_prog && j < a.S && a.prognostic != nullptr;
    const bool to_tar = is_prog && j > a.context && a.target != nullptr;
    const bool to_pres = !is_prog && a.prescribed != nullptr;
    if (!(to_prog || to_tar || to_pres)) continue;
    const int4 tab = is_prog ? a.prog_tab[c] : a.pres_tab[c];
    const int t = a.frames[(long long)b * S1 + j];
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (t >= 0 && t < a.T && tab.x >= 0 && tab.x < a.V) {      // a missing frame is zeros (datasets.py:405-409)
      v = load4(a.store + ((long long)t * a.V + tab.x) * a.plane + p0, live, vin && full);
      if (a.normalize) {
        const float mean = __int_as_float(tab.y), sd = __int_as_float(tab.z);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = __fdiv_rn(__fsub_rn(v[k], mean), sd);
      }
      if (tab.w) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = v[k] != v[k] ? 0.f : v[k];
      }
    }
    if (to_pres) store4(a.prescribed + (((long long)b * a.S + j) * a.P + c) * a.plane + p0, live, vpres && full, v);
    if (to_tar)
      store4(a.target + (((long long)b * (a.S - a.context) + (j - 1 - a.context)) * a.C + c) * a.plane + p0, live, vtar && full,
             v);
    if (to_prog) {
      if (a.noise != 0.f) {      // the noised value goes to prognostic alone (datasets.py:413-414)
        const long long e = ((long long)j * a.C + c) * a.plane + p0;
        const f32x4 eps = noise4(a.seed, (uint32_t)a.items[b], a.q0, e, live, plane4);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = __fadd_rn(v[k], __fmul_rn(a.noise, eps[k]));
      }
      store4(a.prognostic + (((long long)b * a.S + j) * a.C + c) * a.plane + p0, live, vprog && full, v);
    }
  }
}

// ---- statistics -------------------------------------------------------------------------------------------------------------
// PASS 1: partial[v][blk] = {count of non-NaN values, their sum};  PASS 2: {unused, sum of (x - mean[v])^2}
template <int PASS>
__global__ __launch_bounds__(NT) void stats_pass_kernel(const float* __restrict__ store, const int* __restrict__ frames,
                                                        long long n_frames, long long T, int V, long long plane, long long nq,
                                                        long long tpr, const double* __restrict__ mean,
                                                        double* __restrict__ partial) {
  const int v = blockIdx.y;
  const bool vin = (plane & 3) == 0 && aligned16(store);
  const double mu = PASS == 2 ? mean[v] : 0.0;
  double s = 0.0, cnt = 0.0;      // a count stays exact in a double up to 2^53
  const long long tiles = n_frames * tpr;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long f = tile / tpr;
    const long long q = (tile - f * tpr) * NT + threadIdx.x;
    const int t = frames[f];
    if (t < 0 || t >= T || q >= nq) continue;
    const long long p0 = 4 * q;
    const int live = plane - p0 < 4 ? (int)(plane - p0) : 4;
    const f32x4 x = load4(store + ((long long)t * V + v) * plane + p0, live, vin && live == 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < live && x[k] == x[k]) {
        if (PASS == 1) {
          s += (double)x[k];
          cnt += 1.0;
        } else {
          const double d = (double)x[k] - mu;
          s += d * d;
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    cnt += __shfl_xor(cnt, o, 64);
  }
  __shared__ double sh[2][NT / 64];
  if ((threadIdx.x & 63) == 0) {
    sh[0][threadIdx.x >> 6] = cnt;
    sh[1][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double c = 0.0, t = 0.0;
    for (int w = 0; w < NT / 64; ++w) {
      c += sh[0][w];
      t += sh[1][w];
    }
    partial[((long long)v * gridDim.x + blockIdx.x) * 2 + 0] = c;
    partial[((long long)v * gridDim.x + blockIdx.x) * 2 + 1] = t;
  }
}

// one thread per variable adds the workgroups' partials in workgroup order
template <int PASS>
__global__ void stats_finish_kernel(const double* __restrict__ partial, int V, int blocks, double* __restrict__ mean,
                                    double* __restrict__ out) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  double c = 0.0, s = 0.0;
  for (int b = 0; b < blocks; ++b) {
    c += partial[((long long)v * blocks + b) * 2 + 0];
    s += partial[((long long)v * blocks + b) * 2 + 1];
  }
  if (PASS == 1) {
    out[3 * v + 0] = c;
    out[3 * v + 1] = s;
    mean[v] = s / c;      // 0 / 0 = NaN for a variable without a value: pass two then adds nothing
  } else {
    out[3 * v + 2] = s;
  }
}

// ---- group mean -------------------------------------------------------------------------------------------------------------
// a thread owns the unit (g, v, 4 plane elements) and walks the listed frames in list order, loading only its group's
__global__ __launch_bounds__(NT) void group_mean_kernel(const float* __restrict__ store, const int* __restrict__ frames,
                                                        const int* __restrict__ groups, long long n_frames, long long T, int V,
                                                        long long plane, long long nq, long long tpr, long long tiles,
                                                        float* __restrict__ out) {
  const bool plane4 = (plane & 3) == 0;
  const bool vin = plane4 && aligned16(store), vout = plane4 && aligned16(out);
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long row = tile / tpr;      // g * V + v
    const long long q = (tile - row * tpr) * NT + threadIdx.x;
    if (q >= nq) continue;
    const int g = (int)(row / V), v = (int)(row - (long long)g * V);
    const long long p0 = 4 * q;
    const int live = plane - p0 < 4 ? (int)(plane - p0) : 4;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (long long f = 0; f < n_frames; ++f) {
      if (groups[f] != g) continue;
      const int t = frames[f];
      if (t < 0 || t >= T) continue;
      const f32x4 x = load4(store + ((long long)t * V + v) * plane + p0, live, vin && live == 4);
      if (x[0] == x[0]) { s0 += (double)x[0]; ++c0; }
      if (live > 1 && x[1] == x[1]) { s1 += (double)x[1]; ++c1; }
      if (live > 2 && x[2] == x[2]) { s2 += (double)x[2]; ++c2; }
      if (live > 3 && x[3] == x[3]) { s3 += (double)x[3]; ++c3; }
    }
    const float nan = __int_as_float(0x7fc00000);
    f32x4 m;
    m[0] = c0 ? (float)(s0 / (double)c0) : nan;
    m[1] = c1 ? (float)(s1 / (double)c1) : nan;
    m[2] = c2 ? (float)(s2 / (double)c2) : nan;
    m[3] = c3 ? (float)(s3 / (double)c3) : nan;
    store4(out + row * plane + p0, live, vout && live == 4, m);
  }
}

// ---- coarsen ----------------------------------------------------------------------------------------------------------------
// K > 0: a thread owns 4 consecutive outputs of a row: K 16-byte loads per input row, one 16-byte store (Wo % 4 == 0, both
// bases aligned).  K = 0: a thread owns one output, 4-byte accesses, any k.  The adds of an output are the same in both: rows
// outer, columns inner.
template <int K>
__global__ __launch_bounds__(NT) void coarsen_kernel(const float* __restrict__ in, float* __restrict__ out, long long n_units,
                                                     int Ho, int Wo, int k) {
  const float nan = __int_as_float(0x7fc00000);
  const int kk = K > 0 ? K : k;
  const long long W = (long long)Wo * kk, H = (long long)Ho * kk;
  constexpr int OUTS = K > 0 ? 4 : 1;
  const int upr = Wo / OUTS;      // units per output row
  for (long long u = (long long)blockIdx.x * NT + threadIdx.x; u < n_units; u += (long long)gridDim.x * NT) {
    const long long orow = u / upr;      // plane * Ho + oh
    const int ow = (int)(u - orow * upr) * OUTS;
    const long long pl = orow / Ho;
    const int oh = (int)(orow - pl * Ho);
    const float* __restrict__ src = in + (pl * H + (long long)oh * kk) * W + (long long)ow * kk;
    double s[OUTS];
    int c[OUTS];
#pragma unroll
    for (int o = 0; o < OUTS; ++o) {
      s[o] = 0.0;
      c[o] = 0;
    }
    for (int r = 0; r < kk; ++r) {
      const float* __restrict__ rp = src + r * W;
      if constexpr (K > 0) {
        f32x4 x[K];
#pragma unroll
        for (int i = 0; i < K; ++i) x[i] = *reinterpret_cast<const f32x4*>(rp + 4 * i);
#pragma unroll
        for (int e = 0; e < 4 * K; ++e) {
          const float xv = x[e / 4][e % 4];
          if (xv == xv) {
            s[e / K] += (double)xv;
            ++c[e / K];
          }
        }
      } else {
        for (int i = 0; i < kk; ++i) {
          const float xv = rp[i];
          if (xv == xv) {
            s[0] += (double)xv;
            ++c[0];
          }
        }
      }
    }
    if constexpr (K > 0) {
      f32x4 m;
#pragma unroll
      for (int o = 0; o < 4; ++o) m[o] = c[o] ? (float)(s[o] / (double)c[o]) : nan;
      *reinterpret_cast<f32x4*>(out + orow * Wo + ow) = m;
    } else {
      out[orow * Wo + ow] = c[0] ? (float)(s[0] / (double)c[0]) : nan;
    }
  }
}

static bool host_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace dataset
}  // namespace dlwp

using namespace dlwp;

extern "C" int32_t dlwp_dataset_grid_blocks(void) { return dataset::MAX_BLOCKS; }

extern "C" int32_t dlwp_dataset_gather_f32(const float* store_dev, int64_t n_times, int32_t n_vars, int64_t plane,
                                           const int32_t* frames_dev, const int32_t* items_dev, int32_t batch, int32_t seq,
                                           int32_t context, const int32_t* prog_table_dev, int32_t n_prog,
                                           const int32_t* pres_table_dev, int32_t n_pres, float* prescribed_dev,
                                           float* prognostic_dev, float* target_dev, int32_t normalize, float noise, int64_t seed,
                                           int64_t offset, void* stream) {
  DLWP_REQUIRE(store_dev && frames_dev, DLWP_ERR_INVALID_ARGUMENT, "dataset gather: null store or frame table");
  DLWP_REQUIRE(n_times > 0 && n_vars > 0 && plane > 0 && batch > 0 && seq > 0, DLWP_ERR_INVALID_ARGUMENT,
               "dataset gather: bad shape (T %lld, V %d, plane %lld, B %d, S %d)", (long long)n_times, n_vars, (long long)plane,
               batch, seq);
  DLWP_REQUIRE(n_times <= INT32_MAX, DLWP_ERR_INVALID_ARGUMENT, "dataset gather: the frame table holds int32 time indices");
  DLWP_REQUIRE(context >= 0 && context <= seq && n_prog >= 0 && n_pres >= 0, DLWP_ERR_INVALID_ARGUMENT,
               "dataset gather: bad context %d / channel counts %d, %d", context, n_prog, n_pres);
  DLWP_REQUIRE(n_prog == 0 || prog_table_dev, DLWP_ERR_INVALID_ARGUMENT, "dataset gather: null prognostic channel table");
  DLWP_REQUIRE(n_pres == 0 || !prescribed_dev || pres_table_dev, DLWP_ERR_INVALID_ARGUMENT,
               "dataset gather: null prescribed channel table");
  DLWP_REQUIRE(noise == 0.f || !prognostic_dev || items_dev, DLWP_ERR_INVALID_ARGUMENT,
               "dataset gather: noise needs the item of every sample");
  DLWP_REQUIRE(offset >= 0 && (offset & 3) == 0, DLWP_ERR_INVALID_ARGUMENT, "the offset must be a non-negative multiple of 4");
  DLWP_REQUIRE(dataset::host_aligned(store_dev, 4) && dataset::host_aligned(prescribed_dev, 4) &&
                   dataset::host_aligned(prognostic_dev, 4) && dataset::host_aligned(target_dev, 4) &&
                   dataset::host_aligned(prog_table_dev, 16) && dataset::host_aligned(pres_table_dev, 16),
               DLWP_ERR_INVALID_ARGUMENT, "dataset gather: tensors must be 4-byte and channel tables 16-byte aligned");
  dataset::GatherArgs a;
  a.store = store_dev;
  a.frames = frames_dev;
  a.items = items_dev;
  a.prog_tab = reinterpret_cast<const int4*>(prog_table_dev);
  a.pres_tab = reinterpret_cast<const int4*>(pres_table_dev);
  a.prescribed = n_pres > 0 ? prescribed_dev : nullptr;
  a.prognostic = n_prog > 0 ? prognostic_dev : nullptr;
  a.target = n_prog > 0 && context < seq ? target_dev : nullptr;
  a.T = n_times;
  a.plane = plane;
  a.nq = (plane + 3) / 4;
  a.tpr = (a.nq + dataset::NT - 1) / dataset::NT;
  a.V = n_vars;
  a.B = batch;
  a.S = seq;
  a.context = context;
  a.C = n_prog;
  a.P = a.prescribed ? n_pres : 0;
  a.normalize = normalize;
  a.noise = noise;
  a.seed = (uint64_t)seed;
  a.q0 = (uint64_t)offset >> 2;
  a.rows_prog = (a.prognostic || a.target) ? (long long)batch * (seq + 1) * n_prog : 0;
  const long long rows = a.rows_prog + (long long)batch * seq * a.P;
  if (rows == 0) return DLWP_OK;
  DLWP_REQUIRE(a.tpr <= INT64_MAX / rows, DLWP_ERR_INVALID_ARGUMENT, "dataset gather: bad shape");
  a.tiles = rows * a.tpr;
  hipLaunchKernelGGL(dataset::gather_kernel, dim3(dataset::grid_for(a.tiles, dataset::MAX_BLOCKS)), dim3(dataset::NT), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" size_t dlwp_dataset_stats_workspace_bytes(int32_t n_vars) {
  if (n_vars <= 0) return 0;
  return ((size_t)n_vars * dataset::STAT_BLOCKS * 2 + (size_t)n_vars) * sizeof(double);
}

extern "C" int32_t dlwp_dataset_stats_f64(const float* store_dev, int64_t n_times, int32_t n_vars, int64_t plane,
                                          const int32_t* frames_dev, int64_t n_frames, double* out_dev, void* workspace_dev,
                                          size_t workspace_bytes, void* stream) {
  DLWP_REQUIRE(store_dev && frames_dev && out_dev && workspace_dev, DLWP_ERR_INVALID_ARGUMENT, "dataset stats: null argument");
  DLWP_REQUIRE(n_times > 0 && n_times <= INT32_MAX && n_vars > 0 && n_vars <= 65535 && plane > 0 && n_frames > 0,
               DLWP_ERR_INVALID_ARGUMENT, "dataset stats: bad shape (T %lld, V %d, plane %lld, %lld frames)", (long long)n_times,
               n_vars, (long long)plane, (long long)n_frames);
  DLWP_REQUIRE(workspace_bytes >= dlwp_dataset_stats_workspace_bytes(n_vars), DLWP_ERR_INVALID_ARGUMENT,
               "dataset stats: workspace of %zu bytes, %zu needed", workspace_bytes, dlwp_dataset_stats_workspace_bytes(n_vars));
  DLWP_REQUIRE(dataset::host_aligned(store_dev, 4) && dataset::host_aligned(out_dev, 8) && dataset::host_aligned(workspace_dev, 8),
               DLWP_ERR_INVALID_ARGUMENT, "dataset stats: the store must be 4-byte, the sums and the workspace 8-byte aligned");
  const long long nq = (plane + 3) / 4, tpr = (nq + dataset::NT - 1) / dataset::NT;
  DLWP_REQUIRE(tpr <= INT64_MAX / n_frames, DLWP_ERR_INVALID_ARGUMENT, "dataset stats: bad shape");
  double* partial = reinterpret_cast<double*>(workspace_dev);
  double* mean = partial + (size_t)n_vars * dataset::STAT_BLOCKS * 2;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(dataset::STAT_BLOCKS, (unsigned)n_vars), fin((unsigned)((n_vars + 63) / 64));
  hipLaunchKernelGGL(dataset::stats_pass_kernel<1>, grid, dim3(dataset::NT), 0, s, store_dev, frames_dev, (long long)n_frames,
                     (long long)n_times, n_vars, (long long)plane, nq, tpr, (const double*)mean, partial);
  hipLaunchKernelGGL(dataset::stats_finish_kernel<1>, fin, dim3(64), 0, s, (const double*)partial, n_vars, dataset::STAT_BLOCKS, mean,
                     out_dev);
  hipLaunchKernelGGL(dataset::stats_pass_kernel<2>, grid, dim3(dataset::NT), 0, s, store_dev, frames_dev, (long long)n_frames,
                     (long long)n_times, n_vars, (long long)plane, nq, tpr, (const double*)mean, partial);
  hipLaunchKernelGGL(dataset::stats_finish_kernel<2>, fin, dim3(64), 0, s, (const double*)partial, n_vars, dataset::STAT_BLOCKS, mean,
                     out_dev);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" int32_t dlwp_dataset_group_mean_f32(const float* store_dev, int64_t n_times, int32_t n_vars, int64_t plane,
                                               const int32_t* frames_dev, const int32_t* groups_dev, int64_t n_frames,
                                               int32_t n_groups, float* out_dev, void* stream) {
  DLWP_REQUIRE(store_dev && frames_dev && groups_dev && out_dev, DLWP_ERR_INVALID_ARGUMENT, "dataset group mean: null argument");
  DLWP_REQUIRE(n_times > 0 && n_times <= INT32_MAX && n_vars > 0 && plane > 0 && n_frames > 0 && n_groups > 0,
               DLWP_ERR_INVALID_ARGUMENT, "dataset group mean: bad shape (T %lld, V %d, plane %lld, %lld frames, %d groups)",
               (long long)n_times, n_vars, (long long)plane, (long long)n_frames, n_groups);
  DLWP_REQUIRE(dataset::host_aligned(store_dev, 4) && dataset::host_aligned(out_dev, 4), DLWP_ERR_INVALID_ARGUMENT,
               "dataset group mean: tensors must be 4-byte aligned");
  const long long nq = (plane + 3) / 4, tpr = (nq + dataset::NT - 1) / dataset::NT;
  const long long rows = (long long)n_groups * n_vars;
  DLWP_REQUIRE(tpr <= INT64_MAX / rows, DLWP_ERR_INVALID_ARGUMENT, "dataset group mean: bad shape");
  const long long tiles = rows * tpr;
  hipLaunchKernelGGL(dataset::group_mean_kernel, dim3(dataset::grid_for(tiles, dataset::MAX_BLOCKS)), dim3(dataset::NT), 0,
                     reinterpret_cast<hipStream_t>(stream), store_dev, frames_dev, groups_dev, (long long)n_frames,
                     (long long)n_times, n_vars, (long long)plane, nq, tpr, tiles, out_dev);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" int32_t dlwp_coarsen_mean_f32(const float* in_dev, float* out_dev, int64_t planes, int32_t height, int32_t width,
                                         int32_t k, void* stream) {
  DLWP_REQUIRE(in_dev && out_dev, DLWP_ERR_INVALID_ARGUMENT, "coarsen: null argument");
  DLWP_REQUIRE(planes > 0 && height > 0 && width > 0 && k > 0, DLWP_ERR_INVALID_ARGUMENT, "coarsen: bad shape [%lld, %d, %d] / %d",
               (long long)planes, height, width, k);
  // xarray's coarsen(boundary="exact"), the default the reference uses, raises for a ragged edge
  DLWP_REQUIRE(height % k == 0 && width % k == 0, DLWP_ERR_INVALID_ARGUMENT, "coarsen: %d x %d is not divisible by %d", height, width, k);
  DLWP_REQUIRE(dataset::host_aligned(in_dev, 4) && dataset::host_aligned(out_dev, 4), DLWP_ERR_INVALID_ARGUMENT,
               "coarsen: tensors must be 4-byte aligned");
  const int ho = height / k, wo = width / k;
  DLWP_REQUIRE(planes <= INT64_MAX / height / width, DLWP_ERR_INVALID_ARGUMENT, "coarsen: bad shape");
  const bool vec = (k == 2 || k == 4) && wo % 4 == 0 && dataset::host_aligned(in_dev, 16) && dataset::host_aligned(out_dev, 16);
  const long long units = planes * ho * (vec ? wo / 4 : wo);
  const dim3 grid(dataset::grid_for((units + dataset::NT - 1) / dataset::NT, dataset::MAX_BLOCKS)), block(dataset::NT);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (vec && k == 2)
    hipLaunchKernelGGL(dataset::coarsen_kernel<2>, grid, block, 0, s, in_dev, out_dev, units, ho, wo, k);
  else if (vec)
    hipLaunchKernelGGL(dataset::coarsen_kernel<4>, grid, block, 0, s, in_dev, out_dev, units, ho, wo, k);
  else
    hipLaunchKernelGGL(dataset::coarsen_kernel<0>, grid, block, 0, s, in_dev, out_dev, units, ho, wo, k);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}
