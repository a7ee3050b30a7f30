// GraphCastNet training on MI355X (gfx950): the backward pieces beside the forward gather-GEMM of csrc/graphcast.hip.
//
// training.gc_mlp / training.gc_layer (through ops.gc_*) differentiate every MLP of the step from its saved inputs, hidden
// pre-activations z_i and LayerNorm input.  The data gradients dA = dZ W run on dlwp_gc_linear_f32 (torch's [out][in]
// weight is its [k][n] operand; an act'(z) epilogue).  This file adds
//
//   dlwp_gc_weight_grad_f32    dW = A^T dZ (+ db), dW in torch's [out][in] layout.  The reduction runs over batch * rows
//                              rows (up to ~200k edge rows), split into row slices: grid (n tiles, k tiles, slices), a
//                              64 (out) x 128 (in) tile per workgroup, four waves of 32 x 64, rows staged through a
//                              double-buffered LDS stage 32 deep (one barrier per stage; the next stage's loads are in
//                              flight during this stage's 32 MFMAs per wave).  A is gathered with the forward's modes
//                              (dense / batch-stride-0 rows, channels-first, [agg, x]) and may be act(z) of a saved
//                              pre-activation; dZ is row-major or channels-first.  Each workgroup writes its partial tile
//                              to the workspace; sum_slices_kernel adds the slices in order.
//   dlwp_gc_layernorm_bwd_f32  LayerNorm backward, one wave per row, mean / rstd recomputed from the saved input; the row
//                              gradient may add the node MLP's aggregate gradient gathered by the edge's destination
//                              (/ in-degree), so ge'_tot = ge' + g_agg[dst] never takes a pass of its own.  dgamma / dbeta
//                              as per-workgroup partials summed in order.
//   dlwp_gc_segment_sum_f32    per-node sums of edge rows in CSC order or through a CSR-by-source permutation (the source /
//                              destination products' gradients), optionally summed over the batch (shared tables).
//
// Products are v_mfma_f32_16x16x4_f32 (exact fp32 products).  No atomics: every sum has a fixed order, so gradients are
// bitwise reproducible for a given shape.
#include "gc_common.hpp"

namespace dlwp {
namespace gcb {

using gc::activate;

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int TN = 64;                 // dW rows (output features) per tile
constexpr int TK = 128;                // dW columns (input features) per tile
constexpr int BR = 32;                 // reduction rows per LDS stage
constexpr int LDZ = TN + 16;           // the 16 x 4 MFMA operand (lk * 80 + li) hits 64 distinct banks
constexpr int LDX = TK + 16;           // likewise (lk * 144 + li)
constexpr int kMaxWidth = 512;
constexpr int kMaxIn = 4096;
constexpr int kMaxSlices = 64;
constexpr size_t kMaxPartialBytes = 32u << 20;   // dW partials: small next to the saved activations
constexpr int kLnBlocks = 512;         // LayerNorm backward workgroups (fixed: the dgamma / dbeta partial order)

struct WgArgs {
  int mode;
  const float* a;
  long long a_bs;
  int lda;
  const float* e;
  long long e_bs;
  int agg_w;
  const int* row_ptr;
  int agg_mean;
  int a_act;
  int K, N, rows;
  long long M;
  const float* dz;
  int dz_layout;
  int ldz;
  long long rows_per_slice;
  float* part;                         // [slices][N][K]
  float* part_b;                       // [slices][N] or null
};

// A[m][k] of the forward's operand (zero outside [0, M) x [0, K)); graphcast.hip's load_a reads it from a precomputed ARow
__device__ __forceinline__ float load_a(const WgArgs& p, long long m, int k) {
  if (m >= p.M || k >= p.K) return 0.f;
  const long long b = m / p.rows, q = m - b * p.rows;
  if (p.mode == 1) return activate(p.a[b * p.a_bs + (long long)k * p.rows + q], p.a_act);
  if (p.mode == 2) {
    if (k < p.agg_w) {
      const int j0 = p.row_ptr[q], j1 = p.row_ptr[q + 1];
      const float* e = p.e + b * p.e_bs + k;
      float s = 0.f;
      for (int j = j0; j < j1; ++j) s += e[(long long)j * p.agg_w];
      if (p.agg_mean && j1 > j0) s = s / (float)(j1 - j0);
      return s;
    }
    k -= p.agg_w;
  }
  return activate(p.a[b * p.a_bs + q * p.lda + k], p.a_act);
}

__device__ __forceinline__ float load_dz(const WgArgs& p, long long m, int j) {
  if (m >= p.M || j >= p.N) return 0.f;
  if (p.dz_layout == 1) {
    const long long b = m / p.rows, q = m - b * p.rows;
    return p.dz[(b * p.N + j) * p.rows + q];
  }
  return p.dz[m * p.ldz + j];
}

__global__ void __launch_bounds__(kThreads) weight_grad_kernel(const WgArgs p) {
  __shared__ float Zs[2][BR * LDZ];
  __shared__ float Xs[2][BR * LDX];
  const int t = threadIdx.x, wave = t / kWave, lane = t % kWave;
  const int li = lane & 15, lk = lane >> 4;
  const int wr = wave >> 1, wc = wave & 1;
  const int n0 = blockIdx.x * TN, k0 = blockIdx.y * TK;
  const long long r_begin = (long long)blockIdx.z * p.rows_per_slice;
  const long long r_end = r_begin + p.rows_per_slice < p.M ? r_begin + p.rows_per_slice : p.M;

  // staging maps: row-major operands read along the feature (coalesced per row), channels-first ones along rows
  const bool zcf = p.dz_layout == 1, xcf = p.mode == 1;
  const int z_c = zcf ? t / BR : t % TN, z_r = zcf ? t % BR : t / TN;
  const int z_cs = zcf ? kThreads / BR : 0, z_rs = zcf ? 0 : kThreads / TN;       // 8 elements per thread
  const int x_c = xcf ? t / BR : t % TK, x_r = xcf ? t % BR : t / TK;
  const int x_cs = xcf ? kThreads / BR : 0, x_rs = xcf ? 0 : kThreads / TK;       // 16 elements per thread

  float rz[8], rx[16];
  auto fetch = [&](long long r0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const long long m = r0 + z_r + i * z_rs;
      rz[i] = m < r_end ? load_dz(p, m, n0 + z_c + i * z_cs) : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const long long m = r0 + x_r + i * x_rs;
      rx[i] = m < r_end ? load_a(p, m, k0 + x_c + i * x_cs) : 0.f;
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 8; ++i) Zs[buf][(z_r + i * z_rs) * LDZ + z_c + i * z_cs] = rz[i];
#pragma unroll
    for (int i = 0; i < 16; ++i) Xs[buf][(x_r + i * x_rs) * LDX + x_c + i * x_cs] = rx[i];
  };

  f32x4 acc[2][4];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool do_bias = p.part_b && blockIdx.y == 0 && t < TN;
  float bsum = 0.f;

  int buf = 0;
  if (r_begin < r_end) {
    fetch(r_begin);
    stash(0);
  }
  __syncthreads();
  for (long long r0 = r_begin; r0 < r_end; r0 += BR) {
    const bool more = r0 + BR < r_end;
    if (more) fetch(r0 + BR);         // in flight during this stage's products
    const float* zb = Zs[buf];
    const float* xb = Xs[buf];
    if (do_bias) {
#pragma unroll 8
      for (int r = 0; r < BR; ++r) bsum += zb[r * LDZ + t];
    }
#pragma unroll
    for (int kk = 0; kk < BR; kk += 4) {
      const float* za = zb + (kk + lk) * LDZ + wr * 32 + li;
      const float* xa = xb + (kk + lk) * LDX + wc * 64 + li;
      const float a0 = za[0], a1 = za[16];
      float b[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) b[c] = xa[16 * c];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        acc[0][c] = mfma16x16x4(a0, b[c], acc[0][c]);
        acc[1][c] = mfma16x16x4(a1, b[c], acc[1][c]);
      }
    }
    if (more) stash(buf ^ 1);         // the other buffer was last read before the previous barrier
    __syncthreads();
    buf ^= 1;
  }

  // partial tile: lane holds dW[n0 + wr 32 + 16 r + 4 lk + i][k0 + wc 64 + 16 c + li]
  float* part = p.part + (long long)blockIdx.z * p.N * p.K;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int k = k0 + wc * 64 + 16 * c + li;
    if (k >= p.K) continue;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int n = n0 + wr * 32 + 16 * r + 4 * lk + i;
        if (n < p.N) part[(long long)n * p.K + k] = acc[r][c][i];
      }
  }
  if (do_bias && n0 + t < p.N) p.part_b[(long long)blockIdx.z * p.N + n0 + t] = bsum;
}

// out[r * ldo + c] = sum_{s < S} part[s * stride + r * cols + c], s in order
__global__ void __launch_bounds__(kThreads) sum_slices_kernel(const float* __restrict__ part, int S, long long stride,
                                                              int rows, int cols, float* __restrict__ out, int ldo) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (long long)rows * cols) return;
  float s = 0.f;
  for (int k = 0; k < S; ++k) s += part[k * stride + i];
  out[(i / cols) * ldo + i % cols] = s;
}

struct LnArgs {
  const float* x;
  const float* gamma;
  float eps;
  const float* gy;
  const float* g_agg;
  long long g_agg_bs;
  const int* idx;
  const int* deg;
  long long total;
  int rows, d;
  float* g_total;
  float* gx;
  float* part;                         // [blocks][2][d]
};

__global__ void __launch_bounds__(kThreads) layernorm_bwd_kernel(const LnArgs p) {
  constexpr int W = kThreads / kWave;
  constexpr int V = kMaxWidth / kWave;
  __shared__ float red[W][2][kMaxWidth];
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int d = p.d;
  float pg[V], pb[V];
#pragma unroll
  for (int i = 0; i < V; ++i) pg[i] = pb[i] = 0.f;
  for (long long m = (long long)blockIdx.x * W + wave; m < p.total; m += (long long)gridDim.x * W) {
    const long long b = m / p.rows, q = m - b * p.rows;
    const float* xr = p.x + m * d;
    float x[V], g[V];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const int k = lane + i * kWave;
      x[i] = k < d ? xr[k] : 0.f;
      s += x[i];
    }
    const float mean = wave_sum(s) / (float)d;
    float qs = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const int k = lane + i * kWave;
      const float c = k < d ? x[i] - mean : 0.f;
      qs = fmaf(c, c, qs);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(qs) / (float)d + p.eps);
    const float* ga = nullptr;
    float scale = 1.f;
    if (p.g_agg) {
      const int n = p.idx[q];
      ga = p.g_agg + b * p.g_agg_bs + (long long)n * d;
      if (p.deg) scale = 1.0f / (float)max(p.deg[n], 1);
    }
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const int k = lane + i * kWave;
      float gv = 0.f;
      if (k < d) {
        if (p.gy) gv = p.gy[m * d + k];
        if (ga) gv += p.deg ? ga[k] * scale : ga[k];
        if (p.g_total) p.g_total[m * d + k] = gv;
        x[i] = (x[i] - mean) * rstd;              // xhat
        pg[i] = fmaf(gv, x[i], pg[i]);
        pb[i] += gv;
        g[i] = gv * p.gamma[k];                   // d xhat
        s1 += g[i];
        s2 = fmaf(g[i], x[i], s2);
      } else {
        g[i] = 0.f;
      }
    }
    const float m1 = wave_sum(s1) / (float)d, m2 = wave_sum(s2) / (float)d;
    float* o = p.gx + m * d;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const int k = lane + i * kWave;
      if (k < d) o[k] = rstd * (g[i] - m1 - x[i] * m2);
    }
  }
  // per-workgroup dgamma / dbeta: the waves' partials added in wave order
#pragma unroll
  for (int i = 0; i < V; ++i) {
    red[wave][0][lane + i * kWave] = pg[i];
    red[wave][1][lane + i * kWave] = pb[i];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < 2 * d; c += kThreads) {
    const int h = c / d, k = c - h * d;
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < W; ++w) s += red[w][h][k];
    p.part[(long long)blockIdx.x * 2 * d + c] = s;
  }
}

__global__ void __launch_bounds__(kThreads) segment_sum_kernel(const float* __restrict__ in, long long in_bs,
                                                               const int* __restrict__ row_ptr, const int* __restrict__ perm,
                                                               int n_seg, int d, int batch, int batch_sum,
                                                               float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  const long long per = (long long)n_seg * d;
  const int out_batches = batch_sum ? 1 : batch;
  if (i >= per * out_batches) return;
  const int bo = (int)(i / per);
  const long long r = i - bo * per;
  const int n = (int)(r / d), c = (int)(r - (long long)n * d);
  const int j0 = row_ptr ? row_ptr[n] : n, j1 = row_ptr ? row_ptr[n + 1] : n + 1;
  const int b0 = batch_sum ? 0 : bo, b1 = batch_sum ? batch : bo + 1;
  float s = 0.f;
  for (int b = b0; b < b1; ++b) {
    const float* base = in + b * in_bs + c;
    for (int j = j0; j < j1; ++j) s += base[(long long)(perm ? perm[j] : j) * d];
  }
  out[i] = s;
}

// the slicing of dlwp_gc_weight_grad_f32: a function of the shape alone (the partial order, so bitwise reproducibility)
struct Slicing {
  int slices;
  long long rows_per_slice;
};

__host__ inline Slicing slicing(int k, int n, long long m) {
  const long long tiles = (long long)((n + TN - 1) / TN) * ((k + TK - 1) / TK);
  const long long stages = (m + BR - 1) / BR;
  long long s = (1024 + tiles - 1) / tiles;                     // ~4 workgroups per CU
  s = std::min<long long>(s, (stages + 7) / 8);                  // at least 8 stages per slice
  s = std::min<long long>(s, (long long)(kMaxPartialBytes / ((size_t)k * n * sizeof(float))));
  s = std::max<long long>(1, std::min<long long>(s, kMaxSlices));
  const long long rps = ((stages + s - 1) / s) * BR;
  return Slicing{(int)((m + rps - 1) / rps), rps};
}

}  // namespace gcb
}  // namespace dlwp

using namespace dlwp;

extern "C" size_t dlwp_gc_weight_grad_workspace_bytes(int32_t k, int32_t n, int32_t batch, int32_t rows) {
  if (k <= 0 || n <= 0 || batch <= 0 || rows <= 0 || k > gcb::kMaxIn || n > gcb::kMaxWidth) return 0;
  const gcb::Slicing s = gcb::slicing(k, n, (long long)batch * rows);
  return (size_t)s.slices * ((size_t)n * k + n) * sizeof(float);
}

extern "C" int32_t dlwp_gc_weight_grad_f32(const dlwp_gc_linear_args* a, const float* dz, int32_t dz_layout, int32_t ldz,
                                           float* dw, int32_t ldw, float* db, void* workspace, size_t workspace_bytes,
                                           void* stream) {
  DLWP_REQUIRE(a && dz && dw, DLWP_ERR_INVALID_ARGUMENT, "gc weight grad: null argument");
  DLWP_REQUIRE(a->a, DLWP_ERR_INVALID_ARGUMENT, "gc weight grad: null A");
  DLWP_REQUIRE(a->a_mode >= 0 && a->a_mode <= 2, DLWP_ERR_INVALID_ARGUMENT, "gc weight grad: A mode %d", a->a_mode);
  DLWP_REQUIRE(a->k > 0 && a->n > 0 && a->batch > 0 && a->rows > 0, DLWP_ERR_INVALID_ARGUMENT,
               "gc weight grad: k %d n %d batch %d rows %d", a->k, a->n, a->batch, a->rows);
  DLWP_REQUIRE(a->k <= gcb::kMaxIn && a->n <= gcb::kMaxWidth, DLWP_ERR_UNSUPPORTED,
               "gc weight grad: %d -> %d is outside the envelope", a->k, a->n);
  DLWP_REQUIRE(a->a_act >= 0 && a->a_act <= 2 && (a->a_act == 0 || a->a_mode != 2), DLWP_ERR_UNSUPPORTED,
               "gc weight grad: A activation %d in mode %d", a->a_act, a->a_mode);
  DLWP_REQUIRE(dz_layout == 0 || dz_layout == 1, DLWP_ERR_INVALID_ARGUMENT, "gc weight grad: dz layout %d", dz_layout);
  DLWP_REQUIRE(dz_layout == 1 || ldz >= a->n, DLWP_ERR_INVALID_ARGUMENT, "gc weight grad: ldz %d < n %d", ldz, a->n);
  DLWP_REQUIRE(ldw >= a->k, DLWP_ERR_INVALID_ARGUMENT, "gc weight grad: ldw %d < k %d", ldw, a->k);
  if (a->a_mode == 2) {
    DLWP_REQUIRE(a->agg_e && a->row_ptr, DLWP_ERR_INVALID_ARGUMENT, "gc weight grad: aggregate without edges / row_ptr");
    DLWP_REQUIRE(a->agg_width > 0 && a->agg_width < a->k && a->lda >= a->k - a->agg_width, DLWP_ERR_INVALID_ARGUMENT,
                 "gc weight grad: aggregate width %d of %d (lda %d)", a->agg_width, a->k, a->lda);
    DLWP_REQUIRE(a->agg_mean == 0 || a->agg_mean == 1, DLWP_ERR_UNSUPPORTED, "gc weight grad: aggregation %d", a->agg_mean);
  } else if (a->a_mode == 0) {
    DLWP_REQUIRE(a->lda >= a->k, DLWP_ERR_INVALID_ARGUMENT, "gc weight grad: lda %d < k %d", a->lda, a->k);
  }
  const long long M = (long long)a->batch * a->rows;
  const size_t need = dlwp_gc_weight_grad_workspace_bytes(a->k, a->n, a->batch, a->rows);
  DLWP_REQUIRE(workspace && workspace_bytes >= need, DLWP_ERR_INVALID_ARGUMENT, "gc weight grad: workspace %zu < %zu",
               workspace_bytes, need);
  const gcb::Slicing sl = gcb::slicing(a->k, a->n, M);
  gcb::WgArgs p;
  p.mode = a->a_mode;
  p.a = a->a;
  p.a_bs = a->a_batch_stride;
  p.lda = a->lda;
  p.e = a->agg_e;
  p.e_bs = a->agg_batch_stride;
  p.agg_w = a->agg_width;
  p.row_ptr = a->row_ptr;
  p.agg_mean = a->agg_mean;
  p.a_act = a->a_act;
  p.K = a->k;
  p.N = a->n;
  p.rows = a->rows;
  p.M = M;
  p.dz = dz;
  p.dz_layout = dz_layout;
  p.ldz = ldz;
  p.rows_per_slice = sl.rows_per_slice;
  p.part = (float*)workspace;
  p.part_b = db ? p.part + (size_t)sl.slices * a->n * a->k : nullptr;
  const dim3 grid((unsigned)((a->n + gcb::TN - 1) / gcb::TN), (unsigned)((a->k + gcb::TK - 1) / gcb::TK), (unsigned)sl.slices);
  hipLaunchKernelGGL(gcb::weight_grad_kernel, grid, dim3(gcb::kThreads), 0, (hipStream_t)stream, p);
  DLWP_HIP_CHECK(hipGetLastError());
  const long long nk = (long long)a->n * a->k;
  hipLaunchKernelGGL(gcb::sum_slices_kernel, dim3((unsigned)((nk + gcb::kThreads - 1) / gcb::kThreads)), dim3(gcb::kThreads), 0,
                     (hipStream_t)stream, p.part, sl.slices, nk, a->n, a->k, dw, ldw);
  DLWP_HIP_CHECK(hipGetLastError());
  if (db) {
    hipLaunchKernelGGL(gcb::sum_slices_kernel, dim3((unsigned)((a->n + gcb::kThreads - 1) / gcb::kThreads)), dim3(gcb::kThreads),
                       0, (hipStream_t)stream, p.part_b, sl.slices, (long long)a->n, 1, a->n, db, a->n);
    DLWP_HIP_CHECK(hipGetLastError());
  }
  return DLWP_OK;
}

static int ln_blocks(long long total) {
  const long long need = (total + gcb::kThreads / gcb::kWave - 1) / (gcb::kThreads / gcb::kWave);
  return (int)std::max<long long>(1, std::min<long long>(need, gcb::kLnBlocks));
}

extern "C" size_t dlwp_gc_layernorm_bwd_workspace_bytes(int32_t batch, int32_t rows, int32_t width) {
  if (batch <= 0 || rows <= 0 || width <= 0 || width > gcb::kMaxWidth) return 0;
  return (size_t)ln_blocks((long long)batch * rows) * 2 * width * sizeof(float);
}

extern "C" int32_t dlwp_gc_layernorm_bwd_f32(const float* x, const float* gamma, float eps, const float* gy, const float* g_agg,
                                             int64_t g_agg_batch_stride, const int32_t* idx, const int32_t* deg, int32_t batch,
                                             int32_t rows, int32_t width, float* g_total, float* gx, float* dgamma,
                                             float* dbeta, void* workspace, size_t workspace_bytes, void* stream) {
  DLWP_REQUIRE(x && gamma && gx && dgamma && dbeta, DLWP_ERR_INVALID_ARGUMENT, "gc layernorm bwd: null tensor");
  DLWP_REQUIRE(gy || g_agg, DLWP_ERR_INVALID_ARGUMENT, "gc layernorm bwd: no output gradient");
  DLWP_REQUIRE(!g_agg || idx, DLWP_ERR_INVALID_ARGUMENT, "gc layernorm bwd: a gathered gradient needs its index");
  DLWP_REQUIRE(batch > 0 && rows > 0 && width > 0, DLWP_ERR_INVALID_ARGUMENT, "gc layernorm bwd: batch %d rows %d width %d",
               batch, rows, width);
  DLWP_REQUIRE(width <= gcb::kMaxWidth, DLWP_ERR_UNSUPPORTED, "gc layernorm bwd: width %d", width);
  const size_t need = dlwp_gc_layernorm_bwd_workspace_bytes(batch, rows, width);
  DLWP_REQUIRE(workspace && workspace_bytes >= need, DLWP_ERR_INVALID_ARGUMENT, "gc layernorm bwd: workspace %zu < %zu",
               workspace_bytes, need);
  gcb::LnArgs p;
  p.x = x;
  p.gamma = gamma;
  p.eps = eps;
  p.gy = gy;
  p.g_agg = g_agg;
  p.g_agg_bs = g_agg_batch_stride;
  p.idx = idx;
  p.deg = deg;
  p.total = (long long)batch * rows;
  p.rows = rows;
  p.d = width;
  p.g_total = g_total;
  p.gx = gx;
  p.part = (float*)workspace;
  const int blocks = ln_blocks(p.total);
  hipLaunchKernelGGL(gcb::layernorm_bwd_kernel, dim3(blocks), dim3(gcb::kThreads), 0, (hipStream_t)stream, p);
  DLWP_HIP_CHECK(hipGetLastError());
  const unsigned rb = (unsigned)((width + gcb::kThreads - 1) / gcb::kThreads);
  hipLaunchKernelGGL(gcb::sum_slices_kernel, dim3(rb), dim3(gcb::kThreads), 0, (hipStream_t)stream, p.part, blocks,
                     2LL * width, 1, width, dgamma, width);
  DLWP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(gcb::sum_slices_kernel, dim3(rb), dim3(gcb::kThreads), 0, (hipStream_t)stream, p.part + width, blocks,
                     2LL * width, 1, width, dbeta, width);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" int32_t dlwp_gc_segment_sum_f32(const float* in, int64_t in_batch_stride, const int32_t* row_ptr, const int32_t* perm,
                                           int32_t n_segments, int32_t width, int32_t batch, int32_t batch_sum, float* out,
                                           void* stream) {
  DLWP_REQUIRE(in && out, DLWP_ERR_INVALID_ARGUMENT, "gc segment sum: null tensor");
  DLWP_REQUIRE(n_segments > 0 && width > 0 && batch > 0, DLWP_ERR_INVALID_ARGUMENT,
               "gc segment sum: %d segments of width %d, batch %d", n_segments, width, batch);
  DLWP_REQUIRE(batch_sum == 0 || batch_sum == 1, DLWP_ERR_INVALID_ARGUMENT, "gc segment sum: batch_sum %d", batch_sum);
  DLWP_REQUIRE(!perm || row_ptr, DLWP_ERR_INVALID_ARGUMENT, "gc segment sum: a permutation needs its row_ptr");
  const long long total = (long long)n_segments * width * (batch_sum ? 1 : batch);
  const long long blocks = (total + gcb::kThreads - 1) / gcb::kThreads;
  DLWP_REQUIRE(blocks <= INT32_MAX, DLWP_ERR_UNSUPPORTED, "gc segment sum: %lld outputs", total);
  hipLaunchKernelGGL(gcb::segment_sum_kernel, dim3((unsigned)blocks), dim3(gcb::kThreads), 0, (hipStream_t)stream, in,
                     (long long)in_batch_stride, row_ptr, perm, n_segments, width, batch, batch_sum, out);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}
