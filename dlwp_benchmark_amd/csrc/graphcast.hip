// GraphCastNet on MI355X (gfx950): a wide gather-GEMM for every MLP of the step.
//
// Replaces the arithmetic of the reference GraphCastNet (models/graphcast/graph_cast_net.py) built from MeshGraphMLP,
// MeshGraphEdgeMLPConcat (gnn_layers/mesh_graph_mlp.py), the encoder / processor / decoder blocks and
// aggregate_and_concat (gnn_layers/utils.py).  Two entry points; models/graphcast.py (through ops.gc_*) chains them into the
// MLPs of the step:
//
//   dlwp_gc_linear_f32      one Linear, out = act(A W^T + b [+ P_src[src] + P_dst[dst]]) [+ res], on a 64 x 128 output
//                           tile per workgroup (four waves of 32 x 64), K staged through LDS 32 deep.  The A operand is
//                           gathered while it is staged:
//                             mode 0  rows of a [rows, lda] table per sample (batch stride 0: one table for the batch),
//                             mode 1  channels-first [B, K, rows] (the grid embedder reads x_t as the rollout assembles it),
//                             mode 2  [agg_{edges into n} e, x_n]: the node MLP's concat (utils.py:379 order), the aggregate
//                                     summed in CSC order while the tile is staged -- neither the aggregate nor the concat
//                                     exists in memory.
//                           The epilogue gathers two per-node products by the edge's source / destination: the first Linear
//                           of an edge MLP on [e, x_src, x_dst] is W_e e + (W_s x_src)[src] + (W_d x_dst)[dst] + b, where
//                           the node products are computed once per node (one more dlwp_gc_linear_f32 per node table), so
//                           no [E, 3D] concat is built and the 2D-deep part of the product runs once per node, not per edge.
//                           The output is row-major or channels-first [B, N, rows] (the final MLP writes [B, C, H, W]) and
//                           may take a residual in its own layout (the rollout's prognostic_t[:, -1] + step).
//                           Training adds two flags (both off by default): act on the A load (a hidden Linear reads
//                           act(z) of the saved pre-activation z, so act(z) never exists in memory) and an epilogue factor
//                           act'(z) (the data gradient (dZ W) * act'(z) of a hidden Linear; csrc/graphcast_bwd.hip).
//   dlwp_gc_layernorm_f32   LayerNorm over rows (two-pass, biased variance, like torch) plus an optional residual, one
//                           wave per row; may run in place.
//
// Products are v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulation.  Every weight is read once per 64-row tile.
// Every output element has one writer and every sum runs in a fixed order (k order in the MFMA chain, CSC order in the
// aggregate): no atomics, bitwise reproducible, and a sample's result does not depend on its batch neighbours.
#include "gc_common.hpp"

namespace dlwp {
namespace gc {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int BM = 64;                 // rows per tile
constexpr int BN = 128;                // output columns per tile
constexpr int BK = 32;                 // K per LDS stage
constexpr int LDA = BM + 17;           // k-major A tile: the row-major stash (32 lanes along k) hits 17 k mod 64, 32
                                       //   distinct banks; the 16 x 4 MFMA operand (17 k + i) is at most 2-way
constexpr int LDB = BN + 16;           // B tile: the 16 x 4 operand hits 64 distinct banks (16 k + i)
constexpr int kMaxWidth = 512;         // hidden / output widths (envelope of the model)
constexpr int kMaxIn = 4096;           // input width of one Linear

struct Args {
  int mode;
  const float* a;
  long long a_bs;
  int lda;
  const float* e;
  long long e_bs;
  int agg_w;
  const int* row_ptr;
  int agg_mean;
  const float* wt;
  const float* bias;
  int K, N, rows;
  long long M;
  const float* ps;
  const int* src;
  long long ps_bs;
  int ld_ps;
  const float* pd;
  const int* dst;
  long long pd_bs;
  int ld_pd;
  int act;
  float* out;
  int out_layout;
  int ldo;
  long long out_bs;
  const float* res;
  long long res_bs;
  int a_act;                           // act applied to A as it is loaded (modes 0 / 1)
  const float* gz;                     // epilogue v *= act'(gz[m * ld_gz + j]) (the data gradient of a hidden Linear)
  int gz_act;
  int ld_gz;
};

// One staging row of the A tile, decomposed once per thread before the K loop: the row's base offset in `a` (mode 1: its
// column p of the channels-first block), mode 2's edge range and the sample's edge-table base.  rows past M have ok = 0.
struct ARow {
  long long off, e_off;
  int j0, j1;
  bool ok;
};

__device__ __forceinline__ ARow a_row(const Args& p, long long m) {
  ARow r{0, 0, 0, 0, m < p.M};
  if (!r.ok) return r;
  const long long b = m / p.rows, q = m - b * p.rows;
  r.off = b * p.a_bs + (p.mode == 1 ? q : q * p.lda);
  if (p.mode == 2) {
    r.e_off = b * p.e_bs;
    r.j0 = p.row_ptr[q];
    r.j1 = p.row_ptr[q + 1];
  }
  return r;
}

// A-tile element (row described by `r`, column k); zero outside [M, K)
// (graphcast_bwd.hip's load_a reads the same operand, decomposing the row per element)
__device__ __forceinline__ float load_a(const Args& p, const ARow& r, int k) {
  if (!r.ok || k >= p.K) return 0.f;
  if (p.mode == 1) return p.a[r.off + (long long)k * p.rows];
  if (p.mode == 2) {
    if (k < p.agg_w) {
      const float* e = p.e + r.e_off + k;
      float s = 0.f;
      for (int j = r.j0; j < r.j1; ++j) s += e[(long long)j * p.agg_w];
      if (p.agg_mean && r.j1 > r.j0) s = s / (float)(r.j1 - r.j0);
      return s;
    }
    k -= p.agg_w;
  }
  return p.a[r.off + k];
}

__global__ void __launch_bounds__(kThreads) linear_kernel(const Args p) {
  __shared__ float As[BK * LDA];
  __shared__ float Bs[BK * LDB];
  const int t = threadIdx.x, wave = t / kWave, lane = t % kWave;
  const int li = lane & 15, lk = lane >> 4;
  const int wr = wave >> 1, wc = wave & 1;
  const long long m0 = (long long)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;

  // staging maps: row-major A reads along k (coalesced per row), channels-first A along rows
  const bool cf = p.mode == 1;
  const int a_k = cf ? t / BM : t % BK;
  const int a_r = cf ? t % BM : t / BK;
  const int a_kstep = cf ? kThreads / BM : 0, a_rstep = cf ? 0 : kThreads / BK;
  const int b_c = t % BN, b_k = t / BN;
  const int col = n0 + b_c;

  // channels-first: the thread's 8 elements share one row; row-major: 8 rows
  ARow arow[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) arow[i] = (cf && i) ? arow[0] : a_row(p, m0 + a_r + i * a_rstep);

  float ra[8], rb[16];
  auto fetch = [&](int k0) {
    if (p.mode == 2 && k0 + a_k < p.agg_w) {
      // the aggregate: the thread's 8 rows share column k, so their edge sums run interleaved, U edge steps of loads in
      // flight at once instead of 8 serial chains; each row still adds in CSC order (skipped steps add nothing)
      const int k = k0 + a_k;
      int n_max = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        ra[i] = 0.f;
        n_max = max(n_max, arow[i].j1 - arow[i].j0);
      }
      constexpr int U = 4;          // edge steps whose loads are in flight together (32 loads per thread)
      for (int jj = 0; jj < n_max; jj += U) {
        float v[U][8];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int i = 0; i < 8; ++i)
            v[u][i] = jj + u < arow[i].j1 - arow[i].j0
                          ? p.e[arow[i].e_off + (long long)(arow[i].j0 + jj + u) * p.agg_w + k] : 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int i = 0; i < 8; ++i)
            if (jj + u < arow[i].j1 - arow[i].j0) ra[i] += v[u][i];
      }
      if (p.agg_mean) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (arow[i].j1 > arow[i].j0) ra[i] = ra[i] / (float)(arow[i].j1 - arow[i].j0);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) ra[i] = load_a(p, arow[i], k0 + a_k + i * a_kstep);
      if (p.a_act) {                  // act(0) = 0: the zero padding stays zero
#pragma unroll
        for (int i = 0; i < 8; ++i) ra[i] = activate(ra[i], p.a_act);
      }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int k = k0 + b_k + 2 * i;
      rb[i] = (k < p.K && col < p.N) ? p.wt[(long long)k * p.N + col] : 0.f;
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int i = 0; i < 8; ++i) As[(a_k + i * a_kstep) * LDA + a_r + i * a_rstep] = ra[i];
#pragma unroll
    for (int i = 0; i < 16; ++i) Bs[(b_k + 2 * i) * LDB + b_c] = rb[i];
  };

  f32x4 acc[2][4];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  fetch(0);
  for (int k0 = 0; k0 < p.K; k0 += BK) {
    __syncthreads();                  // the previous stage's reads are done
    stash();
    __syncthreads();
    if (k0 + BK < p.K) fetch(k0 + BK);  // the next stage's loads overlap this stage's products
#pragma unroll
    for (int kk = 0; kk < BK; kk += 4) {
      const float* ak = As + (kk + lk) * LDA + wr * 32 + li;
      const float* bk = Bs + (kk + lk) * LDB + wc * 64 + li;
      const float a0 = ak[0], a1 = ak[16];
      float b[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) b[c] = bk[16 * c];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        acc[0][c] = mfma16x16x4(a0, b[c], acc[0][c]);
        acc[1][c] = mfma16x16x4(a1, b[c], acc[1][c]);
      }
    }
  }

  // epilogue: lane holds D[4 lk + i][li] of each 16 x 16 tile
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int j = n0 + wc * 64 + 16 * c + li;
    if (j >= p.N) continue;
    const float bj = p.bias[j];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long m = m0 + wr * 32 + 16 * r + 4 * lk + i;
        if (m >= p.M) continue;
        const long long b = m / p.rows, q = m - b * p.rows;
        float v = acc[r][c][i] + bj;
        if (p.ps) v += p.ps[b * p.ps_bs + (long long)p.src[q] * p.ld_ps + j];
        if (p.pd) v += p.pd[b * p.pd_bs + (long long)p.dst[q] * p.ld_pd + j];
        v = activate(v, p.act);
        if (p.gz) v *= activate_grad(p.gz[m * p.ld_gz + j], p.gz_act);
        const long long o = p.out_layout == 1 ? b * p.out_bs + (long long)j * p.rows + q : m * p.ldo + j;
        if (p.res) v += p.res[(p.out_layout == 1 ? b * p.res_bs + (long long)j * p.rows + q : b * p.res_bs + q * p.ldo + j)];
        p.out[o] = v;
      }
  }
}

// out[m] = LN(in[m]) * g + beta [+ res], one wave per row of width d <= kMaxWidth (8 values per lane)
__global__ void __launch_bounds__(kThreads) layernorm_kernel(const float* in, float* out, long long rows_total, int d,
                                                             const float* __restrict__ g, const float* __restrict__ beta,
                                                             float eps, const float* res, long long res_bs, int res_rows) {
  const long long m = (long long)blockIdx.x * (kThreads / kWave) + threadIdx.x / kWave;
  const int lane = threadIdx.x % kWave;
  if (m >= rows_total) return;
  constexpr int V = kMaxWidth / kWave;
  float x[V];
  const float* row = in + m * d;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const int k = lane + i * kWave;
    x[i] = k < d ? row[k] : 0.f;
    s += x[i];
  }
  const float mean = wave_sum(s) / (float)d;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const int k = lane + i * kWave;
    const float c = k < d ? x[i] - mean : 0.f;
    q = fmaf(c, c, q);
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)d + eps);
  const float* rr = res ? res + (m / res_rows) * res_bs + (m % res_rows) * d : nullptr;
  float* o = out + m * d;
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const int k = lane + i * kWave;
    if (k < d) {
      float v = fmaf((x[i] - mean) * rstd, g[k], beta[k]);
      if (rr) v += rr[k];
      o[k] = v;
    }
  }
}

}  // namespace gc
}  // namespace dlwp

using namespace dlwp;

extern "C" int32_t dlwp_gc_linear_f32(const dlwp_gc_linear_args* a, void* stream) {
  DLWP_REQUIRE(a, DLWP_ERR_INVALID_ARGUMENT, "gc linear: null arguments");
  DLWP_REQUIRE(a->a_mode >= 0 && a->a_mode <= 2, DLWP_ERR_INVALID_ARGUMENT, "gc linear: A mode %d", a->a_mode);
  DLWP_REQUIRE(a->k > 0 && a->n > 0 && a->batch > 0 && a->rows > 0, DLWP_ERR_INVALID_ARGUMENT,
               "gc linear: k %d n %d batch %d rows %d", a->k, a->n, a->batch, a->rows);
  DLWP_REQUIRE(a->k <= gc::kMaxIn && a->n <= gc::kMaxWidth, DLWP_ERR_UNSUPPORTED, "gc linear: %d -> %d is outside the envelope",
               a->k, a->n);
  DLWP_REQUIRE(a->batch <= 65535, DLWP_ERR_UNSUPPORTED, "gc linear: batch %d", a->batch);
  DLWP_REQUIRE(a->a && a->wt && a->bias && a->out, DLWP_ERR_INVALID_ARGUMENT, "gc linear: null tensor");
  DLWP_REQUIRE(a->act >= 0 && a->act <= 2, DLWP_ERR_UNSUPPORTED, "gc linear: activation %d", a->act);
  DLWP_REQUIRE(a->out_layout == 0 || a->out_layout == 1, DLWP_ERR_INVALID_ARGUMENT, "gc linear: out layout %d", a->out_layout);
  if (a->a_mode == 2) {
    DLWP_REQUIRE(a->agg_e && a->row_ptr, DLWP_ERR_INVALID_ARGUMENT, "gc linear: aggregate without edges / row_ptr");
    DLWP_REQUIRE(a->agg_width > 0 && a->agg_width < a->k && a->lda >= a->k - a->agg_width, DLWP_ERR_INVALID_ARGUMENT,
                 "gc linear: aggregate width %d of %d (lda %d)", a->agg_width, a->k, a->lda);
    DLWP_REQUIRE(a->agg_mean == 0 || a->agg_mean == 1, DLWP_ERR_UNSUPPORTED, "gc linear: aggregation %d", a->agg_mean);
  } else if (a->a_mode == 0) {
    DLWP_REQUIRE(a->lda >= a->k, DLWP_ERR_INVALID_ARGUMENT, "gc linear: lda %d < k %d", a->lda, a->k);
  }
  DLWP_REQUIRE(!a->src_products == !a->src_index && !a->dst_products == !a->dst_index, DLWP_ERR_INVALID_ARGUMENT,
               "gc linear: a gathered product needs its index");
  DLWP_REQUIRE(a->out_layout == 1 || a->ldo >= a->n, DLWP_ERR_INVALID_ARGUMENT, "gc linear: ldo %d < n %d", a->ldo, a->n);
  DLWP_REQUIRE((const float*)a->out != a->a && (const float*)a->out != a->agg_e, DLWP_ERR_INVALID_ARGUMENT,
               "gc linear: the output may not alias the A operand");
  DLWP_REQUIRE(a->a_act >= 0 && a->a_act <= 2 && (a->a_act == 0 || a->a_mode != 2), DLWP_ERR_UNSUPPORTED,
               "gc linear: A activation %d in mode %d", a->a_act, a->a_mode);
  DLWP_REQUIRE(!a->act_grad_z || (a->act_grad >= 1 && a->act_grad <= 2 && a->out_layout == 0 && a->ld_act_grad_z >= a->n),
               DLWP_ERR_INVALID_ARGUMENT, "gc linear: act' epilogue %d (ld %d, out layout %d)", a->act_grad,
               a->ld_act_grad_z, a->out_layout);
  gc::Args p;
  p.mode = a->a_mode;
  p.a = a->a;
  p.a_bs = a->a_batch_stride;
  p.lda = a->lda;
  p.e = a->agg_e;
  p.e_bs = a->agg_batch_stride;
  p.agg_w = a->agg_width;
  p.row_ptr = a->row_ptr;
  p.agg_mean = a->agg_mean;
  p.wt = a->wt;
  p.bias = a->bias;
  p.K = a->k;
  p.N = a->n;
  p.rows = a->rows;
  p.M = (long long)a->batch * a->rows;
  p.ps = a->src_products;
  p.src = a->src_index;
  p.ps_bs = a->src_products_batch_stride;
  p.ld_ps = a->ld_src_products;
  p.pd = a->dst_products;
  p.dst = a->dst_index;
  p.pd_bs = a->dst_products_batch_stride;
  p.ld_pd = a->ld_dst_products;
  p.act = a->act;
  p.out = a->out;
  p.out_layout = a->out_layout;
  p.ldo = a->ldo;
  p.out_bs = a->out_layout == 1 ? (long long)a->n * a->rows : 0;
  p.res = a->res;
  p.res_bs = a->res_batch_stride;
  p.a_act = a->a_act;
  p.gz = a->act_grad_z;
  p.gz_act = a->act_grad;
  p.ld_gz = a->ld_act_grad_z;
  const long long mt = (p.M + gc::BM - 1) / gc::BM;
  DLWP_REQUIRE(mt <= INT32_MAX, DLWP_ERR_UNSUPPORTED, "gc linear: %lld rows", p.M);
  const dim3 grid((unsigned)mt, (unsigned)((a->n + gc::BN - 1) / gc::BN));
  hipLaunchKernelGGL(gc::linear_kernel, grid, dim3(gc::kThreads), 0, (hipStream_t)stream, p);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" int32_t dlwp_gc_layernorm_f32(const float* in_dev, float* out_dev, int32_t batch, int32_t rows, int32_t width,
                                         const float* gamma, const float* beta, float eps, const float* res_dev,
                                         int64_t res_batch_stride, void* stream) {
  DLWP_REQUIRE(in_dev && out_dev && gamma && beta, DLWP_ERR_INVALID_ARGUMENT, "gc layernorm: null tensor");
  DLWP_REQUIRE(batch > 0 && rows > 0 && width > 0, DLWP_ERR_INVALID_ARGUMENT, "gc layernorm: batch %d rows %d width %d", batch,
               rows, width);
  DLWP_REQUIRE(width <= gc::kMaxWidth, DLWP_ERR_UNSUPPORTED, "gc layernorm: width %d", width);
  const long long total = (long long)batch * rows;
  const long long blocks = (total + gc::kThreads / gc::kWave - 1) / (gc::kThreads / gc::kWave);
  DLWP_REQUIRE(blocks <= INT32_MAX, DLWP_ERR_UNSUPPORTED, "gc layernorm: %lld rows", total);
  hipLaunchKernelGGL(gc::layernorm_kernel, dim3((unsigned)blocks), dim3(gc::kThreads), 0, (hipStream_t)stream, in_dev, out_dev,
                     total, width, gamma, beta, eps, res_dev, (long long)res_batch_stride, rows);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}
