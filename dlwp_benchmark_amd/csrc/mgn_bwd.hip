// MeshGraphNet training on MI355X (gfx950): the backward of dlwp_mgn_mlp_f32 and dlwp_mgn_processor_layer_f32.
//
// Differentiates the reference's MeshGraphMLP (models/graphcast/gnn_layers/mesh_graph_mlp.py), MeshEdgeBlock
// (mesh_edge_block.py), MeshNodeBlock (mesh_node_block.py) and the concat / aggregate helpers of utils.py
// (concat_message_function :96-111, agg_concat_dgl :340-380), which reference scripts/train.py:271 reaches through
// `loss.backward()`.  Nothing of the forward is saved except each layer's INPUTS: every kernel recomputes the forward of
// the rows it owns in LDS (flash-style) and backpropagates through it there.
//
//   mlp_bwd_kernel     one MeshGraphMLP over rows (the node / edge encoders and the node decoder): a tile of R rows is
//                      gathered, the Linear chain is recomputed keeping every Linear's input, the upstream gradient runs
//                      back through the LayerNorm and the chain, and the input gradient is written in the input's layout.
//   layer_bwd_kernel   pass (a) of one processor layer.  A workgroup owns T destination nodes of one sample and every
//                      edge into them (CSC order), as the forward does.  Pass 1 over the edge chunks recomputes e' and the
//                      per-node sums; the node MLP is recomputed and backpropagated (dx_out -> d[agg, x]); pass 2
//                      recomputes each edge chunk again and backpropagates de' = de_out + dagg[dst] (/ in-degree for mean)
//                      through the edge LayerNorm and MLP.  de_in is written per edge, the x_dst part of the edge input
//                      gradient is added into the owner's nodes in edge order, the x_src part goes to a [B, E, D] scratch.
//   src_gather_kernel  pass (b): dx_in[n] += the x_src parts of every edge leaving n, through a source-sorted permutation
//                      of the CSC edges (a CSR by source, built on the host once per graph).
//   sum_partials_kernel  pass (c): parameter gradients.  A capped grid of kPartials workgroups, two per CU, loops over
//                      the tiles; each accumulates its own partial of every parameter gradient (a read-add-write by the
//                      one thread that owns the element, in tile and chunk order) in LDS when the partial fits beside the
//                      tile with two workgroups per CU (then writes it once), else in its global partial row; this launch
//                      sums the rows in workgroup order.  The same launch sums a shared edge table's per-sample de_in over the batch.
//
// Every output element has one writer, every sum runs in a fixed order, no atomics: bitwise reproducible, and a sample's
// input gradients do not depend on its batch neighbours.  Products are fp32 FMA chains (exact fp32 products).
// Parameter gradients are laid out per MLP as [W_0 (d_0 x d_1, [in][out]), b_0, W_1, b_1, ..., gamma, beta].
//
// The forward's pieces that are recomputed here -- kThreads, kWave, round4, dense, layernorm_row, the base of Mlp -- and
// fill_mlp / set_lds are mgn_common.hpp's, the very definitions mgn.hip runs.
#include "mgn_common.hpp"

namespace dlwp {
namespace mgn_bwd {

using namespace mgn;   // what mgn_common.hpp defines there

constexpr int kWaves = kThreads / kWave;
constexpr int kMaxWidth = 64;         // hidden and output widths (include/dlwp_hip.h)
constexpr int kMaxMlpIn = 256;        // input width of dlwp_mgn_mlp_bwd_f32
constexpr size_t kLdsTwoPerCu = 80 * 1024;   // two workgroups share a CU's 160 KiB
constexpr int kPartials = 512;                // partial-writing workgroups: two per CU (MI355X: 256 CUs)

struct Mlp : MlpBase {
  float eps;
  int off_w[5];          // offsets in the parameter-gradient layout
  int off_b[5];
  int off_g;             // gamma at off_g, beta at off_g + dims[n]
  int n_params;
};

// dh[r][k] = sum_j dl[r][j] wt[k][j]  (the input gradient of one Linear, j order), times [mask[r][k] > 0] when mask is
// given (the ReLU in front of the Linear: mask is the ReLU's output, the Linear's input)
__device__ __forceinline__ void dense_t(const float* dl, int ldd, int n_out, float* dh, int ldh, int n_in,
                                        const float* __restrict__ wt, const float* mask, int ldm, int R) {
  const int pairs = (R >> 2) * n_in;
  for (int p = threadIdx.x; p < pairs; p += kThreads) {
    const int k = p % n_in, r0 = (p / n_in) * 4;
    const float* d0 = dl + r0 * ldd;
    const float* d1 = d0 + ldd;
    const float* d2 = d1 + ldd;
    const float* d3 = d2 + ldd;
    const float* w = wt + (size_t)k * n_out;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int j = 0;
    for (; j + 4 <= n_out; j += 4) {
      const float w0 = w[j], w1 = w[j + 1], w2 = w[j + 2], w3 = w[j + 3];
      const float4 x0 = *reinterpret_cast<const float4*>(d0 + j);
      const float4 x1 = *reinterpret_cast<const float4*>(d1 + j);
      const float4 x2 = *reinterpret_cast<const float4*>(d2 + j);
      const float4 x3 = *reinterpret_cast<const float4*>(d3 + j);
      a0 = fmaf(x0.x, w0, a0); a1 = fmaf(x1.x, w0, a1); a2 = fmaf(x2.x, w0, a2); a3 = fmaf(x3.x, w0, a3);
      a0 = fmaf(x0.y, w1, a0); a1 = fmaf(x1.y, w1, a1); a2 = fmaf(x2.y, w1, a2); a3 = fmaf(x3.y, w1, a3);
      a0 = fmaf(x0.z, w2, a0); a1 = fmaf(x1.z, w2, a1); a2 = fmaf(x2.z, w2, a2); a3 = fmaf(x3.z, w2, a3);
      a0 = fmaf(x0.w, w3, a0); a1 = fmaf(x1.w, w3, a1); a2 = fmaf(x2.w, w3, a2); a3 = fmaf(x3.w, w3, a3);
    }
    for (; j < n_out; ++j) {
      const float wj = w[j];
      a0 = fmaf(d0[j], wj, a0); a1 = fmaf(d1[j], wj, a1); a2 = fmaf(d2[j], wj, a2); a3 = fmaf(d3[j], wj, a3);
    }
    if (mask) {
      const float* m = mask + r0 * ldm + k;
      a0 = m[0] > 0.f ? a0 : 0.f;
      a1 = m[ldm] > 0.f ? a1 : 0.f;
      a2 = m[2 * ldm] > 0.f ? a2 : 0.f;
      a3 = m[3 * ldm] > 0.f ? a3 : 0.f;
    }
    float* o = dh + r0 * ldh + k;
    o[0] = a0; o[ldh] = a1; o[2 * ldh] = a2; o[3 * ldh] = a3;
  }
}

// this workgroup's partial of one Linear's weight and bias gradient over `rows` rows (row order):
//   pw[k][j] (+)= sum_r h[r][k] dl[r][j],   pb[j] (+)= sum_r dl[r][j]
// `first`: store instead of add.  The element -> thread map depends only on the widths, so every partial element is
// read and written by one thread of the workgroup, always the same one.
__device__ __forceinline__ void wgrad(const float* h, int ldh, int n_in, const float* dl, int ldd, int n_out, int rows,
                                      float* pw, float* pb, bool first) {
  const int nw = n_in * n_out;
  for (int p = threadIdx.x; p < nw + n_out; p += kThreads) {
    float s = 0.f;
    if (p < nw) {
      const int k = p / n_out, j = p % n_out;
      for (int r = 0; r < rows; ++r) s = fmaf(h[r * ldh + k], dl[r * ldd + j], s);
      pw[p] = first ? s : pw[p] + s;
    } else {
      const int j = p - nw;
      for (int r = 0; r < rows; ++r) s += dl[r * ldd + j];
      pb[j] = first ? s : pb[j] + s;
    }
  }
}

// LayerNorm gamma / beta partials: pg[j] (+)= sum_r xhat[r][j] dy[r][j], pbeta[j] (+)= sum_r dy[r][j]
__device__ __forceinline__ void ln_wgrad(const float* xh, int ldx, const float* dy, int ldy, int d, int rows, float* pg,
                                         bool first) {
  for (int p = threadIdx.x; p < 2 * d; p += kThreads) {
    const int j = p % d;
    float s = 0.f;
    if (p < d) {
      for (int r = 0; r < rows; ++r) s = fmaf(xh[r * ldx + j], dy[r * ldy + j], s);
    } else {
      for (int r = 0; r < rows; ++r) s += dy[r * ldy + j];
    }
    pg[p] = first ? s : pg[p] + s;
  }
}

// zero partial row for an MLP this workgroup never saw a row of (same element -> thread map as wgrad / ln_wgrad)
__device__ __forceinline__ void zero_partials(const Mlp& m, float* part) {
  for (int l = 0; l < m.n; ++l) {
    const int nw = m.dims[l] * m.dims[l + 1];
    for (int p = threadIdx.x; p < nw + m.dims[l + 1]; p += kThreads) {
      if (p < nw) part[m.off_w[l] + p] = 0.f;
      else part[m.off_b[l] + p - nw] = 0.f;
    }
  }
  if (m.g)
    for (int p = threadIdx.x; p < 2 * m.dims[m.n]; p += kThreads) part[m.off_g + p] = 0.f;
}

// LayerNorm backward of one row, one wave: z (the pre-norm row) is replaced by xhat, dz = rstd (dy g - mean(dy g)
// - xhat mean(dy g xhat))
__device__ __forceinline__ void layernorm_bwd_row(float* z, const float* dy, float* dz, int d, const float* __restrict__ g,
                                                  float eps, int lane) {
  float s = 0.f;
  for (int k = lane; k < d; k += kWave) s += z[k];
  const float mean = wave_sum(s) / (float)d;
  float q = 0.f;
  for (int k = lane; k < d; k += kWave) {
    const float c = z[k] - mean;
    q = fmaf(c, c, q);
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)d + eps);
  float s1 = 0.f, s2 = 0.f;
  for (int k = lane; k < d; k += kWave) {
    const float xh = (z[k] - mean) * rstd;
    const float gg = dy[k] * g[k];
    s1 += gg;
    s2 = fmaf(gg, xh, s2);
  }
  const float m1 = wave_sum(s1) / (float)d, m2 = wave_sum(s2) / (float)d;
  for (int k = lane; k < d; k += kWave) {
    const float xh = (z[k] - mean) * rstd;
    z[k] = xh;
    dz[k] = rstd * (dy[k] * g[k] - m1 - xh * m2);
  }
}

// LDS of one MLP's recomputation: h[0] the input tile [R][ld0], h[1..n-1] the hidden activations and h[n] the pre-norm
// output [R][ldh]; da / db the gradient ping-pong [R][ld0]
struct Tiles {
  float* h[6];
  int ld[6];
  float* da;
  float* db;
  int ldg;
};

// forward chain over R rows keeping every Linear's input; h[0] is filled
__device__ __forceinline__ void forward_chain(const Mlp& m, const Tiles& t, int R) {
  for (int l = 0; l < m.n; ++l) {
    dense(t.h[l], t.ld[l], m.dims[l], t.h[l + 1], t.ld[l + 1], m.dims[l + 1], m.wt[l], m.bias[l], R, l + 1 < m.n);
    __syncthreads();
  }
}

// backward chain: dl holds d(pre-norm output) [R][ldg] (= t.db); Linear l's weight / bias partials, then the input
// gradient of Linear l.  Returns the buffer holding d(input) [R][ldg] (need_dx) or nullptr.
__device__ __forceinline__ float* backward_chain(const Mlp& m, const Tiles& t, int R, int rows, float* part, bool first,
                                                 bool need_dx) {
  float* cur = t.db;
  float* nxt = t.da;
  for (int l = m.n - 1; l >= 0; --l) {
    wgrad(t.h[l], t.ld[l], m.dims[l], cur, t.ldg, m.dims[l + 1], rows, part + m.off_w[l], part + m.off_b[l], first);
    if (l > 0 || need_dx) dense_t(cur, t.ldg, m.dims[l + 1], nxt, t.ldg, m.dims[l], m.wt[l], l > 0 ? t.h[l] : nullptr,
                                  t.ld[l], R);
    __syncthreads();
    float* tmp = cur; cur = nxt; nxt = tmp;
  }
  return need_dx ? cur : nullptr;
}

// carve the tiles out of LDS at `p`; returns the first float past them
__device__ __forceinline__ float* carve(const Mlp& m, Tiles& t, float* p, int R, int ld0, int ldh, int n_max) {
  t.h[0] = p;
  t.ld[0] = ld0;
  p += (size_t)R * ld0;
  for (int l = 1; l <= n_max; ++l) {
    t.h[l] = p;
    t.ld[l] = ldh;
    p += (size_t)R * ldh;
  }
  // the last Linear writes h[m.n]: the pre-norm output
  t.da = p;
  p += (size_t)R * ld0;
  t.db = p;
  p += (size_t)R * ld0;
  t.ldg = ld0;
  return p;
}

// ---------------------------------------------------------------------------------------------------------------------------
// row-wise MLP backward.  layout 0: [rows_total, C] row-major; layout 1: [batch, C, rows] channels-first
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) mlp_bwd_kernel(Mlp m, const float* __restrict__ in,
                                                           const float* __restrict__ dout, float* __restrict__ din,
                                                           float* __restrict__ partials, long long rows_total, int rows,
                                                           int in_layout, int out_layout, int R, int ld0, int ldh,
                                                           int lds_partials) {
  extern __shared__ float4 smem4[];
  Tiles t;
  float* lpart = carve(m, t, reinterpret_cast<float*>(smem4), R, ld0, ldh, m.n);
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int cin = m.dims[0], cout = m.dims[m.n];
  float* gpart = partials + (size_t)blockIdx.x * m.n_params;
  float* part = lds_partials ? lpart : gpart;
  const long long n_tiles = (rows_total + R - 1) / R;
  bool first = true;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long row0 = tile * R;
    const int valid = (int)min((long long)R, rows_total - row0);
    for (int idx = threadIdx.x; idx < R * cin; idx += kThreads) {
      int r, k;
      if (in_layout == 1) { r = idx % R; k = idx / R; } else { r = idx / cin; k = idx % cin; }
      const long long row = row0 + r;
      float v = 0.f;
      if (r < valid) {
        if (in_layout == 1) {
          const long long bb = row / rows, p = row % rows;
          v = in[((size_t)bb * cin + k) * rows + p];
        } else {
          v = in[(size_t)row * cin + k];
        }
      }
      t.h[0][r * ld0 + k] = v;
    }
    // upstream gradient -> da (LayerNorm) or db (d pre-norm output directly)
    float* dy = m.g ? t.da : t.db;
    for (int idx = threadIdx.x; idx < R * cout; idx += kThreads) {
      int r, j;
      if (out_layout == 1) { r = idx % R; j = idx / R; } else { r = idx / cout; j = idx % cout; }
      const long long row = row0 + r;
      float v = 0.f;
      if (r < valid) {
        if (out_layout == 1) {
          const long long bb = row / rows, p = row % rows;
          v = dout[((size_t)bb * cout + j) * rows + p];
        } else {
          v = dout[(size_t)row * cout + j];
        }
      }
      dy[r * ld0 + j] = v;
    }
    __syncthreads();
    forward_chain(m, t, R);
    float* z = t.h[m.n];
    if (m.g) {
      for (int r = wave; r < R; r += kWaves) {
        if (r < valid) {
          layernorm_bwd_row(z + r * ldh, t.da + r * ld0, t.db + r * ld0, cout, m.g, m.eps, lane);
        } else {
          for (int k = lane; k < cout; k += kWave) t.db[r * ld0 + k] = 0.f;
        }
      }
      __syncthreads();
      ln_wgrad(z, ldh, t.da, ld0, cout, valid, part + m.off_g, first);
      __syncthreads();
    }
    float* dx = backward_chain(m, t, R, valid, part, first, din != nullptr);
    first = false;
    if (dx) {
      for (int idx = threadIdx.x; idx < R * cin; idx += kThreads) {
        int r, k;
        if (in_layout == 1) { r = idx % R; k = idx / R; } else { r = idx / cin; k = idx % cin; }
        if (r >= valid) continue;
        const long long row = row0 + r;
        const float v = dx[r * ld0 + k];
        if (in_layout == 1) {
          const long long bb = row / rows, p = row % rows;
          din[((size_t)bb * cin + k) * rows + p] = v;
        } else {
          din[(size_t)row * cin + k] = v;
        }
      }
      __syncthreads();
    }
  }
  if (first) zero_partials(m, part);
  if (lds_partials) {
    __syncthreads();
    for (int i = threadIdx.x; i < m.n_params; i += kThreads) gpart[i] = lpart[i];
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// processor-layer backward, pass (a).  Tiles of T = R destination nodes of one sample, edges in chunks of R.
// LDS: the recomputation tiles (ld0 >= 3D) shared by the edge and the node MLP, DY [R][ldh] (d e' of a chunk),
// NG [T][ldh] (node sums, then d agg), NX [T][ldh] (the owner's dx)
// ---------------------------------------------------------------------------------------------------------------------------
struct LayerArgs {
  Mlp em, nm;
  int mean_agg;
  const int* row_ptr;
  const int* src;
  const int* dst;
  int n_nodes, n_edges, batch;
  const float* x_in;
  const float* e_in;
  long long e_in_stride;
  const float* dx_out;
  const float* de_out;         // [B, E, D] or null
  float* dx_in;                // the owner's part; pass (b) adds the source parts
  float* de_in;                // [B, E, D] (the final one, or the per-sample scratch of a shared table)
  float* xsrc;                 // [B, E, D] scratch: the x_src part of each edge's input gradient
  float* partials;             // [gridDim.x][em.n_params + nm.n_params]
  int R, ld0, ldh, n_max;
  int lds_partials;            // accumulate the partial row in LDS (after NX), write it once
};

__global__ void __launch_bounds__(kThreads) layer_bwd_kernel(LayerArgs a) {
  extern __shared__ float4 smem4[];
  const Mlp& em = a.em;
  const Mlp& nm = a.nm;
  const int R = a.R, T = a.R, ld0 = a.ld0, ldh = a.ldh;
  Tiles t;
  float* p = carve(em, t, reinterpret_cast<float*>(smem4), R, ld0, ldh, a.n_max);
  float* DY = p;
  float* NG = DY + (size_t)R * ldh;
  float* NX = NG + (size_t)T * ldh;
  const int D = em.dims[em.n];
  const int D2 = 2 * D, D3 = 3 * D;
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int n_par = em.n_params + nm.n_params;
  float* lpart = NX + (size_t)T * ldh;
  float* gpart = a.partials + (size_t)blockIdx.x * n_par;
  float* part_e = a.lds_partials ? lpart : gpart;
  float* part_n = part_e + em.n_params;
  const int tps = (a.n_nodes + T - 1) / T;
  const int n_tiles = tps * a.batch;
  bool first_e = true, first_n = true;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int bidx = tile / tps;
    const int n0 = (tile % tps) * T, n1 = min(n0 + T, a.n_nodes);
    const int nv = n1 - n0;
    const float* xb = a.x_in + (size_t)bidx * a.n_nodes * D;
    const float* eb = a.e_in + (size_t)bidx * a.e_in_stride;
    const size_t eo = (size_t)bidx * a.n_edges * D;
    const int e_begin = a.row_ptr[n0], e_end = a.row_ptr[n1];
    for (int idx = threadIdx.x; idx < T * D; idx += kThreads) NG[(idx / D) * ldh + idx % D] = 0.f;
    __syncthreads();
    // ---- pass 1: e' of every edge into the tile and the per-node sums (CSC order)
    for (int c0 = e_begin; c0 < e_end; c0 += R) {
      const int rows = min(R, e_end - c0);
      for (int idx = threadIdx.x; idx < R * D3; idx += kThreads) {
        const int r = idx / D3, k = idx % D3;
        float v = 0.f;
        if (r < rows) {
          const int e = c0 + r;
          if (k < D) v = eb[(size_t)e * D + k];
          else if (k < D2) v = xb[(size_t)a.src[e] * D + (k - D)];
          else v = xb[(size_t)a.dst[e] * D + (k - D2)];
        }
        t.h[0][r * ld0 + k] = v;
      }
      __syncthreads();
      forward_chain(em, t, R);
      float* z = t.h[em.n];
      for (int r = wave; r < rows; r += kWaves) {
        float* row = z + r * ldh;
        layernorm_row(row, D, em.g, em.b, em.eps, lane);
        const float* ein = eb + (size_t)(c0 + r) * D;
        for (int k = lane; k < D; k += kWave) row[k] += ein[k];
      }
      __syncthreads();
      for (int idx = threadIdx.x; idx < T * D; idx += kThreads) {
        const int tt = idx / D, k = idx % D;
        const int n = n0 + tt;
        if (n >= n1) continue;
        const int lo = max(a.row_ptr[n] - c0, 0), hi = min(a.row_ptr[n + 1] - c0, rows);
        float s = NG[tt * ldh + k];
        for (int r = lo; r < hi; ++r) s += z[r * ldh + k];
        NG[tt * ldh + k] = s;
      }
      __syncthreads();
    }
    // ---- node block: recompute [agg, x] -> MLP -> LayerNorm, backpropagate dx_out
    for (int idx = threadIdx.x; idx < R * D2; idx += kThreads) {
      const int tt = idx / D2, k = idx % D2;
      const int n = n0 + tt;
      float v = 0.f;
      if (tt < nv) {
        if (k < D) {
          v = NG[tt * ldh + k];
          if (a.mean_agg) {
            const int deg = a.row_ptr[n + 1] - a.row_ptr[n];
            v = deg > 0 ? v / (float)deg : 0.f;
          }
        } else {
          v = xb[(size_t)n * D + (k - D)];
        }
      }
      t.h[0][tt * ld0 + k] = v;
    }
    for (int idx = threadIdx.x; idx < T * D; idx += kThreads) {
      const int tt = idx / D, k = idx % D;
      const float v = tt < nv ? a.dx_out[((size_t)bidx * a.n_nodes + n0 + tt) * D + k] : 0.f;
      t.da[tt * ld0 + k] = v;
      NX[tt * ldh + k] = v;                 // the residual x' = ... + x
    }
    __syncthreads();
    forward_chain(nm, t, R);
    {
      float* z = t.h[nm.n];
      for (int r = wave; r < R; r += kWaves) {
        if (r < nv) {
          layernorm_bwd_row(z + r * ldh, t.da + r * ld0, t.db + r * ld0, D, nm.g, nm.eps, lane);
        } else {
          for (int k = lane; k < D; k += kWave) t.db[r * ld0 + k] = 0.f;
        }
      }
      __syncthreads();
      ln_wgrad(z, ldh, t.da, ld0, D, nv, part_n + nm.off_g, first_n);
      __syncthreads();
      const float* dnode = backward_chain(nm, t, R, nv, part_n, first_n, true);
      first_n = false;
      for (int idx = threadIdx.x; idx < T * D; idx += kThreads) {
        const int tt = idx / D, k = idx % D;
        if (tt >= nv) {
          NG[tt * ldh + k] = 0.f;
          continue;
        }
        float g = dnode[tt * ld0 + k];
        if (a.mean_agg) {
          const int deg = a.row_ptr[n0 + tt + 1] - a.row_ptr[n0 + tt];
          g = deg > 0 ? g / (float)deg : 0.f;
        }
        NG[tt * ldh + k] = g;                                   // d agg (per edge into the node)
        NX[tt * ldh + k] += dnode[tt * ld0 + D + k];            // d x through the node MLP's input
      }
      __syncthreads();
    }
    // ---- pass 2: every edge chunk again, de' = de_out + d agg[dst] through LayerNorm and the edge MLP
    for (int c0 = e_begin; c0 < e_end; c0 += R) {
      const int rows = min(R, e_end - c0);
      for (int idx = threadIdx.x; idx < R * D3; idx += kThreads) {
        const int r = idx / D3, k = idx % D3;
        float v = 0.f;
        if (r < rows) {
          const int e = c0 + r;
          if (k < D) v = eb[(size_t)e * D + k];
          else if (k < D2) v = xb[(size_t)a.src[e] * D + (k - D)];
          else v = xb[(size_t)a.dst[e] * D + (k - D2)];
        }
        t.h[0][r * ld0 + k] = v;
      }
      for (int idx = threadIdx.x; idx < R * D; idx += kThreads) {
        const int r = idx / D, k = idx % D;
        float v = 0.f;
        if (r < rows) {
          const int e = c0 + r;
          v = NG[(a.dst[e] - n0) * ldh + k];
          if (a.de_out) v += a.de_out[eo + (size_t)e * D + k];
        }
        DY[r * ldh + k] = v;
      }
      __syncthreads();
      forward_chain(em, t, R);
      float* z = t.h[em.n];
      for (int r = wave; r < R; r += kWaves) {
        if (r < rows) {
          layernorm_bwd_row(z + r * ldh, DY + r * ldh, t.db + r * ld0, D, em.g, em.eps, lane);
        } else {
          for (int k = lane; k < D; k += kWave) t.db[r * ld0 + k] = 0.f;
        }
      }
      __syncthreads();
      ln_wgrad(z, ldh, DY, ldh, D, rows, part_e + em.off_g, first_e);
      const float* dedge = backward_chain(em, t, R, rows, part_e, first_e, true);
      first_e = false;
      // de_in = de' (residual) + the e part; the x_src part to the scratch
      for (int idx = threadIdx.x; idx < rows * D; idx += kThreads) {
        const int r = idx / D, k = idx % D;
        const size_t o = eo + (size_t)(c0 + r) * D + k;
        a.de_in[o] = DY[r * ldh + k] + dedge[r * ld0 + k];
        a.xsrc[o] = dedge[r * ld0 + D + k];
      }
      // the x_dst part into the owner's nodes, edge order
      for (int idx = threadIdx.x; idx < T * D; idx += kThreads) {
        const int tt = idx / D, k = idx % D;
        const int n = n0 + tt;
        if (n >= n1) continue;
        const int lo = max(a.row_ptr[n] - c0, 0), hi = min(a.row_ptr[n + 1] - c0, rows);
        float s = NX[tt * ldh + k];
        for (int r = lo; r < hi; ++r) s += dedge[r * ld0 + D2 + k];
        NX[tt * ldh + k] = s;
      }
      __syncthreads();
    }
    for (int idx = threadIdx.x; idx < nv * D; idx += kThreads)
      a.dx_in[((size_t)bidx * a.n_nodes + n0) * D + idx] = NX[(idx / D) * ldh + idx % D];
    __syncthreads();
  }
  if (first_e) zero_partials(em, part_e);
  if (first_n) zero_partials(nm, part_n);
  if (a.lds_partials) {
    __syncthreads();
    for (int i = threadIdx.x; i < n_par; i += kThreads) gpart[i] = lpart[i];
  }
}

// pass (b): dx_in[b][n][k] += sum over the edges leaving n (source-sorted order) of xsrc[b][e][k]
__global__ void __launch_bounds__(kThreads) src_gather_kernel(const int* __restrict__ src_row_ptr,
                                                              const int* __restrict__ src_perm,
                                                              const float* __restrict__ xsrc, float* __restrict__ dx_in,
                                                              int n_nodes, int n_edges, int D, int batch) {
  const long long total = (long long)batch * n_nodes * D;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
    const int k = (int)(i % D);
    const long long bn = i / D;
    const int n = (int)(bn % n_nodes), b = (int)(bn / n_nodes);
    const float* xs = xsrc + (size_t)b * n_edges * D + k;
    float s = dx_in[i];
    for (int j = src_row_ptr[n]; j < src_row_ptr[n + 1]; ++j) s += xs[(size_t)src_perm[j] * D];
    dx_in[i] = s;
  }
}

// pass (c): out[p] = sum_{g < parts} in[g * stride + p] for p < n, g order (parameter partials; a shared table's de_in
// over the batch)
__global__ void __launch_bounds__(kThreads) sum_partials_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                long long n, long long stride, int parts) {
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < n; p += (long long)gridDim.x * kThreads) {
    float s = 0.f;
    for (int g = 0; g < parts; ++g) s += in[(size_t)g * stride + p];
    out[p] = s;
  }
}

static int32_t to_mlp(const dlwp_mgn_mlp_desc* d, Mlp& m, int max_in) {
  const int32_t rc = fill_mlp(d, m, max_in, kMaxWidth, "mgn bwd", "backward envelope");
  if (rc) return rc;
  m.eps = d->ln_eps;
  DLWP_REQUIRE((m.g == nullptr) == (m.b == nullptr), DLWP_ERR_INVALID_ARGUMENT, "mgn bwd: LayerNorm needs gamma and beta");
  int off = 0;
  for (int i = 0; i < 5; ++i) {
    m.off_w[i] = m.off_b[i] = 0;
    if (i < m.n) {
      m.off_w[i] = off;
      off += m.dims[i] * m.dims[i + 1];
      m.off_b[i] = off;
      off += m.dims[i + 1];
    }
  }
  m.off_g = off;
  if (m.g) off += 2 * m.dims[m.n];
  m.n_params = off;
  return DLWP_OK;
}

static int hidden_width(const Mlp& m) {
  int w = 0;
  for (int i = 1; i <= m.n; ++i) w = std::max(w, m.dims[i]);
  return w;
}

struct Tile {
  int R, lds_partials;
  size_t lds;
};

// rows per tile (64, 32, 16 or 8) and where the parameter partials live, always two workgroups per CU: the partials in
// LDS beside the largest tile that leaves room for them, else in the global partial row beside the largest tile (inside
// the envelope a row takes at most 4352 bytes, so 16 rows always fit).  One workgroup per CU with the partials in LDS
// was measured slower (D = 48, 410 against 271 ms per training step).
static Tile pick_tile(size_t bytes_per_row, size_t partial_bytes) {
  for (int r = 64; r >= 8; r >>= 1)
    if (r * bytes_per_row + partial_bytes <= kLdsTwoPerCu) return Tile{r, 1, r * bytes_per_row + partial_bytes};
  for (int r = 64; r >= 8; r >>= 1)
    if (r * bytes_per_row <= kLdsTwoPerCu) return Tile{r, 0, r * bytes_per_row};
  return Tile{0, 0, 0};
}

struct MlpPlan {
  int R, ld0, ldh, grid, lds_partials;
  size_t lds;
};

static MlpPlan plan_mlp(const Mlp& m, long long rows_total) {
  MlpPlan p{};
  p.ldh = round4(hidden_width(m));
  p.ld0 = std::max(round4(m.dims[0]), p.ldh);
  const size_t per_row = (3 * (size_t)p.ld0 + (size_t)m.n * p.ldh) * sizeof(float);
  const Tile t = pick_tile(per_row, (size_t)m.n_params * sizeof(float));
  p.R = t.R;
  p.lds = t.lds;
  p.lds_partials = t.lds_partials;
  const long long tiles = p.R ? (rows_total + p.R - 1) / p.R : 0;
  p.grid = (int)std::min<long long>(tiles, kPartials);
  return p;
}

struct LayerPlan {
  int R, ld0, ldh, n_max, grid, lds_partials;
  size_t lds;
};

static LayerPlan plan_layer(const Mlp& em, const Mlp& nm, int n_nodes, int batch) {
  LayerPlan p{};
  const int D = em.dims[em.n];
  p.n_max = std::max(em.n, nm.n);
  p.ldh = round4(D);
  p.ld0 = round4(3 * D);
  const size_t per_row = (3 * (size_t)p.ld0 + (size_t)(p.n_max + 3) * p.ldh) * sizeof(float);
  const Tile t = pick_tile(per_row, (size_t)(em.n_params + nm.n_params) * sizeof(float));
  p.R = t.R;
  p.lds = t.lds;
  p.lds_partials = t.lds_partials;
  const long long tiles = p.R ? (long long)((n_nodes + p.R - 1) / p.R) * batch : 0;
  p.grid = (int)std::min<long long>(tiles, kPartials);
  return p;
}

static int32_t check_layer(const Mlp& em, const Mlp& nm) {
  const int D = em.dims[em.n];
  DLWP_REQUIRE(em.dims[0] == 3 * D && nm.dims[0] == 2 * D && nm.dims[nm.n] == D, DLWP_ERR_INVALID_ARGUMENT,
               "mgn layer bwd: edge MLP %d -> %d, node MLP %d -> %d (want 3D -> D and 2D -> D)", em.dims[0], D, nm.dims[0],
               nm.dims[nm.n]);
  for (int i = 1; i < em.n; ++i)
    DLWP_REQUIRE(em.dims[i] <= D, DLWP_ERR_UNSUPPORTED, "mgn layer bwd: edge hidden %d > %d", em.dims[i], D);
  for (int i = 1; i < nm.n; ++i)
    DLWP_REQUIRE(nm.dims[i] <= D, DLWP_ERR_UNSUPPORTED, "mgn layer bwd: node hidden %d > %d", nm.dims[i], D);
  DLWP_REQUIRE(em.g && nm.g, DLWP_ERR_INVALID_ARGUMENT, "mgn layer bwd: both MLPs end in a LayerNorm");
  return DLWP_OK;
}

static unsigned elementwise_grid(long long n) {
  return (unsigned)std::max<long long>(1, std::min<long long>((n + kThreads - 1) / kThreads, 4096));
}

}  // namespace mgn_bwd
}  // namespace dlwp

using namespace dlwp;

extern "C" size_t dlwp_mgn_mlp_bwd_workspace_bytes(const dlwp_mgn_mlp_desc* mlp, int32_t batch, int32_t rows) {
  mgn_bwd::Mlp m;
  if (batch <= 0 || rows <= 0 || mgn_bwd::to_mlp(mlp, m, mgn_bwd::kMaxMlpIn) != DLWP_OK) return 0;
  const mgn_bwd::MlpPlan p = mgn_bwd::plan_mlp(m, (long long)batch * rows);
  return (size_t)p.grid * m.n_params * sizeof(float);
}

extern "C" int32_t dlwp_mgn_mlp_bwd_f32(const dlwp_mgn_mlp_desc* mlp, const float* in_dev, const float* grad_out_dev,
                                        float* grad_in_dev, float* param_grad_dev, int32_t batch, int32_t rows,
                                        int32_t in_layout, int32_t out_layout, void* workspace, size_t workspace_bytes,
                                        void* stream) {
  mgn_bwd::Mlp m;
  int32_t rc = mgn_bwd::to_mlp(mlp, m, mgn_bwd::kMaxMlpIn);
  if (rc) return rc;
  DLWP_REQUIRE(in_dev && grad_out_dev && param_grad_dev && workspace, DLWP_ERR_INVALID_ARGUMENT, "mgn mlp bwd: null tensor");
  DLWP_REQUIRE(batch > 0 && rows > 0, DLWP_ERR_INVALID_ARGUMENT, "mgn mlp bwd: batch %d rows %d", batch, rows);
  DLWP_REQUIRE((in_layout == 0 || in_layout == 1) && (out_layout == 0 || out_layout == 1), DLWP_ERR_INVALID_ARGUMENT,
               "mgn mlp bwd: layout %d / %d", in_layout, out_layout);
  DLWP_REQUIRE(grad_in_dev != in_dev && grad_in_dev != grad_out_dev, DLWP_ERR_INVALID_ARGUMENT,
               "mgn mlp bwd: grad_in aliases an input");
  const size_t need = dlwp_mgn_mlp_bwd_workspace_bytes(mlp, batch, rows);
  DLWP_REQUIRE(workspace_bytes >= need, DLWP_ERR_WORKSPACE, "mgn mlp bwd: workspace of %zu bytes, %zu needed",
               workspace_bytes, need);
  const long long total = (long long)batch * rows;
  const mgn_bwd::MlpPlan p = mgn_bwd::plan_mlp(m, total);
  DLWP_REQUIRE(p.R > 0, DLWP_ERR_UNSUPPORTED, "mgn mlp bwd: no row tile fits LDS");
  rc = mgn_bwd::set_lds(mgn_bwd::mlp_bwd_kernel, p.lds);
  if (rc) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(mgn_bwd::mlp_bwd_kernel, dim3((unsigned)p.grid), dim3(mgn_bwd::kThreads), p.lds, s, m, in_dev,
                     grad_out_dev, grad_in_dev, part, total, rows, in_layout, out_layout, p.R, p.ld0, p.ldh,
                     p.lds_partials);
  DLWP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(mgn_bwd::sum_partials_kernel, dim3(mgn_bwd::elementwise_grid(m.n_params)), dim3(mgn_bwd::kThreads), 0,
                     s, part, param_grad_dev, (long long)m.n_params, (long long)m.n_params, p.grid);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" size_t dlwp_mgn_processor_layer_bwd_workspace_bytes(const dlwp_mgn_mlp_desc* edge_mlp,
                                                               const dlwp_mgn_mlp_desc* node_mlp, int32_t n_nodes,
                                                               int32_t n_edges, int32_t batch, int32_t e_shared) {
  mgn_bwd::Mlp em, nm;
  if (n_nodes <= 0 || n_edges < 0 || batch <= 0) return 0;
  if (mgn_bwd::to_mlp(edge_mlp, em, 3 * mgn_bwd::kMaxWidth) || mgn_bwd::to_mlp(node_mlp, nm, 2 * mgn_bwd::kMaxWidth))
    return 0;
  if (mgn_bwd::check_layer(em, nm)) return 0;
  const mgn_bwd::LayerPlan p = mgn_bwd::plan_layer(em, nm, n_nodes, batch);
  const size_t bed = (size_t)batch * n_edges * em.dims[em.n];
  return ((size_t)p.grid * (em.n_params + nm.n_params) + bed * (e_shared ? 2 : 1)) * sizeof(float);
}

extern "C" int32_t dlwp_mgn_processor_layer_bwd_f32(
    const dlwp_mgn_mlp_desc* edge_mlp, const dlwp_mgn_mlp_desc* node_mlp, int32_t aggregation, const int32_t* row_ptr_dev,
    const int32_t* src_dev, const int32_t* dst_dev, const int32_t* src_row_ptr_dev, const int32_t* src_perm_dev,
    int32_t n_nodes, int32_t n_edges, int32_t batch, const float* x_in_dev, const float* e_in_dev, int64_t e_in_batch_stride,
    const float* dx_out_dev, const float* de_out_dev, float* dx_in_dev, float* de_in_dev, float* edge_grad_dev,
    float* node_grad_dev, void* workspace, size_t workspace_bytes, void* stream) {
  mgn_bwd::Mlp em, nm;
  int32_t rc = mgn_bwd::to_mlp(edge_mlp, em, 3 * mgn_bwd::kMaxWidth);
  if (rc) return rc;
  rc = mgn_bwd::to_mlp(node_mlp, nm, 2 * mgn_bwd::kMaxWidth);
  if (rc) return rc;
  rc = mgn_bwd::check_layer(em, nm);
  if (rc) return rc;
  const int D = em.dims[em.n];
  DLWP_REQUIRE(aggregation == 0 || aggregation == 1, DLWP_ERR_UNSUPPORTED, "mgn layer bwd: aggregation %d", aggregation);
  DLWP_REQUIRE(row_ptr_dev && src_dev && dst_dev && src_row_ptr_dev && src_perm_dev && x_in_dev && e_in_dev && dx_out_dev &&
                   dx_in_dev && de_in_dev && edge_grad_dev && node_grad_dev && workspace,
               DLWP_ERR_INVALID_ARGUMENT, "mgn layer bwd: null tensor");
  DLWP_REQUIRE(n_nodes > 0 && n_edges >= 0 && batch > 0, DLWP_ERR_INVALID_ARGUMENT, "mgn layer bwd: nodes %d edges %d batch %d",
               n_nodes, n_edges, batch);
  DLWP_REQUIRE(e_in_batch_stride == 0 || e_in_batch_stride == (int64_t)n_edges * D, DLWP_ERR_INVALID_ARGUMENT,
               "mgn layer bwd: edge batch stride %lld (0 or n_edges * D)", (long long)e_in_batch_stride);
  DLWP_REQUIRE(dx_in_dev != x_in_dev && dx_in_dev != dx_out_dev && de_in_dev != e_in_dev && de_in_dev != de_out_dev,
               DLWP_ERR_INVALID_ARGUMENT, "mgn layer bwd: an output aliases an input");
  const bool shared = e_in_batch_stride == 0;
  const size_t need = dlwp_mgn_processor_layer_bwd_workspace_bytes(edge_mlp, node_mlp, n_nodes, n_edges, batch, shared);
  DLWP_REQUIRE(workspace_bytes >= need, DLWP_ERR_WORKSPACE, "mgn layer bwd: workspace of %zu bytes, %zu needed",
               workspace_bytes, need);
  const mgn_bwd::LayerPlan p = mgn_bwd::plan_layer(em, nm, n_nodes, batch);
  DLWP_REQUIRE(p.R > 0, DLWP_ERR_UNSUPPORTED, "mgn layer bwd: no tile fits LDS");
  rc = mgn_bwd::set_lds(mgn_bwd::layer_bwd_kernel, p.lds);
  if (rc) return rc;
  const long long n_par = (long long)em.n_params + nm.n_params;
  const size_t bed = (size_t)batch * n_edges * D;
  float* part = static_cast<float*>(workspace);
  float* xsrc = part + (size_t)p.grid * n_par;
  float* de_scratch = xsrc + bed;
  mgn_bwd::LayerArgs a;
  a.em = em;
  a.nm = nm;
  a.mean_agg = aggregation;
  a.row_ptr = row_ptr_dev;
  a.src = src_dev;
  a.dst = dst_dev;
  a.n_nodes = n_nodes;
  a.n_edges = n_edges;
  a.batch = batch;
  a.x_in = x_in_dev;
  a.e_in = e_in_dev;
  a.e_in_stride = (long long)e_in_batch_stride;
  a.dx_out = dx_out_dev;
  a.de_out = de_out_dev;
  a.dx_in = dx_in_dev;
  a.de_in = shared ? de_scratch : de_in_dev;
  a.xsrc = xsrc;
  a.partials = part;
  a.R = p.R;
  a.ld0 = p.ld0;
  a.ldh = p.ldh;
  a.n_max = p.n_max;
  a.lds_partials = p.lds_partials;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mgn_bwd::layer_bwd_kernel, dim3((unsigned)p.grid), dim3(mgn_bwd::kThreads), p.lds, s, a);
  DLWP_HIP_CHECK(hipGetLastError());
  const long long nd = (long long)batch * n_nodes * D;
  hipLaunchKernelGGL(mgn_bwd::src_gather_kernel, dim3(mgn_bwd::elementwise_grid(nd)), dim3(mgn_bwd::kThreads), 0, s,
                     src_row_ptr_dev, src_perm_dev, xsrc, dx_in_dev, n_nodes, n_edges, D, batch);
  DLWP_HIP_CHECK(hipGetLastError());
  // parameter partials: rows of [edge params | node params], one launch per MLP
  hipLaunchKernelGGL(mgn_bwd::sum_partials_kernel, dim3(mgn_bwd::elementwise_grid(em.n_params)), dim3(mgn_bwd::kThreads), 0,
                     s, part, edge_grad_dev, (long long)em.n_params, n_par, p.grid);
  DLWP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(mgn_bwd::sum_partials_kernel, dim3(mgn_bwd::elementwise_grid(nm.n_params)), dim3(mgn_bwd::kThreads), 0,
                     s, part + em.n_params, node_grad_dev, (long long)nm.n_params, n_par, p.grid);
  DLWP_HIP_CHECK(hipGetLastError());
  if (shared && n_edges > 0) {
    const long long ed = (long long)n_edges * D;
    hipLaunchKernelGGL(mgn_bwd::sum_partials_kernel, dim3(mgn_bwd::elementwise_grid(ed)), dim3(mgn_bwd::kThreads), 0, s,
                       de_scratch, de_in_dev, ed, ed, batch);
    DLWP_HIP_CHECK(hipGetLastError());
  }
  return DLWP_OK;
}
