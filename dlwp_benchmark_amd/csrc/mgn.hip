// MeshGraphNet message passing on MI355X (gfx950).
//
// Replaces the per-step arithmetic of the reference MeshGraphNet (models/mgn/meshgraphnet.py:412-423) and the layers it is
// built from (models/graphcast/gnn_layers/mesh_graph_mlp.py MeshGraphMLP / MeshGraphEdgeMLPConcat, mesh_edge_block.py,
// mesh_node_block.py, utils.py concat_message_function :96-111 and agg_concat_dgl :340-380):
//
//   dlwp_mgn_mlp_f32               one MeshGraphMLP row by row: Linear -> ReLU -> ... -> Linear [-> LayerNorm].  Rows are
//                                  read row-major or channels-first [B, C, rows] (the node encoder reads x_t as the rollout
//                                  assembles it) and written either way (the decoder writes [B, C, H, W]).
//   dlwp_mgn_processor_layer_f32   one MeshEdgeBlock + MeshNodeBlock pair in ONE launch.  A workgroup owns T consecutive
//                                  destination nodes of one sample and therefore every edge into them (edges are stored in
//                                  CSC order, sorted by destination).  Per chunk of R edges: gather [e, x_src, x_dst] into
//                                  LDS, the edge MLP, LayerNorm, + e, store e' (its only reader is the same owner in the next
//                                  layer, so it may overwrite e), and add e' into the owner's per-node sums in edge order.
//                                  Then per node: [agg, x] (utils.py:379 order), the node MLP, LayerNorm, + x into the other
//                                  half of a ping-pong node buffer.
//
// Every output element has exactly one writer and every sum runs in a fixed order: no atomics, bitwise reproducible, and a
// sample's result does not depend on its batch neighbours.  Products are fp32 FMA chains in k order (exact fp32, no
// reduced-precision operand).  Linear weights arrive TRANSPOSED, [in][out], so that neighbouring lanes (neighbouring output
// columns) load neighbouring words.  Two product forms, chosen per launch from the widths:
//   matrix (any width >= 64): v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation).  A wave owns a 16-column
//     slice of the output and every 16-row tile of the LDS activations; per 4-deep k step each lane loads ONE weight (the
//     B operand, a 16 x 4 panel per wave, shared by all row tiles) and one activation per row tile from LDS.  Tiles are
//     R = 16..64 rows; LDS row strides are padded off multiples of 32 words so the 16 rows of an A operand hit distinct
//     banks.
//   scalar (narrow layers, the yaml config's 32 / 34): fp32 FMA chains in k order; each lane keeps four rows'
//     accumulators, so one weight load feeds four FMAs and one 16-byte LDS read feeds four more.
// LDS holds the activations of one tile only; weights stream through the caches.
//
// kThreads, kWave, round4, dense, layernorm_row, the base of Mlp, fill_mlp and set_lds are mgn_common.hpp's, shared with
// mgn_bwd.hip.
#include "mgn_common.hpp"

namespace dlwp {
namespace mgn {

constexpr int kMaxWidth = 512;        // hidden and output widths
constexpr int kMaxInWidth = 2048;     // input width of dlwp_mgn_mlp_f32
constexpr size_t kLdsBudget = 64 * 1024;
constexpr size_t kLdsMax = 150 * 1024;

struct Mlp : MlpBase {
  float eps;
};

// the same product on the matrix pipe; RT = R / 16 row tiles.  Lane l supplies A[i = l & 15][k = l >> 4] and
// B[k = l >> 4][j = l & 15] and holds D[4 (l >> 4) + r][l & 15] (common.hpp mfma16x16x4).
template <int RT>
__device__ __forceinline__ void dense_mfma(const float* in, int ldi, int n_in, float* out, int ldo, int n_out,
                                           const float* __restrict__ wt, const float* __restrict__ bias, bool relu) {
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int li = lane & 15, lk = lane >> 4;
  const int ctiles = (n_out + 15) >> 4;
  const int kmain = n_in & ~3;
  for (int ct = wave; ct < ctiles; ct += kThreads / kWave) {
    const int j = ct * 16 + li;
    const bool jok = j < n_out;
    const float bj = jok ? bias[j] : 0.f;
    f32x4 acc[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) acc[r] = f32x4{bj, bj, bj, bj};
    const float* wcol = wt + (jok ? j : 0) + (size_t)lk * n_out;
    const float* arow = in + li * ldi + lk;
    int k = 0;
#pragma unroll 4
    for (; k < kmain; k += 4) {
      const float b = jok ? wcol[(size_t)k * n_out] : 0.f;
#pragma unroll
      for (int r = 0; r < RT; ++r) acc[r] = mfma16x16x4(arow[r * 16 * ldi + k], b, acc[r]);
    }
    if (k < n_in) {                 // k tail: lanes past n_in supply zeros to both operands
      const bool kok = k + lk < n_in;
      const float b = (jok && kok) ? wcol[(size_t)k * n_out] : 0.f;
#pragma unroll
      for (int r = 0; r < RT; ++r) acc[r] = mfma16x16x4(kok ? arow[r * 16 * ldi + k] : 0.f, b, acc[r]);
    }
    if (jok) {
#pragma unroll
      for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float v = acc[r][i];
          out[(r * 16 + 4 * lk + i) * ldo + j] = relu ? fmaxf(v, 0.f) : v;
        }
    }
  }
}

// the Linear chain of one MLP, ping-ponging between two LDS tiles; returns the tile holding the result and its stride.
// mfma: the matrix form (R % 16 == 0)
__device__ __forceinline__ float* chain(const Mlp& m, float* a, int lda, float* b, int ldb, int R, bool mfma, int& ld_res) {
  for (int l = 0; l < m.n; ++l) {
    const bool relu = l + 1 < m.n;
    if (!mfma)
      dense(a, lda, m.dims[l], b, ldb, m.dims[l + 1], m.wt[l], m.bias[l], R, relu);
    else if (R == 16)
      dense_mfma<1>(a, lda, m.dims[l], b, ldb, m.dims[l + 1], m.wt[l], m.bias[l], relu);
    else if (R == 32)
      dense_mfma<2>(a, lda, m.dims[l], b, ldb, m.dims[l + 1], m.wt[l], m.bias[l], relu);
    else
      dense_mfma<4>(a, lda, m.dims[l], b, ldb, m.dims[l + 1], m.wt[l], m.bias[l], relu);
    __syncthreads();
    float* t = a; a = b; b = t;
    const int tl = lda; lda = ldb; ldb = tl;
  }
  ld_res = lda;
  return a;
}

// ---------------------------------------------------------------------------------------------------------------------------
// row-wise MLP.  layout 0: [rows_total, C] row-major; layout 1: [batch, C, rows] channels-first (row = b * rows + p)
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) mlp_kernel(Mlp m, const float* __restrict__ in, float* __restrict__ out,
                                                       long long rows_total, int rows, int in_layout, int out_layout, int R,
                                                       int ld, int mfma) {
  extern __shared__ float4 smem4[];
  float* A = reinterpret_cast<float*>(smem4);
  float* B = A + (size_t)R * ld;
  const long long row0 = (long long)blockIdx.x * R;
  const int cin = m.dims[0], cout = m.dims[m.n];
  for (int idx = threadIdx.x; idx < R * cin; idx += kThreads) {
    int r, k;
    if (in_layout == 1) { r = idx % R; k = idx / R; } else { r = idx / cin; k = idx % cin; }
    const long long row = row0 + r;
    float v = 0.f;
    if (row < rows_total) {
      if (in_layout == 1) {
        const long long bb = row / rows, p = row % rows;
        v = in[((size_t)bb * cin + k) * rows + p];
      } else {
        v = in[(size_t)row * cin + k];
      }
    }
    A[r * ld + k] = v;
  }
  __syncthreads();
  int ldr;
  float* res = chain(m, A, ld, B, ld, R, mfma != 0, ldr);
  if (m.g) {
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    for (int r = wave; r < R; r += kThreads / kWave) layernorm_row(res + r * ldr, cout, m.g, m.b, m.eps, lane);
    __syncthreads();
  }
  for (int idx = threadIdx.x; idx < R * cout; idx += kThreads) {
    int r, j;
    if (out_layout == 1) { r = idx % R; j = idx / R; } else { r = idx / cout; j = idx % cout; }
    const long long row = row0 + r;
    if (row >= rows_total) continue;
    const float v = res[r * ldr + j];
    if (out_layout == 1) {
      const long long bb = row / rows, p = row % rows;
      out[((size_t)bb * cout + j) * rows + p] = v;
    } else {
      out[(size_t)row * cout + j] = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// one processor layer (edge block + node block).  grid (ceil(N / T), batch); T <= R destination nodes per workgroup,
// edges in chunks of R.  LDS: A [R][lda >= 3D] (concat / ping), B [R][ldb >= D] (pong), G [T][ldb] (per-node sums)
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) layer_kernel(Mlp em, Mlp nm, int mean_agg, const int* __restrict__ row_ptr,
                                                         const int* __restrict__ src, const int* __restrict__ dst,
                                                         int n_nodes, int n_edges,
                                                         const float* __restrict__ x_in, float* __restrict__ x_out,
                                                         const float* e_in, long long e_in_stride, float* e_out, int R,
                                                         int T, int lda, int ldb, int mfma) {
  extern __shared__ float4 smem4[];
  float* A = reinterpret_cast<float*>(smem4);
  float* B = A + (size_t)R * lda;
  float* G = B + (size_t)R * ldb;
  const int D = em.dims[em.n];
  const int bidx = blockIdx.y;
  const int n0 = blockIdx.x * T, n1 = min(n0 + T, n_nodes);
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const float* xb = x_in + (size_t)bidx * n_nodes * D;
  const float* eb = e_in + (size_t)bidx * e_in_stride;
  float* eo = e_out + (size_t)bidx * n_edges * D;
  for (int idx = threadIdx.x; idx < T * D; idx += kThreads) G[(idx / D) * ldb + idx % D] = 0.f;
  __syncthreads();
  const int e_begin = row_ptr[n0], e_end = row_ptr[n1];
  const int D3 = 3 * D;
  for (int c0 = e_begin; c0 < e_end; c0 += R) {
    const int rows = min(R, e_end - c0);
    // gather [e, x[src], x[dst]] (concat_message_function order)
    for (int idx = threadIdx.x; idx < R * D3; idx += kThreads) {
      const int r = idx / D3, k = idx % D3;
      float v = 0.f;
      if (r < rows) {
        const int e = c0 + r;
        if (k < D) {
          v = eb[(size_t)e * D + k];
        } else if (k < 2 * D) {
          v = xb[(size_t)src[e] * D + (k - D)];
        } else {
          v = xb[(size_t)dst[e] * D + (k - 2 * D)];
        }
      }
      A[r * lda + k] = v;
    }
    __syncthreads();
    int ldr;
    float* res = chain(em, A, lda, B, ldb, R, mfma != 0, ldr);
    // LayerNorm + residual (mesh_edge_block.py: efeat_new + efeat); e is re-read: this workgroup has not stored it yet
    for (int r = wave; r < rows; r += kThreads / kWave) {
      float* row = res + r * ldr;
      layernorm_row(row, D, em.g, em.b, em.eps, lane);
      const float* ein = eb + (size_t)(c0 + r) * D;
      float* eout = eo + (size_t)(c0 + r) * D;
      for (int k = lane; k < D; k += kWave) {
        const float v = row[k] + ein[k];
        row[k] = v;
        eout[k] = v;
      }
    }
    __syncthreads();
    // per-node sums in edge order: lane pair (node t, channel k) walks the chunk's edges into t
    for (int idx = threadIdx.x; idx < T * D; idx += kThreads) {
      const int t = idx / D, k = idx % D;
      const int n = n0 + t;
      if (n >= n1) continue;
      const int lo = max(row_ptr[n] - c0, 0), hi = min(row_ptr[n + 1] - c0, rows);
      float s = G[t * ldb + k];
      for (int r = lo; r < hi; ++r) s += res[r * ldr + k];
      G[t * ldb + k] = s;
    }
    __syncthreads();
  }
  // node block: [agg, x] -> MLP -> LayerNorm -> + x
  const int D2 = 2 * D;
  for (int idx = threadIdx.x; idx < R * D2; idx += kThreads) {     // rows T..R-1 of the node tile stay zero
    const int t = idx / D2, k = idx % D2;
    const int n = n0 + t;
    float v = 0.f;
    if (t < T && n < n1) {
      if (k < D) {
        v = G[t * ldb + k];
        if (mean_agg) {
          const int deg = row_ptr[n + 1] - row_ptr[n];
          v = deg > 0 ? v / (float)deg : 0.f;
        }
      } else {
        v = xb[(size_t)n * D + (k - D)];
      }
    }
    A[t * lda + k] = v;
  }
  __syncthreads();
  int ldr;
  float* res = chain(nm, A, lda, B, ldb, R, mfma != 0, ldr);
  for (int t = wave; t < n1 - n0; t += kThreads / kWave) {
    float* row = res + t * ldr;
    layernorm_row(row, D, nm.g, nm.b, nm.eps, lane);
    const float* xin = xb + (size_t)(n0 + t) * D;
    float* xo = x_out + ((size_t)bidx * n_nodes + n0 + t) * D;
    for (int k = lane; k < D; k += kWave) xo[k] = row[k] + xin[k];
  }
}

static int32_t to_mlp(const dlwp_mgn_mlp_desc* d, Mlp& m, int max_in) {
  const int32_t rc = fill_mlp(d, m, max_in, kMaxWidth, "mgn", "envelope");
  if (rc) return rc;
  m.eps = d->ln_eps;
  DLWP_REQUIRE((m.g == nullptr) == (m.b == nullptr), DLWP_ERR_INVALID_ARGUMENT, "mgn: LayerNorm needs both gamma and beta");
  return DLWP_OK;
}

static int max_dim(const Mlp& m) {
  int w = 0;
  for (int i = 0; i <= m.n; ++i) w = std::max(w, m.dims[i]);
  return w;
}

// scalar form: the largest tile of rows in {64, 32, 16, 8} whose LDS fits the budget; 8 up to kLdsMax, else 4 (only
// dlwp_mgn_mlp_f32 with inputs over ~1200 wide gets there)
static int pick_rows(size_t bytes_per_row) {
  for (int r = 64; r >= 8; r >>= 1)
    if (r * bytes_per_row <= kLdsBudget) return r;
  if (8 * bytes_per_row <= kLdsMax) return 8;
  return 4;
}

// matrix form: tiles of 64, 32 or 16 rows (0: even 16 rows exceed kLdsMax)
static int pick_rows_mfma(size_t bytes_per_row) {
  for (int r = 64; r >= 16; r >>= 1)
    if (r * bytes_per_row <= kLdsBudget) return r;
  return 16 * bytes_per_row <= kLdsMax ? 16 : 0;
}

// LDS row stride: whole float4s; for the matrix form off multiples of 32 words, so that the 16 rows one A operand reads
// fall in distinct banks
static int pad_ld(int x, bool mfma) {
  int ld = round4(x);
  if (mfma && ld % 32 == 0) ld += 4;
  return ld;
}

constexpr int kMfmaMinWidth = 64;     // narrower layers keep the scalar form (16-column tiles would idle too many lanes)

}  // namespace mgn
}  // namespace dlwp

using namespace dlwp;

extern "C" int32_t dlwp_mgn_mlp_f32(const dlwp_mgn_mlp_desc* mlp, const float* in_dev, float* out_dev, int32_t batch,
                                    int32_t rows, int32_t in_layout, int32_t out_layout, void* stream) {
  mgn::Mlp m;
  int32_t rc = mgn::to_mlp(mlp, m, mgn::kMaxInWidth);
  if (rc) return rc;
  DLWP_REQUIRE(in_dev && out_dev, DLWP_ERR_INVALID_ARGUMENT, "mgn mlp: null tensor");
  DLWP_REQUIRE(batch > 0 && rows > 0, DLWP_ERR_INVALID_ARGUMENT, "mgn mlp: batch %d rows %d", batch, rows);
  DLWP_REQUIRE((in_layout == 0 || in_layout == 1) && (out_layout == 0 || out_layout == 1), DLWP_ERR_INVALID_ARGUMENT,
               "mgn mlp: layout %d / %d", in_layout, out_layout);
  int widest_out = 0;
  for (int i = 1; i <= m.n; ++i) widest_out = std::max(widest_out, m.dims[i]);
  bool mfma = widest_out >= mgn::kMfmaMinWidth;
  int ld = mgn::pad_ld(mgn::max_dim(m), mfma);
  int R = mfma ? mgn::pick_rows_mfma(2 * (size_t)ld * sizeof(float)) : 0;
  if (R == 0) {                       // scalar form
    mfma = false;
    ld = mgn::pad_ld(mgn::max_dim(m), false);
    R = mgn::pick_rows(2 * (size_t)ld * sizeof(float));
  }
  const size_t lds = 2 * (size_t)R * ld * sizeof(float);
  DLWP_REQUIRE(lds <= mgn::kLdsMax, DLWP_ERR_UNSUPPORTED, "mgn mlp: %zu bytes of LDS", lds);
  rc = mgn::set_lds(mgn::mlp_kernel, lds);
  if (rc) return rc;
  const long long total = (long long)batch * rows;
  const long long blocks = (total + R - 1) / R;
  DLWP_REQUIRE(blocks <= INT32_MAX, DLWP_ERR_UNSUPPORTED, "mgn mlp: %lld rows", total);
  hipLaunchKernelGGL(mgn::mlp_kernel, dim3((unsigned)blocks), dim3(mgn::kThreads), lds,
                     reinterpret_cast<hipStream_t>(stream), m, in_dev, out_dev, total, rows, in_layout, out_layout, R, ld,
                     (int)mfma);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" int32_t dlwp_mgn_processor_layer_f32(const dlwp_mgn_mlp_desc* edge_mlp, const dlwp_mgn_mlp_desc* node_mlp,
                                                int32_t aggregation, const int32_t* row_ptr_dev, const int32_t* src_dev,
                                                const int32_t* dst_dev, int32_t n_nodes, int32_t n_edges, int32_t batch, const float* x_in_dev,
                                                float* x_out_dev, const float* e_in_dev, int64_t e_in_batch_stride,
                                                float* e_out_dev, void* stream) {
  mgn::Mlp em, nm;
  int32_t rc = mgn::to_mlp(edge_mlp, em, mgn::kMaxWidth * 3);
  if (rc) return rc;
  rc = mgn::to_mlp(node_mlp, nm, mgn::kMaxWidth * 2);
  if (rc) return rc;
  const int D = em.dims[em.n];
  DLWP_REQUIRE(em.dims[0] == 3 * D && nm.dims[0] == 2 * D && nm.dims[nm.n] == D, DLWP_ERR_INVALID_ARGUMENT,
               "mgn layer: edge MLP %d -> %d, node MLP %d -> %d (want 3D -> D and 2D -> D)", em.dims[0], D, nm.dims[0],
               nm.dims[nm.n]);
  for (int i = 1; i < em.n; ++i) DLWP_REQUIRE(em.dims[i] <= D, DLWP_ERR_UNSUPPORTED, "mgn layer: edge hidden %d > %d", em.dims[i], D);
  for (int i = 1; i < nm.n; ++i) DLWP_REQUIRE(nm.dims[i] <= D, DLWP_ERR_UNSUPPORTED, "mgn layer: node hidden %d > %d", nm.dims[i], D);
  DLWP_REQUIRE(em.g && nm.g, DLWP_ERR_INVALID_ARGUMENT, "mgn layer: both MLPs end in a LayerNorm");
  DLWP_REQUIRE(aggregation == 0 || aggregation == 1, DLWP_ERR_UNSUPPORTED, "mgn layer: aggregation %d", aggregation);
  DLWP_REQUIRE(row_ptr_dev && src_dev && dst_dev && x_in_dev && x_out_dev && e_in_dev && e_out_dev, DLWP_ERR_INVALID_ARGUMENT,
               "mgn layer: null tensor");
  DLWP_REQUIRE(n_nodes > 0 && n_edges >= 0 && batch > 0 && batch <= 65535, DLWP_ERR_INVALID_ARGUMENT,
               "mgn layer: nodes %d edges %d batch %d", n_nodes, n_edges, batch);
  DLWP_REQUIRE(x_in_dev != x_out_dev, DLWP_ERR_INVALID_ARGUMENT, "mgn layer: x_out may not alias x_in");
  DLWP_REQUIRE(e_in_batch_stride != 0 || e_in_dev != e_out_dev, DLWP_ERR_INVALID_ARGUMENT,
               "mgn layer: e_out may not alias an edge table shared by the batch (stride 0)");
  DLWP_REQUIRE(e_in_batch_stride == 0 || e_in_batch_stride == (int64_t)n_edges * D, DLWP_ERR_INVALID_ARGUMENT,
               "mgn layer: edge batch stride %lld (0 or n_edges * D)", (long long)e_in_batch_stride);
  const bool mfma = D >= mgn::kMfmaMinWidth;
  const int lda = mgn::pad_ld(3 * D, mfma), ldb = mgn::pad_ld(D, mfma);
  int R, T;
  if (mfma) {
    R = T = mgn::pick_rows_mfma((size_t)(lda + 2 * ldb) * sizeof(float));
    if (R == 0) {                     // 16-edge chunks, 8 destination nodes (rows 8..15 of the node tile are zero)
      R = 16;
      T = (size_t)16 * (lda + 2 * ldb) * sizeof(float) <= mgn::kLdsMax ? 16 : 8;
    }
  } else {
    R = T = mgn::pick_rows((size_t)(lda + 2 * ldb) * sizeof(float));
  }
  const size_t lds = ((size_t)R * (lda + ldb) + (size_t)T * ldb) * sizeof(float);
  DLWP_REQUIRE(lds <= mgn::kLdsMax, DLWP_ERR_UNSUPPORTED, "mgn layer: %zu bytes of LDS", lds);
  rc = mgn::set_lds(mgn::layer_kernel, lds);
  if (rc) return rc;
  const unsigned gx = (unsigned)((n_nodes + T - 1) / T);
  hipLaunchKernelGGL(mgn::layer_kernel, dim3(gx, (unsigned)batch), dim3(mgn::kThreads), lds,
                     reinterpret_cast<hipStream_t>(stream), em, nm, aggregation, row_ptr_dev, src_dev, dst_dev, n_nodes,
                     n_edges, x_in_dev, x_out_dev, e_in_dev, (long long)e_in_batch_stride, e_out_dev, R, T, lda, ldb,
                     (int)mfma);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}
