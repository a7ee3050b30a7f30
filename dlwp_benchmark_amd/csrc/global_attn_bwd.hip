// Backward of the diffusion U-Net's global attention (global_attn.hip) on MI355X (gfx950).
//
// Forward (reference modern_unet.py:565-571): s_ij = scale q_i . k_j, softmax over the QUERY axis i,
//   P_ij = exp(s_ij - L_j),  L_j = m_j + ln sum_i exp(s_ij - m_j),  O_i = sum_j P_ij v_j.
// Gradient, with dO the gradient of O:
//   dV_j = sum_i P_ij dO_i            dP_ij = dO_i . v_j
//   D_j  = sum_i P_ij dP_ij = v_j . dV_j   (a per-KEY delta: the mirror image of flash attention's per-query dO_i . O_i)
//   dS_ij = P_ij (dP_ij - D_j)        dK_j = scale sum_i dS_ij q_i        dQ_i = scale sum_j dS_ij k_j
// The statistics are the forward's workspace as it stands, L2_j = L_j log2(e), so P = exp2(s log2(e) scale - L2_j) is
// recomputed tile by tile and nothing of size N x N is ever written.  Three launches of one kernel template, each a wave per
// 16 "own" rows of one (sample, head) and one slice of <= 128 output columns, sweeping every 16-row tile of the "other" rows:
//   kDV  own = keys j,    other = queries i:  S tile, P, dV^T += dO^T P
//   kDK  own = keys j,    other = queries i:  D_j = v_j . dV_j (from kDV's output) into the workspace, S and dP tiles,
//                                             dS = P (dP - D_j), dK^T += Q^T dS
//   kDQ  own = queries i, other = keys j:     S^T and dP^T tiles, dS^T = P^T (dP^T - D_j), dQ^T += K^T dS^T
// The layout of every launch is the forward's pass 2 (output_kernel): the score-like tiles come out of
// v_mfma_f32_16x16x4_f32 with the other index on the accumulator rows (four per lane group) and the own index on the lane
// column, so they are consumed as the B operand of the accumulating product straight from the registers; the A operand
// (dO, Q or K rows of the other tile) is fetched with scalar loads.  The wave's own operands (<= 128 wide) stay in
// registers; wider heads reload them per chunk and split the output columns into slices, each recomputing S and dP over
// the full d.  Tails: other rows >= N get P = 0, own rows >= N are not written, d is zero-padded to the chunk of 16.
// Row bases are 64-bit.  No atomics and every output element has one writer: results are bitwise reproducible and a
// sample's gradients do not depend on its batch neighbours.  dqkv is written in the forward's input layout
// [Bt, N, heads, {q, k, v}, d], so the projection Linear's backward consumes it as it stands.
#include "global_attn_common.hpp"

namespace dlwp {
namespace gattn_bwd {

using namespace gattn;   // global_attn_common.hpp: kWaves, kRegChunks, load4, mfma4

constexpr int kMaxHeadDim = 1024;

enum Mode { kDV = 0, kDK = 1, kDQ = 2 };

// grid (ceil(tiles / 4), batch * heads, slices), block 256.  qkv [b][n][heads][3][d], go (grad of the output) [b][n][heads d],
// lse2 / dws [bh][n], dqkv like qkv.
template <int MODE, int NT, bool VEC, bool REG>
__global__ __launch_bounds__(256) void bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ go,
                                                  const float* __restrict__ lse2, float* __restrict__ dws,
                                                  float* __restrict__ dqkv, int n, int heads, int d, float c2, float scale,
                                                  int tiles) {
  constexpr bool KM = MODE != kDQ;      // key-major: the own rows are keys, the softmax axis runs over the other rows
  constexpr bool DP = MODE != kDV;      // dS = P (dP - D) rather than P
  const int lane = threadIdx.x & 63, col = lane & 15, g = lane >> 4;
  const int ob = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (ob >= tiles) return;
  const long long bh = blockIdx.y, b = bh / heads;
  const int h = (int)(bh % heads);
  const int dv0 = blockIdx.z * NT * 16;
  const long long ts = (long long)heads * 3 * d;                // qkv token stride
  const long long gs = (long long)heads * d;                    // grad-out token stride
  const float* qb = qkv + b * n * ts + (long long)h * 3 * d;    // q | k | v at + 0 | d | 2 d
  const float* gb = go + b * n * gs + (long long)h * d;
  const float* lrow = lse2 + bh * n;
  float* drow = dws + bh * n;
  // S = X1 . Y1, dP = X2 . Y2 (X: other rows, Y: own rows); G: the A operand of the accumulating product (other rows)
  const float* x1 = KM ? qb : qb + d;
  const float* y1 = KM ? qb + d : qb;
  const float* x2 = MODE == kDK ? gb : qb + 2 * d;
  const float* y2 = MODE == kDK ? qb + 2 * d : gb;
  const long long x2s = MODE == kDK ? gs : ts, y2s = MODE == kDK ? ts : gs;
  const float* gp = MODE == kDV ? gb : MODE == kDK ? qb : qb + d;
  const long long gps = MODE == kDV ? gs : ts;
  const int dch = (d + 15) >> 4;
  const int x = ob * 16 + col;
  const bool xok = x < n;
  const long long xs = xok ? x : 0;
  const float* y1row = y1 + xs * ts;
  const float* y2row = y2 + xs * y2s;
  f32x4 y1r[kRegChunks], y2r[kRegChunks];
  if (REG) {
#pragma unroll
    for (int c = 0; c < kRegChunks; ++c)
      if (c < dch) {
        y1r[c] = load4<VEC>(y1row, c * 16 + 4 * g, d, xok);
        if (DP) y2r[c] = load4<VEC>(y2row, c * 16 + 4 * g, d, xok);
      }
  }
  const float lx = KM && xok ? lrow[x] : 0.f;
  float dx = 0.f;
  if (MODE == kDK) {
    // D_j = v_j . dV_j over this lane's quarter of d, then across the four lane groups (same bits in every lane)
    const float* dvrow = dqkv + ((b * n + xs) * heads + h) * 3 * (long long)d + 2 * d;
    for (int c = 0; c < dch; ++c) {
      const f32x4 v = load4<VEC>(y2row, c * 16 + 4 * g, d, xok), w = load4<VEC>(dvrow, c * 16 + 4 * g, d, xok);
#pragma unroll
      for (int t = 0; t < 4; ++t) dx = fmaf(v[t], w[t], dx);
    }
    dx += __shfl_xor(dx, 16);
    dx += __shfl_xor(dx, 32);
    if (g == 0 && xok && blockIdx.z == 0) drow[x] = dx;
  }
  f32x4 o[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int y0 = 0; y0 < n; y0 += 16) {
    const int yc = y0 + col;
    const bool ycok = yc < n;
    const long long ycs = ycok ? yc : 0;
    const float* x1row = x1 + ycs * ts;
    const float* x2row = x2 + ycs * x2s;
    f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
    if (REG) {
#pragma unroll
      for (int c = 0; c < kRegChunks; ++c)
        if (c < dch) {
          s = mfma4(load4<VEC>(x1row, c * 16 + 4 * g, d, ycok), y1r[c], s);
          if (DP) dp = mfma4(load4<VEC>(x2row, c * 16 + 4 * g, d, ycok), y2r[c], dp);
        }
    } else {
      for (int c = 0; c < dch; ++c) {
        s = mfma4(load4<VEC>(x1row, c * 16 + 4 * g, d, ycok), load4<VEC>(y1row, c * 16 + 4 * g, d, xok), s);
        if (DP) dp = mfma4(load4<VEC>(x2row, c * 16 + 4 * g, d, ycok), load4<VEC>(y2row, c * 16 + 4 * g, d, xok), dp);
      }
    }
    // s[r] = S[y0 + 4 g + r][x] (other row, own column; unscaled), dp[r] likewise
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int yr = y0 + 4 * g + r;
      const bool ok = yr < n;
      const long long yrs = ok ? yr : 0;
      float w = ok ? __builtin_amdgcn_exp2f(fmaf(s[r], c2, KM ? -lx : -lrow[yrs])) : 0.f;
      if (DP) w *= dp[r] - (KM ? dx : (ok ? drow[yrs] : 0.f));
      // OUT^T[c][x] += sum_y G^T[c][y] W[y][x]: A = G^T (row c = col, k = g <-> other row yr), B = W (k = g, column x)
      const float* grow = gp + yrs * gps;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int c = dv0 + 16 * t + col;
        const float a = ok && c < d ? grow[c] : 0.f;
        o[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w, o[t], 0, 0, 0);
      }
    }
  }
  if (!xok) return;
  // o[t][r] = OUT^T[dv0 + 16 t + 4 g + r][x]
  constexpr int part = MODE == kDV ? 2 : MODE == kDK ? 1 : 0;
  const float f = MODE == kDV ? 1.f : scale;
  float* orow = dqkv + ((b * n + x) * heads + h) * 3 * (long long)d + part * d;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int c = dv0 + 16 * t + 4 * g;
    const f32x4 v = o[t] * f;
    if (VEC) {
      if (c < d) *reinterpret_cast<f32x4*>(orow + c) = v;
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (c + r < d) orow[c + r] = v[r];
    }
  }
}

template <int MODE, bool VEC>
void launch(bool reg, int nt, dim3 grid, hipStream_t s, const float* q, const float* g, const float* l, float* dw, float* dq,
            int n, int heads, int d, float c2, float scale, int tiles) {
#define DLWP_GAB(NT, R) hipLaunchKernelGGL((bwd_kernel<MODE, NT, VEC, R>), grid, dim3(256), 0, s, q, g, l, dw, dq, n, heads, d, c2, scale, tiles)
  if (!reg) DLWP_GAB(8, false);
  else if (nt == 1) DLWP_GAB(1, true);
  else if (nt == 2) DLWP_GAB(2, true);
  else if (nt == 4) DLWP_GAB(4, true);
  else DLWP_GAB(8, true);
#undef DLWP_GAB
}

}  // namespace gattn_bwd
}  // namespace dlwp

using namespace dlwp;

extern "C" size_t dlwp_global_attn_bwd_workspace_bytes(int32_t batch, int32_t heads, int32_t tokens) {
  if (batch <= 0 || heads <= 0 || tokens <= 0) return 0;
  return (size_t)batch * heads * tokens * sizeof(float);
}

extern "C" int32_t dlwp_global_attn_bwd_f32(const float* qkv_dev, const float* grad_out_dev, const float* stats_dev,
                                            float* dqkv_dev, int32_t batch, int32_t tokens, int32_t heads, int32_t head_dim,
                                            float scale, void* workspace, size_t workspace_bytes, void* stream) {
  DLWP_REQUIRE(qkv_dev && grad_out_dev && stats_dev && dqkv_dev && workspace, DLWP_ERR_INVALID_ARGUMENT,
               "global attention backward: null argument");
  DLWP_REQUIRE(batch > 0 && tokens > 0 && heads > 0 && head_dim > 0, DLWP_ERR_INVALID_ARGUMENT,
               "global attention backward: bad shape (batch %d, tokens %d, heads %d, head_dim %d)", batch, tokens, heads,
               head_dim);
  DLWP_REQUIRE(head_dim <= gattn_bwd::kMaxHeadDim, DLWP_ERR_UNSUPPORTED,
               "global attention backward: head_dim %d above %d", head_dim, gattn_bwd::kMaxHeadDim);
  DLWP_REQUIRE(workspace_bytes >= dlwp_global_attn_bwd_workspace_bytes(batch, heads, tokens), DLWP_ERR_WORKSPACE,
               "global attention backward: workspace of %zu bytes, %zu needed", workspace_bytes,
               dlwp_global_attn_bwd_workspace_bytes(batch, heads, tokens));
  DLWP_REQUIRE(std::isfinite(scale), DLWP_ERR_INVALID_ARGUMENT, "global attention backward: scale is not finite");
  DLWP_REQUIRE(dqkv_dev != qkv_dev && dqkv_dev != grad_out_dev, DLWP_ERR_INVALID_ARGUMENT,
               "global attention backward: dqkv aliases an input");
  const auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const bool vec = head_dim % 4 == 0 && al(qkv_dev) && al(grad_out_dev) && al(dqkv_dev);
  const int dch = (head_dim + 15) / 16;
  const bool reg = dch <= gattn_bwd::kRegChunks;
  const int nt = !reg ? 8 : dch <= 1 ? 1 : dch <= 2 ? 2 : dch <= 4 ? 4 : 8;
  const int slices = (dch + nt - 1) / nt;
  const int tiles = (tokens + 15) / 16;
  const unsigned gx = (unsigned)((tiles + gattn_bwd::kWaves - 1) / gattn_bwd::kWaves);
  const float c2 = scale * 1.4426950408889634f;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // grid.y carries (sample, head) pairs: chunks of whole samples keep it within its 65535 limit
  const int per = std::max(1, 65535 / heads);
  for (int b0 = 0; b0 < batch; b0 += per) {
    const int nb = std::min(per, batch - b0);
    const size_t off = (size_t)b0 * tokens;
    const float* q = qkv_dev + off * heads * 3 * head_dim;
    const float* g = grad_out_dev + off * heads * head_dim;
    const float* l = stats_dev + off * heads;
    float* dw = reinterpret_cast<float*>(workspace) + off * heads;
    float* dq = dqkv_dev + off * heads * 3 * head_dim;
    const dim3 grid(gx, (unsigned)(nb * heads), (unsigned)slices);
    // kDK reads kDV's dV, kDQ reads kDK's D: stream order is the only synchronisation needed
    if (vec) {
      gattn_bwd::launch<gattn_bwd::kDV, true>(reg, nt, grid, s, q, g, l, dw, dq, tokens, heads, head_dim, c2, scale, tiles);
      gattn_bwd::launch<gattn_bwd::kDK, true>(reg, nt, grid, s, q, g, l, dw, dq, tokens, heads, head_dim, c2, scale, tiles);
      gattn_bwd::launch<gattn_bwd::kDQ, true>(reg, nt, grid, s, q, g, l, dw, dq, tokens, heads, head_dim, c2, scale, tiles);
    } else {
      gattn_bwd::launch<gattn_bwd::kDV, false>(reg, nt, grid, s, q, g, l, dw, dq, tokens, heads, head_dim, c2, scale, tiles);
      gattn_bwd::launch<gattn_bwd::kDK, false>(reg, nt, grid, s, q, g, l, dw, dq, tokens, heads, head_dim, c2, scale, tiles);
      gattn_bwd::launch<gattn_bwd::kDQ, false>(reg, nt, grid, s, q, g, l, dw, dq, tokens, heads, head_dim, c2, scale, tiles);
    }
    DLWP_HIP_CHECK(hipGetLastError());
  }
  return DLWP_OK;
}
