// Global multi-head self-attention of the diffusion U-Net's AttentionBlock on MI355X (gfx950).
//
// Replaces the core of AttentionBlock.forward (reference models/diffusion_models/modern_unet/modern_unet.py:565-571):
//   attn = einsum("bihd,bjhd->bijh", q, k) * scale;  attn = attn.softmax(dim=1);  res = einsum("bijh,bjhd->bihd", attn, v)
// over ALL N = H W tokens of a feature map (no windows).  The softmax runs over dim=1, the QUERY axis: every key's
// weights over all queries sum to one.  With s_ij = scale q_i . k_j, m_j = max_i s_ij, Z_j = sum_i exp(s_ij - m_j):
//   res_i = sum_j exp(s_ij - L_j) v_j,   L_j = m_j + ln Z_j.
//
// Input is the projection Linear's output as it stands, [Bt, N, heads, {q, k, v}, d] (modern_unet.py:558-562: view
// [B, N, heads, 3 d], chunk(3, -1)); output is [Bt, N, heads d], token-major, the input of the output Linear.
//
// Two passes, neither of which writes anything of size N x N:
//   pass 1 (key statistics): one wave per 16 keys of one (sample, head) streams every 16-query tile, S = Q K^T on the
//          accumulator (lane column = key, rows = four queries), online max / rescaled sum per key; the four lanes of a
//          key column are merged by shuffles and L2_j = (m_j + ln Z_j) log2(e) is written to the workspace
//          [Bt heads N] (base 2, so pass 2 needs one v_exp_f32 per score and no conversion).
//   pass 2 (output): one wave per 16 queries and one slice of <= 128 output columns streams every 16-key tile,
//          recomputes S^T = K Q^T (rows = keys, lane column = query), P = exp2(S^T scale log2(e) - L2_j) -- already
//          normalised, never above 1 -- and accumulates O^T += V^T P.  The P tile is consumed as the B operand straight
//          from the accumulator registers: the key index on the accumulator rows is the contraction index of O^T += V^T P
//          (window_attn.hip's "swapped" orientation).  No row normalisation follows.
// Products run on v_mfma_f32_16x16x4_f32 (exact fp32 FMA chains): 32 cycles per instruction leave 24 cycles of vector
// issue per MFMA for the exponentials and the statistics.  The contraction over d is walked in
// chunks of 16: lane group g = lane / 16 supplies d = 16 c + 4 g + t to MFMA t of chunk c, so both operands arrive as
// one 16-byte load per lane and chunk.  Tails: queries >= N enter no statistic (score -inf), keys >= N get P = 0, d is
// padded with zeros to the chunk.  Row bases are 64-bit.  No atomics: results are bitwise reproducible and a sample's
// result does not depend on its batch neighbours.
#include "global_attn_common.hpp"

namespace dlwp {
namespace gattn {

constexpr float kLog2e = 1.4426950408889634f;

// merge of two online-softmax states (base 2); the -inf guard keeps a state that has seen nothing yet
__device__ __forceinline__ void merge(float& m, float& z, float mo, float zo) {
  const float mx = fmaxf(m, mo);
  if (mx != -INFINITY) {
    z = z * __builtin_amdgcn_exp2f(m - mx) + zo * __builtin_amdgcn_exp2f(mo - mx);
    m = mx;
  }
}

// pass 1: lse2[bh][j] = log2(e) (m_j + ln Z_j).  grid (ceil(kblocks / 4), batch * heads), block 256.
template <bool VEC, bool KREG>
__global__ __launch_bounds__(256) void key_stats_kernel(const float* __restrict__ qkv, float* __restrict__ lse2, int n,
                                                        int heads, int d, float c2, int kblocks) {
  const int lane = threadIdx.x & 63, col = lane & 15, g = lane >> 4;
  const int kb = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (kb >= kblocks) return;
  const long long bh = blockIdx.y, b = bh / heads;
  const int h = (int)(bh % heads);
  const long long ts = (long long)heads * 3 * d;               // token stride
  const float* base = qkv + b * n * ts + (long long)h * 3 * d;
  const int dch = (d + 15) >> 4;
  const int j = kb * 16 + col;
  const bool jok = j < n;
  const float* krow = base + (long long)(jok ? j : 0) * ts + d;
  f32x4 kr[kRegChunks];
  if (KREG) {
#pragma unroll
    for (int c = 0; c < kRegChunks; ++c)
      if (c < dch) kr[c] = load4<VEC>(krow, c * 16 + 4 * g, d, jok);
  }
  float m = -INFINITY, z = 0.f;
  for (int i0 = 0; i0 < n; i0 += 16) {
    const int i = i0 + col;
    const bool iok = i < n;
    const float* qrow = base + (long long)(iok ? i : 0) * ts;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (KREG) {
#pragma unroll
      for (int c = 0; c < kRegChunks; ++c)
        if (c < dch) acc = mfma4(load4<VEC>(qrow, c * 16 + 4 * g, d, iok), kr[c], acc);
    } else {
      for (int c = 0; c < dch; ++c)
        acc = mfma4(load4<VEC>(qrow, c * 16 + 4 * g, d, iok), load4<VEC>(krow, c * 16 + 4 * g, d, jok), acc);
    }
    // acc[r] = S[i0 + 4 g + r][j] (unscaled)
    float s[4];
    float mx = m;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      s[r] = i0 + 4 * g + r < n ? acc[r] * c2 : -INFINITY;
      mx = fmaxf(mx, s[r]);
    }
    if (mx != -INFINITY) {
      float zs = z * __builtin_amdgcn_exp2f(m - mx);
#pragma unroll
      for (int r = 0; r < 4; ++r) zs += __builtin_amdgcn_exp2f(s[r] - mx);
      z = zs;
      m = mx;
    }
  }
  // the four lanes of a key column saw disjoint query rows: merge them (every lane ends with the same bits)
#pragma unroll
  for (int off = 16; off <= 32; off <<= 1) {
    const float mo = __shfl_xor(m, off), zo = __shfl_xor(z, off);
    merge(m, z, mo, zo);
  }
  if (g == 0 && jok) lse2[bh * n + j] = m + __builtin_amdgcn_logf(z);
}

// pass 2: out[b][i][h d + dv] for dv in slice blockIdx.z (NT 16-column tiles).  grid (ceil(qblocks / 4), batch * heads,
// slices), block 256.
template <int NT, bool VEC, bool QREG>
__global__ __launch_bounds__(256) void output_kernel(const float* __restrict__ qkv, const float* __restrict__ lse2,
                                                     float* __restrict__ out, int n, int heads, int d, float c2,
                                                     int qblocks) {
  const int lane = threadIdx.x & 63, col = lane & 15, g = lane >> 4;
  const int qb = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (qb >= qblocks) return;
  const long long bh = blockIdx.y, b = bh / heads;
  const int h = (int)(bh % heads);
  const int dv0 = blockIdx.z * NT * 16;
  const long long ts = (long long)heads * 3 * d;
  const float* base = qkv + b * n * ts + (long long)h * 3 * d;
  const float* lrow = lse2 + bh * n;
  const int dch = (d + 15) >> 4;
  const int i = qb * 16 + col;
  const bool iok = i < n;
  const float* qrow = base + (long long)(iok ? i : 0) * ts;
  f32x4 qr[kRegChunks];
  if (QREG) {
#pragma unroll
    for (int c = 0; c < kRegChunks; ++c)
      if (c < dch) qr[c] = load4<VEC>(qrow, c * 16 + 4 * g, d, iok);
  }
  f32x4 o[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int j0 = 0; j0 < n; j0 += 16) {
    const int jk = j0 + col;
    const bool jkok = jk < n;
    const float* krow = base + (long long)(jkok ? jk : 0) * ts + d;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (QREG) {
#pragma unroll
      for (int c = 0; c < kRegChunks; ++c)
        if (c < dch) acc = mfma4(load4<VEC>(krow, c * 16 + 4 * g, d, jkok), qr[c], acc);
    } else {
      for (int c = 0; c < dch; ++c)
        acc = mfma4(load4<VEC>(krow, c * 16 + 4 * g, d, jkok), load4<VEC>(qrow, c * 16 + 4 * g, d, iok), acc);
    }
    // acc[r] = S^T[j0 + 4 g + r][i] (unscaled); P = exp2(s c2 - L2_j), 0 for keys >= N
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int jr = j0 + 4 * g + r;
      const bool ok = jr < n;
      const float p = ok ? __builtin_amdgcn_exp2f(fmaf(acc[r], c2, -lrow[ok ? jr : 0])) : 0.f;
      // O^T[dv][i] += sum_j V^T[dv][j] P[j][i]: A = V^T (row dv = col, k = g <-> key jr), B = P (k = g, column i)
      const float* vrow = base + (long long)(ok ? jr : 0) * ts + 2 * d;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int dv = dv0 + 16 * t + col;
        const float a = ok && dv < d ? vrow[dv] : 0.f;
        o[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, p, o[t], 0, 0, 0);
      }
    }
  }
  if (!iok) return;
  // o[t][r] = O^T[dv0 + 16 t + 4 g + r][i]
  float* orow = out + ((b * n + i) * heads + h) * (long long)d;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int dv = dv0 + 16 * t + 4 * g;
    if (VEC) {
      if (dv < d) *reinterpret_cast<f32x4*>(orow + dv) = o[t];
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (dv + r < d) orow[dv + r] = o[t][r];
    }
  }
}

}  // namespace gattn
}  // namespace dlwp

using namespace dlwp;

extern "C" size_t dlwp_global_attn_workspace_bytes(int32_t batch, int32_t heads, int32_t tokens) {
  if (batch <= 0 || heads <= 0 || tokens <= 0) return 0;
  return (size_t)batch * heads * tokens * sizeof(float);
}

extern "C" int32_t dlwp_global_attn_f32(const float* qkv_dev, float* out_dev, int32_t batch, int32_t tokens,
                                        int32_t heads, int32_t head_dim, float scale, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  DLWP_REQUIRE(qkv_dev && out_dev && workspace, DLWP_ERR_INVALID_ARGUMENT, "global attention: null argument");
  DLWP_REQUIRE(batch > 0 && tokens > 0 && heads > 0 && head_dim > 0, DLWP_ERR_INVALID_ARGUMENT,
               "global attention: bad shape (batch %d, tokens %d, heads %d, head_dim %d)", batch, tokens, heads, head_dim);
  DLWP_REQUIRE(workspace_bytes >= dlwp_global_attn_workspace_bytes(batch, heads, tokens), DLWP_ERR_WORKSPACE,
               "global attention: workspace of %zu bytes, %zu needed", workspace_bytes,
               dlwp_global_attn_workspace_bytes(batch, heads, tokens));
  DLWP_REQUIRE(std::isfinite(scale), DLWP_ERR_INVALID_ARGUMENT, "global attention: scale is not finite");
  DLWP_REQUIRE((long long)heads * 3 * head_dim <= INT32_MAX, DLWP_ERR_INVALID_ARGUMENT, "global attention: heads * 3 * head_dim overflows");
  const bool vec = head_dim % 4 == 0 && (reinterpret_cast<uintptr_t>(qkv_dev) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(out_dev) & 15) == 0;
  const int dch = (head_dim + 15) / 16;
  const bool reg = dch <= gattn::kRegChunks;
  const int nt = !reg ? 8 : dch <= 1 ? 1 : dch <= 2 ? 2 : dch <= 4 ? 4 : 8;
  const int slices = (dch + nt - 1) / nt;
  const int tiles = (tokens + 15) / 16;
  const unsigned gx = (unsigned)((tiles + gattn::kWaves - 1) / gattn::kWaves);
  const float c2 = scale * gattn::kLog2e;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // grid.y carries (sample, head) pairs: chunks of whole samples keep it within its 65535 limit
  const int per = std::max(1, 65535 / heads);
  for (int b0 = 0; b0 < batch; b0 += per) {
    const int nb = std::min(per, batch - b0);
    const size_t off = (size_t)b0 * tokens;
    const float* q = qkv_dev + off * heads * 3 * head_dim;
    float* o = out_dev + off * heads * head_dim;
    float* l = reinterpret_cast<float*>(workspace) + off * heads;
    const dim3 g1(gx, (unsigned)(nb * heads)), g2(gx, (unsigned)(nb * heads), (unsigned)slices);
#define DLWP_GA1(V, R) hipLaunchKernelGGL((gattn::key_stats_kernel<V, R>), g1, dim3(256), 0, s, q, l, tokens, heads, head_dim, c2, tiles)
    if (vec) {
      if (reg) DLWP_GA1(true, true); else DLWP_GA1(true, false);
    } else {
      if (reg) DLWP_GA1(false, true); else DLWP_GA1(false, false);
    }
#undef DLWP_GA1
#define DLWP_GA2(NT, V, R) hipLaunchKernelGGL((gattn::output_kernel<NT, V, R>), g2, dim3(256), 0, s, q, l, o, tokens, heads, head_dim, c2, tiles)
#define DLWP_GA2V(V)                     \
  do {                                   \
    if (!reg) DLWP_GA2(8, V, false);     \
    else if (nt == 1) DLWP_GA2(1, V, true); \
    else if (nt == 2) DLWP_GA2(2, V, true); \
    else if (nt == 4) DLWP_GA2(4, V, true); \
    else DLWP_GA2(8, V, true);           \
  } while (0)
    if (vec) DLWP_GA2V(true);
    else DLWP_GA2V(false);
#undef DLWP_GA2V
#undef DLWP_GA2
    DLWP_HIP_CHECK(hipGetLastError());
  }
  return DLWP_OK;
}
