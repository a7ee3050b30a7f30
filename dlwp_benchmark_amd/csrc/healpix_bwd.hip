// Backward of the HEALPix padding and of the HEALPix-padded 3x3 convolution (conv.hip) on MI355X (gfx950).
//
// Forward (reference utils/healpix.py:165-368 and :69-114): xp = pad(x) is a gather through the table of healpix.pad_table,
// every padded cell a copy of one source cell or the mean of two; z = Conv2d(3x3, padding 0)(xp).
// The adjoint of the gather is the CSR of healpix.pad_adjoint_table: per source cell s of one sample, the padded positions
// q = face*(H+2p)*(W+2p) + padded pixel that read it, with weight 1 or 0.5.  Both kernels are gathers through it -- each
// element of dx has one writer, nothing is zeroed first, no atomics -- so results are bitwise reproducible and a sample's
// gradient does not depend on its batch neighbours.
//
//   healpix_pad_bwd_kernel   dx[s] = sum_e weight_e dy[q_e]                                   (any p the forward takes)
//   conv3x3_hpx_bwd_kernel   dx = pad^T (conv^T dz) for p = 1 without the (H+2)^2 intermediate:
//     interior term   the transposed 3x3 with zero padding on the own face, dx_i += sum_co sum_t W[co, ci, 8-t] dz[co, i+t]:
//                     the tile / LDS staging of conv3x3_cyl_kernel with dz as the input and the weights flipped and
//                     transposed while they are staged
//     halo term       a face-border cell is also read by halo positions (P, Q) of neighbouring faces.  Pass 1
//                     (halo_ring_kernel) computes the transposed 3x3 at every halo position once: the partial stencil
//                     sum_co sum_{r,c} W[co, ci, r, c] dz[co, P-r, Q-c] over the taps inside the face (<= 3 on an edge,
//                     1 on a corner) into a ring buffer of 2 (W+2) + 2 H cells per (face, channel).  Pass 2's epilogue
//                     adds, for each halo entry of a border cell, weight * ring value; the entry for the cell's own
//                     position is the interior term.  (Computing the stencils in the epilogue itself, per border thread
//                     with a loop over cout, serialised the border threads' global loads: a training step of UNetHPX at
//                     nside 32 took 4.7x the torch recomputation.  The ring is n cin 4 (H+1) floats, not (H+2)^2.)
#include "common.hpp"

namespace dlwp {
namespace hpx_bwd {

constexpr int G_CHUNK = 8;   // dz channels staged per LDS round

struct Params {
  const float* dz;           // [N][cout][H][W]
  const float* w;            // [cout][cin][3][3], the forward layout
  float* dx;                 // [N][cin][H][W]
  int N, H, W, cin, cout;
  const int* adj_ptr;        // [12*H*W + 1]
  const int* adj_idx;        // padded positions face*(H+2)*(W+2) + (P*(W+2) + Q)
  const float* adj_w;
  float* ring;               // [N][cin][2 (W+2) + 2 H]: pass 1's halo values
};

// the halo ring of a padded face, 2 (W+2) + 2 H cells: top row, bottom row, left column, right column (corners in the rows)
__device__ __forceinline__ int ring_size(int H, int W) { return 2 * (W + 2) + 2 * H; }
__device__ __forceinline__ int ring_index(int P, int Q, int H, int W) {
  if (P == 0) return Q;
  if (P == H + 1) return (W + 2) + Q;
  return 2 * (W + 2) + (Q == 0 ? 0 : H) + (P - 1);
}

// pass 1: the transposed 3x3 at every halo position of every face, ring [N][cin][R] -- sum_co sum_{r,c} W[co, ci, r, c]
// dz[co, P-r, Q-c] over the taps inside the face (<= 3 on an edge, 1 on a corner); one thread per (face, ci, ring cell)
__global__ __launch_bounds__(256) void halo_ring_kernel(const Params p, long long total) {
  const int R = ring_size(p.H, p.W);
  const long long HW = (long long)p.H * p.W;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int rc = (int)(i % R);
    const long long nc = i / R;
    const int ci = (int)(nc % p.cin);
    const long long n = nc / p.cin;
    int P, Q;
    if (rc < p.W + 2) { P = 0; Q = rc; }
    else if (rc < 2 * (p.W + 2)) { P = p.H + 1; Q = rc - (p.W + 2); }
    else { const int j = rc - 2 * (p.W + 2); Q = j < p.H ? 0 : p.W + 1; P = 1 + (j < p.H ? j : j - p.H); }
    float acc = 0.f;
    const float* dz = p.dz + n * p.cout * HW;
    for (int r = 0; r < 3; ++r) {
      const int y = P - r;
      if (y < 0 || y >= p.H) continue;
      for (int c = 0; c < 3; ++c) {
        const int x = Q - c;
        if (x < 0 || x >= p.W) continue;
        const float* wp = p.w + (long long)ci * 9 + r * 3 + c;
        const float* zp = dz + (long long)y * p.W + x;
        for (int co = 0; co < p.cout; ++co) acc = fmaf(wp[(long long)co * p.cin * 9], zp[(long long)co * HW], acc);
      }
    }
    p.ring[i] = acc;
  }
}

// pass 2: TH x TW dx tile per workgroup (one thread per cell), KC dx channels per thread (blockIdx.z selects the chunk)
template <int TH, int TW, int KC>
__global__ __launch_bounds__(TH * TW) void conv3x3_hpx_bwd_kernel(const Params p) {
  constexpr int NT = TH * TW;
  __shared__ float s_in[G_CHUNK][TH + 2][TW + 2];
  __shared__ float s_w[KC][G_CHUNK][9];
  const int tid = threadIdx.x;
  const int tx = tid % TW, ty = tid / TW;
  const int tiles_w = (p.W + TW - 1) / TW;
  const int w0 = (blockIdx.x % tiles_w) * TW, h0 = (blockIdx.x / tiles_w) * TH;
  const int b = blockIdx.y;
  const int ci0 = blockIdx.z * KC;
  const int ow = w0 + tx, oh = h0 + ty;
  const long long HW = (long long)p.H * p.W;
  float acc[KC];
#pragma unroll
  for (int k = 0; k < KC; ++k) acc[k] = 0.f;
  for (int g0 = 0; g0 < p.cout; g0 += G_CHUNK) {
    __syncthreads();
    for (int i = tid; i < G_CHUNK * (TH + 2) * (TW + 2); i += NT) {
      const int g = i / ((TH + 2) * (TW + 2));
      const int rem = i % ((TH + 2) * (TW + 2));
      const int r = rem / (TW + 2), cc = rem % (TW + 2);
      const int co = g0 + g, ih = h0 + r - 1, iw = w0 + cc - 1;
      float v = 0.f;
      if (co < p.cout && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W)
        v = p.dz[((long long)b * p.cout + co) * HW + (long long)ih * p.W + iw];
      (&s_in[0][0][0])[i] = v;
    }
    for (int i = tid; i < KC * G_CHUNK * 9; i += NT) {
      const int k = i / (G_CHUNK * 9), rem = i % (G_CHUNK * 9);
      const int g = rem / 9, t = rem % 9;
      const int ci = ci0 + k, co = g0 + g;
      (&s_w[0][0][0])[i] = (ci < p.cin && co < p.cout) ? p.w[((long long)co * p.cin + ci) * 9 + (8 - t)] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < G_CHUNK; ++g) {
      float v[9];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) v[r * 3 + cc] = s_in[g][ty + r][tx + cc];
#pragma unroll
      for (int k = 0; k < KC; ++k)
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[k] = fmaf(v[t], s_w[k][g][t], acc[k]);
    }
  }
  if (ow >= p.W || oh >= p.H) return;
  if (oh == 0 || oh == p.H - 1 || ow == 0 || ow == p.W - 1) {
    const int face = b % 12, s0 = b - face;
    const int PW = p.W + 2, PHW = (p.H + 2) * PW, R = ring_size(p.H, p.W);
    const int s = face * (int)HW + oh * p.W + ow;
    for (int e = p.adj_ptr[s]; e < p.adj_ptr[s + 1]; ++e) {
      const int q = p.adj_idx[e];
      const int fq = q / PHW, cell = q - fq * PHW;
      const int P = cell / PW, Q = cell % PW;
      if (P >= 1 && P <= p.H && Q >= 1 && Q <= p.W) continue;      // the own position: the interior term
      const float we = p.adj_w[e];
      const float* rr = p.ring + ((long long)(s0 + fq) * p.cin + ci0) * R + ring_index(P, Q, p.H, p.W);
#pragma unroll
      for (int k = 0; k < KC; ++k)
        if (ci0 + k < p.cin) acc[k] = fmaf(we, rr[(long long)k * R], acc[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < KC; ++k) {
    const int ci = ci0 + k;
    if (ci < p.cin) p.dx[((long long)b * p.cin + ci) * HW + (long long)oh * p.W + ow] = acc[k];
  }
}

// dx [N][C][H][W] from dy [N][C][H+2p][W+2p] through the adjoint CSR
__global__ __launch_bounds__(256) void healpix_pad_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx,
                                                              const int* __restrict__ adj_ptr, const int* __restrict__ adj_idx,
                                                              const float* __restrict__ adj_w, int C, int HW, int PHW,
                                                              long long total) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int cell = (int)(i % HW);
    const long long nc = i / HW;
    const int c = (int)(nc % C);
    const long long n = nc / C;
    const int face = (int)(n % 12);
    const long long s0 = n - face;
    const int s = face * HW + cell;
    float acc = 0.f;
    for (int e = adj_ptr[s]; e < adj_ptr[s + 1]; ++e) {
      const int q = adj_idx[e];
      const int fq = q / PHW;
      acc = fmaf(adj_w[e], dy[((s0 + fq) * C + c) * PHW + (q - fq * PHW)], acc);
    }
    dx[i] = acc;
  }
}

}  // namespace hpx_bwd
}  // namespace dlwp

using namespace dlwp;

template <int KC>
static void launch_bwd_kc(const hpx_bwd::Params& p, hipStream_t s) {
  const int zc = (p.cin + KC - 1) / KC;
  auto tiles = [&](int th, int tw) { return ((p.W + tw - 1) / tw) * ((p.H + th - 1) / th); };
  if (p.W >= 32)
    hipLaunchKernelGGL((hpx_bwd::conv3x3_hpx_bwd_kernel<8, 32, KC>), dim3(tiles(8, 32), p.N, zc), dim3(256), 0, s, p);
  else if (p.W >= 16)
    hipLaunchKernelGGL((hpx_bwd::conv3x3_hpx_bwd_kernel<16, 16, KC>), dim3(tiles(16, 16), p.N, zc), dim3(256), 0, s, p);
  else
    hipLaunchKernelGGL((hpx_bwd::conv3x3_hpx_bwd_kernel<8, 8, KC>), dim3(tiles(8, 8), p.N, zc), dim3(64), 0, s, p);
}

extern "C" size_t dlwp_conv3x3_hpx_bwd_data_workspace_bytes(int32_t n_faces, int32_t H, int32_t W, int32_t cin) {
  if (n_faces <= 0 || H <= 0 || W <= 0 || cin <= 0) return 0;
  return (size_t)n_faces * cin * (2 * (W + 2) + 2 * H) * sizeof(float);
}

extern "C" int32_t dlwp_conv3x3_hpx_bwd_data_f32(const float* dy, const float* weight, float* dx, int32_t n_faces, int32_t H,
                                                 int32_t W, int32_t cin, int32_t cout, const int32_t* adj_indptr,
                                                 const int32_t* adj_index, const float* adj_weight, void* workspace,
                                                 size_t workspace_bytes, void* stream) {
  DLWP_REQUIRE(dy && weight && dx && adj_indptr && adj_index && adj_weight && workspace, DLWP_ERR_INVALID_ARGUMENT,
               "null argument");
  DLWP_REQUIRE(n_faces > 0 && n_faces % 12 == 0, DLWP_ERR_INVALID_ARGUMENT, "n_faces=%d is not a multiple of 12", n_faces);
  DLWP_REQUIRE(H > 0 && W > 0 && cin > 0 && cout > 0, DLWP_ERR_INVALID_ARGUMENT, "bad shape");
  DLWP_REQUIRE(H == W, DLWP_ERR_INVALID_ARGUMENT, "HEALPix faces are square (got %d x %d)", H, W);
  DLWP_REQUIRE((long long)12 * (H + 2) * (W + 2) < (1ll << 31), DLWP_ERR_INVALID_ARGUMENT, "face too large for the 32-bit table");
  DLWP_REQUIRE(n_faces <= 65535, DLWP_ERR_UNSUPPORTED, "n_faces %d exceeds the grid's y dimension (65535)", n_faces);
  DLWP_REQUIRE(dx != dy, DLWP_ERR_INVALID_ARGUMENT, "dx may not alias dy");
  const size_t need = dlwp_conv3x3_hpx_bwd_data_workspace_bytes(n_faces, H, W, cin);
  DLWP_REQUIRE(workspace_bytes >= need, DLWP_ERR_WORKSPACE, "workspace of %zu bytes, %zu needed", workspace_bytes, need);
  hpx_bwd::Params p;
  p.dz = dy; p.w = weight; p.dx = dx; p.N = n_faces; p.H = H; p.W = W; p.cin = cin; p.cout = cout;
  p.adj_ptr = adj_indptr; p.adj_idx = adj_index; p.adj_w = adj_weight; p.ring = static_cast<float*>(workspace);
  // the forward's choice of dx channels per thread (conv.hip launch_conv3x3), with cin as the output channel count
  const int th = W >= 32 ? 8 : (W >= 16 ? 16 : 8), tw = W >= 32 ? 32 : (W >= 16 ? 16 : 8);
  const long long tiles = (long long)((W + tw - 1) / tw) * ((H + th - 1) / th) * n_faces;
  const long long wgs16 = tiles * ((cin + 15) / 16), waves4 = tiles * ((cin + 3) / 4) * (th * tw / 64);
  DLWP_REQUIRE((cin + 0ll) <= 65535ll, DLWP_ERR_UNSUPPORTED, "cin %d exceeds the grid's z dimension (65535)", cin);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const long long ring_total = (long long)(need / sizeof(float));
  long long blocks = (ring_total + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(hpx_bwd::halo_ring_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p, ring_total);
  if (wgs16 >= 1024) launch_bwd_kc<16>(p, s);
  else if (waves4 >= 2048) launch_bwd_kc<4>(p, s);
  else launch_bwd_kc<1>(p, s);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" int32_t dlwp_healpix_pad_bwd_f32(const float* dy, float* dx, const int32_t* adj_indptr, const int32_t* adj_index,
                                            const float* adj_weight, int32_t n_faces, int32_t channels, int32_t H, int32_t W,
                                            int32_t pad, void* stream) {
  DLWP_REQUIRE(dy && dx && adj_indptr && adj_index && adj_weight, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(n_faces > 0 && n_faces % 12 == 0, DLWP_ERR_INVALID_ARGUMENT, "n_faces=%d is not a multiple of 12", n_faces);
  DLWP_REQUIRE(channels > 0 && H > 0 && W > 0 && pad > 0, DLWP_ERR_INVALID_ARGUMENT, "bad shape");
  DLWP_REQUIRE(H == W, DLWP_ERR_INVALID_ARGUMENT, "HEALPix faces are square (got %d x %d)", H, W);
  DLWP_REQUIRE(pad <= H, DLWP_ERR_INVALID_ARGUMENT, "padding %d does not fit a %d x %d face", pad, H, W);
  DLWP_REQUIRE((long long)12 * (H + 2 * pad) * (W + 2 * pad) < (1ll << 31), DLWP_ERR_INVALID_ARGUMENT, "face too large");
  DLWP_REQUIRE(dx != dy, DLWP_ERR_INVALID_ARGUMENT, "dx may not alias dy");
  const int PHW = (H + 2 * pad) * (W + 2 * pad);
  const long long total = (long long)n_faces * channels * H * W;
  long long blocks = (total + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(hpx_bwd::healpix_pad_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     dy, dx, adj_indptr, adj_index, adj_weight, channels, H * W, PHW, total);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}
