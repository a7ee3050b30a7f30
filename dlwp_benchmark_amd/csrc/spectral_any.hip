// Width-generic spectral path for MI355X (gfx950): SpectralConv2d at any Ci, Co in [1, 512], any H, any W that is a
// multiple of 4, any kept rows / columns; and the FNO2d step built on it at any hidden / lifting / projection width.
// fno2d.hip routes a plan here when its shape is outside the domain of the 32-channel kernels.
//
// One spectral convolution is three launches (pruned DFT, the factorisation of fno_unfused.hpp without its fixed widths):
//   fwd_kernel  one workgroup per (sample, in-channel) plane:
//               W-direction  X1[h][k'] = sum_w x[h][w] tf[w][k']   [H x W] x [W x 2 n_cols] on v_mfma_f32_16x16x4_f32,
//                            x read once as 16-byte vectors, X1 kept in LDS
//               H-direction  Xh[r][ky] = fwd_scale sum_h ef[r][h] X1[h][ky]  at the kept rows only  -> xh [mode][B][Ci]
//   mix_kernel  one workgroup per (mode, 64 out-channels): Z[b][o] = sum_c Xh[b][c] Wt[c][o] (complex), the weights
//               streamed once per call (all samples of a 32-sample chunk share each weight load)       -> z [mode][B][Co]
//   inv_kernel  one workgroup per (sample, out-channel) plane:
//               H-direction  Y1[h][ky] = c_k sum_r ei[r][h] Z[r][ky]  (LDS)
//               W-direction  y[h][w] = sum_k' Y1[h][k'] ti[k'][w]  on v_mfma_f32_16x16x4_f32, y written once
// Arithmetic: fp32 throughout (the MFMA products are exact fp32 FMA chains); there is one form, whatever the plan's
// precision_form / launch_form say.  Padding instead of refusal: H, W and 2 n_cols are rounded up to 16 with zero
// twiddles and masked loads / stores, channel counts need no alignment at all.
//
// The FNO step: lifting (1x1, GELU, 1x1), n_layers x GELU(spectral(h) + bias + skip(h)) (no GELU after the last), and
// projection (1x1, GELU, 1x1) + the residual x_t.  The 1x1 convolutions are pw_kernel: 4 pixels x 8 out-channels
// per thread, the weights on the scalar path, the rollout's input read straight from its channel-segment table and
// the residual / output at their rollout strides.  No launch synchronises the host.
#include "spectral_any.hpp"

namespace dlwp {
namespace sany {

struct Dims {
  int B, ci, co, H, W, nr, nc, Hp, Wp, KPp;
  float fwd;
};

// ---------------------------------------------------------------------------------------------
// spectral convolution kernels
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fwd_kernel(const float* __restrict__ x, const float* __restrict__ tf,
                                                  const float2* __restrict__ ef, float2* __restrict__ xh, const Dims d) {
  extern __shared__ float s_x1[];   // [Hp][KPp + 1]
  const int KS = d.KPp + 1;
  const int plane = blockIdx.x;     // b * ci + c
  const int b = plane / d.ci, c = plane - b * d.ci;
  const float* xp = x + (long long)plane * d.H * d.W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lk = lane >> 4;
  // W-direction.  A operand: lane (li, lk) holds x[h = 16 rt + li][k0 + 4 lk + s] of MFMA step s (one 16-byte load per
  // 16 k), so the B operand of step s is row k0 + 4 lk + s of the table: the k order inside a step is permuted
  // consistently on both sides.
  for (int rt = wave; rt < d.Hp / 16; rt += 4) {
    const int h = 16 * rt + li;
    for (int n0 = 0; n0 < d.KPp; n0 += 64) {
      const int nt = min(4, (d.KPp - n0) / 16);
      f32x4 acc[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < d.W; k0 += 16) {
        const int kk = k0 + 4 * lk;
        f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
        if (h < d.H && kk < d.W) a = *reinterpret_cast<const f32x4*>(xp + (long long)h * d.W + kk);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const float* tr = tf + (long long)(kk + s) * d.KPp + n0 + li;   // kk + s < Wp: padded rows are zero
#pragma unroll
          for (int t = 0; t < 4; ++t)
            if (t < nt) acc[t] = mfma16x16x4(a[s], tr[16 * t], acc[t]);
        }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (t < nt)
#pragma unroll
          for (int v = 0; v < 4; ++v) s_x1[(16 * rt + 4 * lk + v) * KS + n0 + 16 * t + li] = acc[t][v];
    }
  }
  __syncthreads();
  // H-direction at the kept rows
  const int nm = d.nr * d.nc;
  for (int m = threadIdx.x; m < nm; m += 256) {
    const int ky = m / d.nr, r = m - ky * d.nr;
    const float2* e = ef + (long long)r * d.H;
    float re = 0.f, im = 0.f;
    for (int hh = 0; hh < d.H; ++hh) {
      const float xr = s_x1[hh * KS + 2 * ky], xi = s_x1[hh * KS + 2 * ky + 1];
      const float2 w = e[hh];
      re = fmaf(w.x, xr, re);
      re = fmaf(-w.y, xi, re);
      im = fmaf(w.x, xi, im);
      im = fmaf(w.y, xr, im);
    }
    xh[((long long)m * d.B + b) * d.ci + c] = float2{re * d.fwd, im * d.fwd};
  }
}

constexpr int kMixB = 32;   // samples per weight load (8 per thread, 4 wave groups)
constexpr int kMixC = 64;   // in-channels staged per LDS round

__global__ __launch_bounds__(256) void mix_kernel(const float2* __restrict__ xh, const float2* __restrict__ wt,
                                                  float2* __restrict__ z, const Dims d) {
  __shared__ float2 s_a[kMixB][kMixC + 1];
  const int m = blockIdx.y;
  const int o = blockIdx.x * 64 + (threadIdx.x & 63);
  const int bg = threadIdx.x >> 6;   // wave: samples b0 + bg + 4 i
  const float2* wm = wt + (long long)m * d.ci * d.co;
  const float2* am = xh + (long long)m * d.B * d.ci;
  for (int b0 = 0; b0 < d.B; b0 += kMixB) {
    float2 acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = float2{0.f, 0.f};
    for (int c0 = 0; c0 < d.ci; c0 += kMixC) {
      __syncthreads();
      for (int i = threadIdx.x; i < kMixB * kMixC; i += 256) {
        const int bb = i / kMixC, cc = i - bb * kMixC;
        s_a[bb][cc] = (b0 + bb < d.B && c0 + cc < d.ci) ? am[(long long)(b0 + bb) * d.ci + c0 + cc] : float2{0.f, 0.f};
      }
      __syncthreads();
      const int cn = min(kMixC, d.ci - c0);
      for (int cc = 0; cc < cn; ++cc) {
        const float2 w = (o < d.co) ? wm[(long long)(c0 + cc) * d.co + o] : float2{0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float2 a = s_a[bg + 4 * i][cc];
          acc[i].x = fmaf(a.x, w.x, acc[i].x);
          acc[i].x = fmaf(-a.y, w.y, acc[i].x);
          acc[i].y = fmaf(a.x, w.y, acc[i].y);
          acc[i].y = fmaf(a.y, w.x, acc[i].y);
        }
      }
    }
    if (o < d.co)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int b = b0 + bg + 4 * i;
        if (b < d.B) z[((long long)m * d.B + b) * d.co + o] = acc[i];
      }
  }
}

__global__ __launch_bounds__(256) void inv_kernel(const float2* __restrict__ z, const float2* __restrict__ ei,
                                                  const float* __restrict__ ck, const float* __restrict__ ti,
                                                  float* __restrict__ y, const Dims d) {
  extern __shared__ float smem[];
  const int KS = d.KPp + 4;                                   // keeps 16-byte rows for the A loads
  float* s_y1 = smem;                                         // [Hp][KS]
  float2* s_z = reinterpret_cast<float2*>(smem + d.Hp * KS);  // [nm]
  const int plane = blockIdx.x;                               // b * co + o
  const int b = plane / d.co, o = plane - b * d.co;
  const int nm = d.nr * d.nc, half = d.KPp / 2;
  for (int m = threadIdx.x; m < nm; m += 256) s_z[m] = z[((long long)m * d.B + b) * d.co + o];
  __syncthreads();
  // H-direction back to every row; padded rows / columns are zero
  for (int i = threadIdx.x; i < d.Hp * half; i += 256) {
    const int h = i / half, ky = i - h * half;
    float re = 0.f, im = 0.f;
    if (h < d.H && ky < d.nc) {
      for (int r = 0; r < d.nr; ++r) {
        const float2 e = ei[(long long)r * d.H + h];
        const float2 v = s_z[ky * d.nr + r];
        re = fmaf(e.x, v.x, re);
        re = fmaf(-e.y, v.y, re);
        im = fmaf(e.x, v.y, im);
        im = fmaf(e.y, v.x, im);
      }
      re *= ck[ky];
      im *= ck[ky];
    }
    s_y1[h * KS + 2 * ky] = re;
    s_y1[h * KS + 2 * ky + 1] = im;
  }
  __syncthreads();
  // W-direction
  float* yp = y + (long long)plane * d.H * d.W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lk = lane >> 4;
  for (int rt = wave; rt < d.Hp / 16; rt += 4) {
    for (int n0 = 0; n0 < d.Wp; n0 += 64) {
      const int nt = min(4, (d.Wp - n0) / 16);
      f32x4 acc[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < d.KPp; k0 += 16) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(s_y1 + (16 * rt + li) * KS + k0 + 4 * lk);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const float* tr = ti + (long long)(k0 + 4 * lk + s) * d.Wp + n0 + li;
#pragma unroll
          for (int t = 0; t < 4; ++t)
            if (t < nt) acc[t] = mfma16x16x4(a[s], tr[16 * t], acc[t]);
        }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int w = n0 + 16 * t + li;
        if (t < nt && w < d.W)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int h = 16 * rt + 4 * lk + v;
            if (h < d.H) yp[(long long)h * d.W + w] = acc[t][v];
          }
      }
    }
  }
}

// weights [.][.][nr][nc] complex of the forward operator -> [nr * nc][ci][co] (mode m = ky * nr + r);
// adjoint: source [co][ci] (the forward operator of the transposed plan), conjugated
__global__ __launch_bounds__(256) void pack_kernel(const float2* __restrict__ src, float2* __restrict__ dst, int ci, int co,
                                                   int nr, int nc, int adjoint) {
  const long long total = (long long)ci * co * nr * nc;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int o = (int)(i % co);
    const int c = (int)((i / co) % ci);
    const int m = (int)(i / ((long long)co * ci));
    const int ky = m / nr, r = m - ky * nr;
    if (adjoint) {
      const float2 v = src[(((long long)o * ci + c) * nr + r) * nc + ky];
      dst[i] = float2{v.x, -v.y};
    } else {
      dst[i] = src[(((long long)c * co + o) * nr + r) * nc + ky];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// weight gradient: G[i][o][r][k] = ck[k] sum_b conj(Xh[m][b][i]) DYh[m][b][o], m = k * nr + r
// ---------------------------------------------------------------------------------------------
// Xh (fwd_scale folded in by fwd_kernel) and DYh are the kept spectra of x and grad_y in the [mode][B][C] layout the
// forward uses.  Each output is one thread's fp32 FMA chain over b in index order: no atomics, bitwise repeatable.
// One workgroup per (mode, 64 out-channels, 32 in-channels) writes the packed image G [mode][Ci][Co] coalesced along o;
// unpack_kernel (the inverse of pack_kernel, through a 64-mode x 32-pair LDS tile) turns it into PyTorch layout, where
// the mode axes are innermost.  (A direct form -- lanes along the modes, a 4 x 8 tile of (i, o) pairs per thread, 512
// contiguous bytes per wave store and no packed image -- was measured and lost: DESIGN.md section 19.)
__global__ __launch_bounds__(256) void wgrad_kernel(const float2* __restrict__ xh, const float2* __restrict__ dyh,
                                                           const float* __restrict__ ck, float2* __restrict__ g,
                                                           const Dims d) {
  __shared__ float2 s_x[kMixB][33];
  const int m = blockIdx.y;
  const int o = blockIdx.x * 64 + (threadIdx.x & 63);
  const int i0 = blockIdx.z * 32, ig = threadIdx.x >> 6;   // wave: in-channels i0 + ig + 4 j
  const float2* xa = xh + (long long)m * d.B * d.ci;
  const float2* da = dyh + (long long)m * d.B * d.co;
  float2 acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = float2{0.f, 0.f};
  for (int b0 = 0; b0 < d.B; b0 += kMixB) {
    __syncthreads();
    for (int i = threadIdx.x; i < kMixB * 32; i += 256) {
      const int bb = i >> 5, cc = i & 31;
      s_x[bb][cc] = (b0 + bb < d.B && i0 + cc < d.ci) ? xa[(long long)(b0 + bb) * d.ci + i0 + cc] : float2{0.f, 0.f};
    }
    __syncthreads();
    const int bn = min(kMixB, d.B - b0);
    for (int bb = 0; bb < bn; ++bb) {
      const float2 dv = (o < d.co) ? da[(long long)(b0 + bb) * d.co + o] : float2{0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float2 xv = s_x[bb][ig + 4 * j];
        acc[j].x = fmaf(xv.x, dv.x, acc[j].x);
        acc[j].x = fmaf(xv.y, dv.y, acc[j].x);
        acc[j].y = fmaf(xv.x, dv.y, acc[j].y);
        acc[j].y = fmaf(-xv.y, dv.x, acc[j].y);
      }
    }
  }
  const float sc = ck[m / d.nr];
  if (o < d.co)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = i0 + ig + 4 * j;
      if (i < d.ci) g[((long long)m * d.ci + i) * d.co + o] = float2{acc[j].x * sc, acc[j].y * sc};
    }
}

__global__ __launch_bounds__(256) void unpack_kernel(const float2* __restrict__ src, float2* __restrict__ dst, int npair,
                                                     int nr, int nc) {
  __shared__ float2 s_t[64][33];
  const int nm = nr * nc;
  const int mp0 = blockIdx.x * 64, q0 = blockIdx.y * 32;
  for (int i = threadIdx.x; i < 64 * 32; i += 256) {
    const int mm = i >> 5, q = i & 31, mp = mp0 + mm;
    if (mp < nm && q0 + q < npair) {
      const int r = mp / nc, ky = mp - r * nc;
      s_t[mm][q] = src[((long long)ky * nr + r) * npair + q0 + q];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * 32; i += 256) {
    const int q = i >> 6, mm = i & 63;
    if (mp0 + mm < nm && q0 + q < npair) dst[(long long)(q0 + q) * nm + mp0 + mm] = s_t[mm][q];
  }
}

// ---------------------------------------------------------------------------------------------
// 1x1 convolution: y[b][o][p] = act(bias[o] + sum_c w[o][c] x[b][c][p] + resid[b][o][p])
// ---------------------------------------------------------------------------------------------
struct PwArgs {
  const float* xp[4];   // input channel segments (concatenated in order)
  long long xbs[4];     // their batch strides (floats)
  int xc[4];            // their channel counts
  int nseg;
  const float* w;       // [cout][cin]
  const float* bias;    // [cout] or null
  const float* resid;   // [B][cout][HW] at batch stride rbs, or null
  long long rbs;
  float* y;             // [B][cout][HW] at batch stride ybs
  long long ybs;
  int cin, cout, HW4, act;
};

template <int OT>
__global__ __launch_bounds__(256) void pw_kernel(const PwArgs p) {
  const int q = blockIdx.x * 256 + threadIdx.x;   // pixel quad
  const int o0 = blockIdx.y * OT, b = blockIdx.z;
  if (q >= p.HW4) return;
  const long long HW = 4LL * p.HW4;
  f32x4 acc[OT];
#pragma unroll
  for (int j = 0; j < OT; ++j) {
    const float bv = (p.bias && o0 + j < p.cout) ? p.bias[o0 + j] : 0.f;
    acc[j] = f32x4{bv, bv, bv, bv};
  }
  int c = 0;
  for (int sg = 0; sg < p.nseg; ++sg) {
    const float* xs = p.xp[sg] + (long long)b * p.xbs[sg] + 4LL * q;
    for (int cs = 0; cs < p.xc[sg]; ++cs, ++c) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(xs + cs * HW);
#pragma unroll
      for (int j = 0; j < OT; ++j) {
        const float wv = (o0 + j < p.cout) ? p.w[(long long)(o0 + j) * p.cin + c] : 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[j][e] = fmaf(xv[e], wv, acc[j][e]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < OT; ++j) {
    if (o0 + j >= p.cout) break;
    f32x4 v = acc[j];
    if (p.resid) {
      const f32x4 r = *reinterpret_cast<const f32x4*>(p.resid + (long long)b * p.rbs + (o0 + j) * HW + 4LL * q);
      v += r;
    }
    if (p.act)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = gelu_erf(v[e]);
    *reinterpret_cast<f32x4*>(p.y + (long long)b * p.ybs + (o0 + j) * HW + 4LL * q) = v;
  }
}

// ---------------------------------------------------------------------------------------------
// host side: spectral convolution
// ---------------------------------------------------------------------------------------------
static inline int round16(int v) { return (v + 15) / 16 * 16; }

template <class K>
static hipError_t allow_lds(K kernel, size_t bytes) {
  // one bound for every plan: a later plan with a smaller image must not lower the limit an earlier plan relies on
  if (bytes <= 48 * 1024) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)kMaxLdsBytes);
}

static Dims dims(const Geom& g, int B) {
  Dims d;
  d.B = B; d.ci = g.ci; d.co = g.co; d.H = g.H; d.W = g.W; d.nr = g.nr; d.nc = g.nc;
  d.Hp = g.Hp; d.Wp = g.Wp; d.KPp = g.KPp; d.fwd = g.fwd;
  return d;
}

int32_t geom_build(Geom& g, int ci, int co, int H, int W, int nr, int nc, const int32_t* rows_in,
                   const int32_t* rows_out, float fwd_scale, float inv_scale, hipStream_t s) {
  DLWP_REQUIRE(ci >= 1 && ci <= kMaxChannels && co >= 1 && co <= kMaxChannels, DLWP_ERR_UNSUPPORTED,
               "spectral convolution %d -> %d channels: the generic kernels take 1 .. %d", ci, co, kMaxChannels);
  DLWP_REQUIRE(H >= 1 && W >= 4 && W % 4 == 0, DLWP_ERR_UNSUPPORTED,
               "grid %d x %d: the width must be a positive multiple of 4", H, W);
  DLWP_REQUIRE(nr >= 1 && nr <= H && nc >= 1 && nc <= W / 2 + 1, DLWP_ERR_INVALID_ARGUMENT, "bad mode counts");
  for (int r = 0; r < nr; ++r)
    DLWP_REQUIRE(rows_in[r] >= 0 && rows_in[r] < H && rows_out[r] >= 0 && rows_out[r] < H, DLWP_ERR_INVALID_ARGUMENT,
                 "kept row %d outside [0, %d)", r, H);
  g.ci = ci; g.co = co; g.H = H; g.W = W; g.nr = nr; g.nc = nc;
  g.Hp = round16(H); g.Wp = round16(W); g.KPp = round16(2 * nc);
  g.fwd = fwd_scale;
  g.rows_o.assign(rows_out, rows_out + nr);
  DLWP_REQUIRE(g.fwd_lds() <= kMaxLdsBytes && g.inv_lds() <= kMaxLdsBytes, DLWP_ERR_UNSUPPORTED,
               "grid height %d x %d kept columns: the per-plane transform image (%zu bytes) exceeds %zu bytes of LDS", H,
               nc, g.inv_lds() > g.fwd_lds() ? g.inv_lds() : g.fwd_lds(), kMaxLdsBytes);
  const double two_pi = 6.283185307179586476925286766559;
  std::vector<float> htf((size_t)g.Wp * g.KPp, 0.f), hti((size_t)g.KPp * g.Wp, 0.f);
  for (int ky = 0; ky < nc; ++ky)
    for (int w = 0; w < W; ++w) {
      const long long m = ((long long)ky * w) % W;
      const double a = two_pi * (double)m / (double)W;
      const float cs = (float)std::cos(a), sn = (float)(-std::sin(a));
      htf[(size_t)w * g.KPp + 2 * ky] = cs;
      htf[(size_t)w * g.KPp + 2 * ky + 1] = sn;
      hti[(size_t)(2 * ky) * g.Wp + w] = cs;
      hti[(size_t)(2 * ky + 1) * g.Wp + w] = sn;
    }
  std::vector<float> hef((size_t)nr * H * 2), hei((size_t)nr * H * 2), hck(nc);
  for (int r = 0; r < nr; ++r)
    for (int h = 0; h < H; ++h) {
      const long long mi = ((long long)rows_in[r] * h) % H, mo = ((long long)rows_out[r] * h) % H;
      const double ai = two_pi * (double)mi / (double)H, ao = two_pi * (double)mo / (double)H;
      hef[((size_t)r * H + h) * 2 + 0] = (float)std::cos(ai);
      hef[((size_t)r * H + h) * 2 + 1] = (float)(-std::sin(ai));
      hei[((size_t)r * H + h) * 2 + 0] = (float)std::cos(ao);
      hei[((size_t)r * H + h) * 2 + 1] = (float)std::sin(ao);
    }
  for (int ky = 0; ky < nc; ++ky) {
    const bool self_conj = (ky == 0) || (W % 2 == 0 && ky == W / 2);
    hck[ky] = (self_conj ? 1.f : 2.f) * inv_scale;
  }
  DLWP_HIP_CHECK(g.tf.upload(htf.data(), htf.size() * 4, s));
  DLWP_HIP_CHECK(g.ti.upload(hti.data(), hti.size() * 4, s));
  DLWP_HIP_CHECK(g.ef.upload(hef.data(), hef.size() * 4, s));
  DLWP_HIP_CHECK(g.ei.upload(hei.data(), hei.size() * 4, s));
  DLWP_HIP_CHECK(g.ck.upload(hck.data(), hck.size() * 4, s));
  DLWP_HIP_CHECK(hipStreamSynchronize(s));   // host staging vectors die at scope exit
  DLWP_HIP_CHECK(allow_lds(fwd_kernel, g.fwd_lds()));
  DLWP_HIP_CHECK(allow_lds(inv_kernel, g.inv_lds()));
  return DLWP_OK;
}

void pack_host(std::vector<float>& dst, const Geom& g, const float* w, int nr_blk, int row_off) {
  dst.resize((size_t)g.nr * g.nc * g.ci * g.co * 2, 0.f);
  for (int c = 0; c < g.ci; ++c)
    for (int o = 0; o < g.co; ++o)
      for (int r = 0; r < nr_blk; ++r)
        for (int ky = 0; ky < g.nc; ++ky) {
          const size_t src = ((((size_t)c * g.co + o) * nr_blk + r) * g.nc + ky) * 2;
          const size_t m = (size_t)ky * g.nr + r + row_off;
          const size_t d = ((m * g.ci + c) * g.co + o) * 2;
          dst[d] = w[src];
          dst[d + 1] = w[src + 1];
        }
}

int32_t pack_dev(const Geom& g, const float* w_dev, int adjoint, float2* wt, hipStream_t s) {
  const long long total = (long long)g.ci * g.co * g.nr * g.nc;
  long long blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(pack_kernel, dim3((unsigned)blocks), dim3(256), 0, s, reinterpret_cast<const float2*>(w_dev), wt,
                     g.ci, g.co, g.nr, g.nc, adjoint ? 1 : 0);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

static size_t xh_bytes(const Geom& g, int B) { return align_up((size_t)g.nr * g.nc * B * g.ci * sizeof(float2), 256); }
static size_t z_bytes(const Geom& g, int B) { return align_up((size_t)g.nr * g.nc * B * g.co * sizeof(float2), 256); }

size_t workspace_bytes(const Geom& g, int B) { return xh_bytes(g, B) + z_bytes(g, B); }

int32_t run_fwd_mix(const Geom& g, const float2* wt, const float* x, int B, void* ws, hipStream_t s) {
  const Dims d = dims(g, B);
  float2* xh = reinterpret_cast<float2*>(ws);
  float2* z = reinterpret_cast<float2*>(reinterpret_cast<char*>(ws) + xh_bytes(g, B));
  hipLaunchKernelGGL(fwd_kernel, dim3(B * g.ci), dim3(256), g.fwd_lds(), s, x, g.tf.as<float>(), g.ef.as<float2>(), xh, d);
  DLWP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(mix_kernel, dim3((g.co + 63) / 64, g.nr * g.nc), dim3(256), 0, s, xh, wt, z, d);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

int32_t run_inv(const Geom& g, float* y, int B, void* ws, hipStream_t s) {
  const Dims d = dims(g, B);
  const float2* z = reinterpret_cast<const float2*>(reinterpret_cast<char*>(ws) + xh_bytes(g, B));
  hipLaunchKernelGGL(inv_kernel, dim3(B * g.co), dim3(256), g.inv_lds(), s, z, g.ei.as<float2>(), g.ck.as<float>(),
                     g.ti.as<float>(), y, d);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

int32_t wgrad_prepare(Geom& g, hipStream_t s) {
  if (g.efo.p) return DLWP_OK;
  const double two_pi = 6.283185307179586476925286766559;
  std::vector<float> h((size_t)g.nr * g.H * 2);
  for (int r = 0; r < g.nr; ++r)
    for (int hh = 0; hh < g.H; ++hh) {
      const double a = two_pi * (double)(((long long)g.rows_o[r] * hh) % g.H) / (double)g.H;
      h[((size_t)r * g.H + hh) * 2 + 0] = (float)std::cos(a);
      h[((size_t)r * g.H + hh) * 2 + 1] = (float)(-std::sin(a));
    }
  DLWP_HIP_CHECK(g.efo.upload(h.data(), h.size() * 4, s));
  DLWP_HIP_CHECK(hipStreamSynchronize(s));   // the staging vector dies at scope exit
  return DLWP_OK;
}

size_t wgrad_workspace_bytes(const Geom& g, int B) {
  return xh_bytes(g, B) + z_bytes(g, B) + align_up((size_t)g.nr * g.nc * g.ci * g.co * sizeof(float2), 256);
}

int32_t run_wgrad(const Geom& g, const float* x, const float* grad_y, float* grad_w, int B, void* ws, hipStream_t s) {
  DLWP_REQUIRE(g.efo.p, DLWP_ERR_INVALID_ARGUMENT, "weight gradient before wgrad_prepare");
  const Dims dx = dims(g, B);
  Dims dy = dx;   // grad_y planes: Co channels, no forward scale (ck carries inv_scale)
  dy.ci = g.co; dy.fwd = 1.f;
  float2* xh = reinterpret_cast<float2*>(ws);
  float2* dyh = reinterpret_cast<float2*>(reinterpret_cast<char*>(ws) + xh_bytes(g, B));
  float2* gp = reinterpret_cast<float2*>(reinterpret_cast<char*>(ws) + xh_bytes(g, B) + z_bytes(g, B));
  hipLaunchKernelGGL(fwd_kernel, dim3(B * g.ci), dim3(256), g.fwd_lds(), s, x, g.tf.as<float>(), g.ef.as<float2>(), xh, dx);
  DLWP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(fwd_kernel, dim3(B * g.co), dim3(256), g.fwd_lds(), s, grad_y, g.tf.as<float>(), g.efo.as<float2>(),
                     dyh, dy);
  DLWP_HIP_CHECK(hipGetLastError());
  const int nm = g.nr * g.nc;
  hipLaunchKernelGGL(wgrad_kernel, dim3((g.co + 63) / 64, nm, (g.ci + 31) / 32), dim3(256), 0, s, xh, dyh, g.ck.as<float>(),
                     gp, dx);
  DLWP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(unpack_kernel, dim3((nm + 63) / 64, (g.ci * g.co + 31) / 32), dim3(256), 0, s, gp,
                     reinterpret_cast<float2*>(grad_w), g.ci * g.co, g.nr, g.nc);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

// ---------------------------------------------------------------------------------------------
// host side: FNO2d
// ---------------------------------------------------------------------------------------------
struct Fno {
  int cin = 0, hid = 0, hid_l = 0, hid_p = 0, cout = 0, L = 0, H = 0, W = 0;
  Geom g;
  DevBuf lw1, lb1, lw2, lb2, pw1, pb1, pw2, pb2, sb;   // sb: [L][hid] spectral biases
  std::vector<DevBuf> wt, skip;                        // per layer: packed spectral weights, skip [hid][hid]
};

int32_t fno_create(Fno** out, const dlwp_fno2d_desc* d, hipStream_t s) {
  *out = nullptr;
  auto in_range = [](int v) { return v >= 1 && v <= kMaxChannels; };
  DLWP_REQUIRE(in_range(d->hidden_channels), DLWP_ERR_UNSUPPORTED, "hidden_channels %d not in [1, %d]", d->hidden_channels,
               kMaxChannels);
  DLWP_REQUIRE(in_range(d->lifting_channels) && in_range(d->projection_channels), DLWP_ERR_UNSUPPORTED,
               "lifting / projection channels %d / %d not in [1, %d]", d->lifting_channels, d->projection_channels,
               kMaxChannels);
  DLWP_REQUIRE(in_range(d->in_channels), DLWP_ERR_UNSUPPORTED, "in_channels %d not in [1, %d]", d->in_channels, kMaxChannels);
  DLWP_REQUIRE(in_range(d->out_channels), DLWP_ERR_UNSUPPORTED, "out_channels %d not in [1, %d]", d->out_channels,
               kMaxChannels);
  DLWP_REQUIRE(d->width > 0 && d->width % 64 == 0 && d->height > 0, DLWP_ERR_UNSUPPORTED,
               "width %d must be a positive multiple of 64", d->width);
  DLWP_REQUIRE(d->n_layers >= 1 && d->n_rows >= 1 && d->n_cols >= 1, DLWP_ERR_INVALID_ARGUMENT, "bad layer/mode count");
  DLWP_REQUIRE(d->lift_w1 && d->lift_b1 && d->lift_w2 && d->lift_b2 && d->spec_w && d->spec_b && d->skip_w &&
                   d->proj_w1 && d->proj_b1 && d->proj_w2 && d->proj_b2 && d->rows_in && d->rows_out,
               DLWP_ERR_INVALID_ARGUMENT, "null weight pointer");
  DLWP_REQUIRE(d->precision_form >= 0 && d->precision_form <= 2, DLWP_ERR_INVALID_ARGUMENT, "precision_form %d not in {0, 1, 2}",
               d->precision_form);
  DLWP_REQUIRE(d->on_timeout == 0 || d->on_timeout == 1, DLWP_ERR_INVALID_ARGUMENT, "on_timeout %d not in {0, 1}", d->on_timeout);
  DLWP_REQUIRE(d->debug_spin_limit >= 0, DLWP_ERR_INVALID_ARGUMENT, "debug_spin_limit must be >= 0");
  for (int l = 0; l < d->n_layers; ++l)
    DLWP_REQUIRE(d->spec_w[l] && d->skip_w[l], DLWP_ERR_INVALID_ARGUMENT, "null weight pointer (layer %d)", l);
  auto* p = new Fno();
  p->cin = d->in_channels; p->hid = d->hidden_channels; p->hid_l = d->lifting_channels; p->hid_p = d->projection_channels;
  p->cout = d->out_channels; p->L = d->n_layers; p->H = d->height; p->W = d->width;
  int32_t rc = geom_build(p->g, p->hid, p->hid, d->height, d->width, d->n_rows, d->n_cols, d->rows_in, d->rows_out,
                          d->fwd_scale, d->inv_scale, s);
  if (rc != DLWP_OK) { delete p; return rc; }
  const size_t hid = (size_t)p->hid;
  hipError_t e = hipSuccess;
  std::vector<float> tmp;
  do {
    if ((e = p->lw1.upload(d->lift_w1, (size_t)p->hid_l * p->cin * 4, s)) != hipSuccess) break;
    if ((e = p->lb1.upload(d->lift_b1, (size_t)p->hid_l * 4, s)) != hipSuccess) break;
    if ((e = p->lw2.upload(d->lift_w2, hid * p->hid_l * 4, s)) != hipSuccess) break;
    if ((e = p->lb2.upload(d->lift_b2, hid * 4, s)) != hipSuccess) break;
    if ((e = p->pw1.upload(d->proj_w1, (size_t)p->hid_p * hid * 4, s)) != hipSuccess) break;
    if ((e = p->pb1.upload(d->proj_b1, (size_t)p->hid_p * 4, s)) != hipSuccess) break;
    if ((e = p->pw2.upload(d->proj_w2, (size_t)p->cout * p->hid_p * 4, s)) != hipSuccess) break;
    if ((e = p->pb2.upload(d->proj_b2, (size_t)p->cout * 4, s)) != hipSuccess) break;
    if ((e = p->sb.upload(d->spec_b, (size_t)p->L * hid * 4, s)) != hipSuccess) break;
    p->wt.resize(p->L);
    p->skip.resize(p->L);
    for (int l = 0; l < p->L && e == hipSuccess; ++l) {
      pack_host(tmp, p->g, d->spec_w[l], d->n_rows, 0);
      if ((e = p->wt[l].upload(tmp.data(), tmp.size() * 4, s)) != hipSuccess) break;
      if ((e = hipStreamSynchronize(s)) != hipSuccess) break;   // tmp is reused by the next layer
      e = p->skip[l].upload(d->skip_w[l], hid * hid * 4, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
  } while (0);
  if (e != hipSuccess) {
    delete p;
    return fail(DLWP_ERR_HIP, "plan upload failed: %s", hipGetErrorString(e));
  }
  *out = p;
  return DLWP_OK;
}

void fno_destroy(Fno* p) { delete p; }

namespace {
struct Ws {
  float *h0, *h1, *sp, *mid;   // activations [B][hid][HW] x 3, MLP hidden [B][max(lifting, projection)][HW]
  void* spec;                  // spectral workspace
  size_t total;
};
Ws carve(const Fno* p, int B, void* base) {
  const size_t HW = (size_t)p->H * p->W;
  const size_t act = align_up((size_t)B * p->hid * HW * 4, 256);
  const size_t mid = align_up((size_t)B * (p->hid_l > p->hid_p ? p->hid_l : p->hid_p) * HW * 4, 256);
  char* c = reinterpret_cast<char*>(base);
  Ws w;
  w.h0 = reinterpret_cast<float*>(c);
  w.h1 = reinterpret_cast<float*>(c + act);
  w.sp = reinterpret_cast<float*>(c + 2 * act);
  w.mid = reinterpret_cast<float*>(c + 3 * act);
  w.spec = c + 3 * act + mid;
  w.total = 3 * act + mid + workspace_bytes(p->g, B);
  return w;
}

// event brackets per kernel class (dlwp_fno2d_rollout_profiled_f32): 0 lifting, 1 forward transform + mode mix,
// 2 inverse transform + layer epilogue, 3 projection, 4 an empty bracket per step
struct Timer {
  std::vector<hipEvent_t> ev[5];
  hipStream_t s = nullptr;
  hipError_t mark(int cls) {
    hipEvent_t e;
    hipError_t rc = hipEventCreate(&e);
    if (rc != hipSuccess) return rc;
    ev[cls].push_back(e);
    return hipEventRecord(e, s);
  }
  ~Timer() {
    for (auto& v : ev)
      for (auto e : v) (void)hipEventDestroy(e);
  }
};

struct Segs {
  const float* ptr[4];
  long long bs[4];
  int ch[4];
  int n;
};

int32_t pw(const Fno* p, const Segs& x, const float* w, const float* bias, int cin, int cout, const float* resid,
           long long rbs, float* y, long long ybs, int act, int B, hipStream_t s) {
  PwArgs a;
  for (int i = 0; i < 4; ++i) {
    a.xp[i] = i < x.n ? x.ptr[i] : nullptr;
    a.xbs[i] = i < x.n ? x.bs[i] : 0;
    a.xc[i] = i < x.n ? x.ch[i] : 0;
  }
  a.nseg = x.n;
  a.w = w; a.bias = bias; a.resid = resid; a.rbs = rbs; a.y = y; a.ybs = ybs;
  a.cin = cin; a.cout = cout; a.HW4 = p->H * p->W / 4; a.act = act;
  const unsigned gx = (unsigned)((a.HW4 + 255) / 256);
  if (cout >= 8) hipLaunchKernelGGL(pw_kernel<8>, dim3(gx, (cout + 7) / 8, B), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(pw_kernel<4>, dim3(gx, (cout + 3) / 4, B), dim3(256), 0, s, a);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

Segs one_seg(const float* ptr, long long bs, int ch) {
  Segs x;
  x.ptr[0] = ptr; x.bs[0] = bs; x.ch[0] = ch; x.n = 1;
  return x;
}

// one backbone step: x_t (segment table) -> out (+ resid), out / resid at their batch strides
int32_t step(const Fno* p, const Segs& xt, int B, const Ws& ws, float* out, long long out_bs, const float* resid,
             long long resid_bs, hipStream_t s, Timer* tm) {
  const long long HW = (long long)p->H * p->W;
  const long long act_bs = (long long)p->hid * HW;
#define DLWP_MARK(cls) do { if (tm) DLWP_HIP_CHECK(tm->mark(cls)); } while (0)
  DLWP_MARK(4);
  DLWP_MARK(4);
  DLWP_MARK(0);
  int32_t rc = pw(p, xt, p->lw1.as<float>(), p->lb1.as<float>(), p->cin, p->hid_l, nullptr, 0, ws.mid, (long long)p->hid_l * HW,
                  1, B, s);
  if (rc != DLWP_OK) return rc;
  rc = pw(p, one_seg(ws.mid, (long long)p->hid_l * HW, p->hid_l), p->lw2.as<float>(), p->lb2.as<float>(), p->hid_l, p->hid,
          nullptr, 0, ws.h0, act_bs, 0, B, s);
  if (rc != DLWP_OK) return rc;
  DLWP_MARK(0);
  float* hin = ws.h0;
  float* hout = ws.h1;
  for (int l = 0; l < p->L; ++l) {
    DLWP_MARK(1);
    rc = run_fwd_mix(p->g, p->wt[l].as<float2>(), hin, B, ws.spec, s);
    if (rc != DLWP_OK) return rc;
    DLWP_MARK(1);
    DLWP_MARK(2);
    rc = run_inv(p->g, ws.sp, B, ws.spec, s);
    if (rc != DLWP_OK) return rc;
    // neuralop FNOBlocks.forward_with_postactivation: GELU after every layer but the last
    rc = pw(p, one_seg(hin, act_bs, p->hid), p->skip[l].as<float>(), p->sb.as<float>() + (size_t)l * p->hid, p->hid, p->hid,
            ws.sp, act_bs, hout, act_bs, l < p->L - 1 ? 1 : 0, B, s);
    if (rc != DLWP_OK) return rc;
    DLWP_MARK(2);
    float* t = hin; hin = hout; hout = t;
  }
  DLWP_MARK(3);
  rc = pw(p, one_seg(hin, act_bs, p->hid), p->pw1.as<float>(), p->pb1.as<float>(), p->hid, p->hid_p, nullptr, 0, ws.mid,
          (long long)p->hid_p * HW, 1, B, s);
  if (rc != DLWP_OK) return rc;
  rc = pw(p, one_seg(ws.mid, (long long)p->hid_p * HW, p->hid_p), p->pw2.as<float>(), p->pb2.as<float>(), p->hid_p, p->cout,
          resid, resid_bs, out, out_bs, 0, B, s);
  if (rc != DLWP_OK) return rc;
  DLWP_MARK(3);
#undef DLWP_MARK
  return DLWP_OK;
}
}  // namespace

size_t fno_workspace_bytes(const Fno* p, int B) { return carve(p, B, nullptr).total; }

int32_t fno_forward(const Fno* p, const float* x, float* y, int B, void* ws_base, size_t ws_bytes, hipStream_t s) {
  DLWP_REQUIRE(x && y && ws_base, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(B > 0, DLWP_ERR_INVALID_ARGUMENT, "batch must be positive");
  DLWP_REQUIRE(B <= 65535, DLWP_ERR_UNSUPPORTED, "batch %d > 65535", B);
  const Ws ws = carve(p, B, ws_base);
  DLWP_REQUIRE(ws_bytes >= ws.total, DLWP_ERR_WORKSPACE, "workspace %zu < required %zu", ws_bytes, ws.total);
  DLWP_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(ws_base) & 255) == 0,
               DLWP_ERR_INVALID_ARGUMENT, "pointers must be 16-byte (workspace 256-byte) aligned");
  const long long HW = (long long)p->H * p->W;
  return step(p, one_seg(x, p->cin * HW, p->cin), B, ws, y, p->cout * HW, nullptr, 0, s, nullptr);
}

int32_t fno_rollout(const Fno* p, const float* constants, int32_t n_const, const float* prescribed, int32_t n_presc,
                    const float* prognostic, int32_t n_prog, int32_t batch, int32_t n_time, int32_t context, float* out,
                    void* ws_base, size_t ws_bytes, hipStream_t s, int32_t step_begin, int32_t step_end, double* class_ms,
                    int32_t* class_launches) {
  DLWP_REQUIRE(prognostic && out && ws_base, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(batch > 0 && context >= 1 && n_time > context, DLWP_ERR_INVALID_ARGUMENT,
               "need batch > 0, context >= 1, n_time > context (got %d, %d, %d)", batch, context, n_time);
  DLWP_REQUIRE(batch <= 65535, DLWP_ERR_UNSUPPORTED, "batch %d > 65535", batch);
  if (!constants) n_const = 0;
  if (!prescribed) n_presc = 0;
  DLWP_REQUIRE(n_const >= 0 && n_presc >= 0 && n_prog == p->cout, DLWP_ERR_INVALID_ARGUMENT,
               "prognostic channels %d != plan out_channels %d", n_prog, p->cout);
  DLWP_REQUIRE(n_const + (n_presc + n_prog) * context == p->cin, DLWP_ERR_INVALID_ARGUMENT,
               "channel count %d + (%d + %d) * %d != plan in_channels %d", n_const, n_presc, n_prog, context, p->cin);
  const Ws ws = carve(p, batch, ws_base);
  DLWP_REQUIRE(ws_bytes >= ws.total, DLWP_ERR_WORKSPACE, "workspace %zu < required %zu", ws_bytes, ws.total);
  DLWP_REQUIRE((reinterpret_cast<uintptr_t>(prognostic) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(constants) & 15) == 0 && (reinterpret_cast<uintptr_t>(prescribed) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(ws_base) & 255) == 0,
               DLWP_ERR_INVALID_ARGUMENT, "pointers must be 16-byte (workspace 256-byte) aligned");
  const long long HW = (long long)p->H * p->W;
  const int T = n_time, ctx = context, To = T - ctx;
  const long long prog_bs = (long long)T * n_prog * HW, out_bs = (long long)To * n_prog * HW;
  if (step_end < 0) step_end = To;
  DLWP_REQUIRE(step_begin >= 0 && step_begin <= step_end && step_end <= To, DLWP_ERR_INVALID_ARGUMENT,
               "step range [%d, %d) outside [0, %d]", step_begin, step_end, To);
  Timer timer;
  timer.s = s;
  Timer* tm = class_ms ? &timer : nullptr;
  for (int t = ctx + step_begin; t < ctx + step_end; ++t) {
    // x_t = cat(constants[:,0], prescribed[:, t-ctx:t], prognostic window)   (fno.py:49-62, :79-100)
    // prognostic window, frame f in [t-ctx, t): input frame f if f < ctx else out[:, f-ctx]
    Segs xt;
    xt.n = 0;
    if (n_const) { xt.ptr[xt.n] = constants; xt.bs[xt.n] = (long long)n_const * HW; xt.ch[xt.n++] = n_const; }
    if (n_presc) {
      xt.ptr[xt.n] = prescribed + (long long)(t - ctx) * n_presc * HW;
      xt.bs[xt.n] = (long long)T * n_presc * HW;
      xt.ch[xt.n++] = n_presc * ctx;
    }
    const int f0 = t - ctx;
    const int n_in = f0 < ctx ? ctx - f0 : 0;   // frames still taken from the input
    if (n_in > 0) { xt.ptr[xt.n] = prognostic + (long long)f0 * n_prog * HW; xt.bs[xt.n] = prog_bs; xt.ch[xt.n++] = n_prog * n_in; }
    if (ctx - n_in > 0) {
      xt.ptr[xt.n] = out + (long long)(f0 + n_in - ctx) * n_prog * HW;
      xt.bs[xt.n] = out_bs;
      xt.ch[xt.n++] = n_prog * (ctx - n_in);
    }
    // residual = last frame of the window (fno.py:103: prognostic_t[:, -1])
    const float* resid;
    long long resid_bs;
    if (t - 1 < ctx) { resid = prognostic + (long long)(t - 1) * n_prog * HW; resid_bs = prog_bs; }
    else { resid = out + (long long)(t - 1 - ctx) * n_prog * HW; resid_bs = out_bs; }
    const int32_t rc = step(p, xt, batch, ws, out + (long long)(t - ctx) * n_prog * HW, out_bs, resid, resid_bs, s, tm);
    if (rc != DLWP_OK) return rc;
  }
  if (tm) {
    DLWP_HIP_CHECK(hipStreamSynchronize(s));
    for (int c = 0; c < 5; ++c) {
      double tot = 0.0;
      const size_t n = timer.ev[c].size() / 2;
      for (size_t i = 0; i < n; ++i) {
        float ms = 0.f;
        DLWP_HIP_CHECK(hipEventElapsedTime(&ms, timer.ev[c][2 * i], timer.ev[c][2 * i + 1]));
        tot += ms;
      }
      class_ms[c] = tot;
      class_launches[c] = (int32_t)n;
    }
  }
  return DLWP_OK;
}

}  // namespace sany
}  // namespace dlwp
