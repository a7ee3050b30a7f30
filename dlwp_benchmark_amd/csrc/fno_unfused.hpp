// FNO2d / SpectralConv2d, one kernel per stage: lifting MLP, per layer modes_kernel (Y -> Z) then layer_kernel
// (x, Z -> y, Y_next), projection MLP (fno2d.hip has the design note).  These are the kernels of launch forms 2 and 3, of
// the fp32_mfma precision form, of the re-run after a fused launch timed out or left the f16 range, and of SpectralConv2d.
// Every kernel here is launched from this file; the orchestration in fno2d.hip calls the host functions at the end
// (declared in fno_plan.hpp).  A part of the translation unit fno_kernels.hip (see there), included nowhere else.
#pragma once
#include "fno_plan.hpp"

namespace dlwp {
namespace fno {

template <int CIN_STEPS, int COUT_TILES, int KP, bool EMIT_Y, bool RESID>
__global__ __launch_bounds__(256) void pw_mlp2_kernel(const MlpParams p) {
  extern __shared__ __align__(16) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int ntile = p.hid >> 4;
  float* s_w1 = smem;
  float* s_b1 = s_w1 + ntile * CIN_STEPS * 64;
  float* s_w2 = s_b1 + p.hid;
  float* s_tr = s_w2 + ntile * 4 * COUT_TILES * 64 + wave * (COUT_TILES * 16 * kTrStride);
  {
    const int n1 = ntile * CIN_STEPS * 64, n2 = ntile * 4 * COUT_TILES * 64;
    for (int i = tid; i < n1; i += blockDim.x) s_w1[i] = p.w1p[i];
    for (int i = tid; i < p.hid; i += blockDim.x) s_b1[i] = p.b1[i];
    for (int i = tid * 4; i < n2; i += blockDim.x * 4)
      *reinterpret_cast<f32x4*>(s_w2 + i) = *reinterpret_cast<const f32x4*>(p.w2p + i);
  }
  __syncthreads();

  const int HW = p.H * p.W;
  const int segs = p.W >> 6;
  const int nrow = p.B * p.H;
  f32x4 bias2[COUT_TILES];
#pragma unroll
  for (int ot = 0; ot < COUT_TILES; ++ot) bias2[ot] = *reinterpret_cast<const f32x4*>(p.b2 + 16 * ot + 4 * g);

  for (int row = blockIdx.x * nw + wave; row < nrow; row += gridDim.x * nw) {
    const int h = row % p.H, b = row / p.H;
    f32x4 yacc[COUT_TILES][KP / 16];
    if (EMIT_Y) {
#pragma unroll
      for (int ot = 0; ot < COUT_TILES; ++ot)
#pragma unroll
        for (int kt = 0; kt < KP / 16; ++kt) yacc[ot][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int ws = 0; ws < segs; ++ws) {
      const int w0 = ws * 64;
      const long long pix = (long long)h * p.W + w0 + 4 * j;
      f32x4 xs[CIN_STEPS];
#pragma unroll
      for (int s = 0; s < CIN_STEPS; ++s) {
        const float* cp = chan_ptr(p.x, 4 * s + g, b, HW);
        xs[s] = cp ? *reinterpret_cast<const f32x4*>(cp + pix) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
      f32x4 acc2[COUT_TILES][4];
#pragma unroll
      for (int ot = 0; ot < COUT_TILES; ++ot)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc2[ot][q] = bias2[ot];

      // Software pipeline over the 16-channel hidden tiles: while the VALU runs GELU on tile t the
      // matrix pipe runs layer 2 of tile t-1 and layer 1 of tile t+1 (independent chains), so the
      // two pipes overlap inside ONE wave instead of relying on a partner wave being out of phase.
      auto fc1 = [&](int t, f32x4(&a1)[4]) {
        const f32x4 bb = *reinterpret_cast<const f32x4*>(s_b1 + 16 * t + 4 * g);
#pragma unroll
        for (int q = 0; q < 4; ++q) a1[q] = bb;
#pragma unroll
        for (int s = 0; s < CIN_STEPS; ++s) {
          const float a = s_w1[(t * CIN_STEPS + s) * 64 + lane];
#pragma unroll
          for (int q = 0; q < 4; ++q) a1[q] = mfma16x16x4(a, xs[s][q], a1[q]);
        }
      };
      // layer 2 sums over the hidden channel = ROW index of the layer-1 accumulator (row = 4g + r):
      // register r of lane-group g is k-slot g of step r -- no lane movement, no LDS.
      auto fc2 = [&](int t, const f32x4(&gl)[4]) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int ot = 0; ot < COUT_TILES; ++ot) {
            const float a2 = s_w2[((t * 4 + r) * COUT_TILES + ot) * 64 + lane];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc2[ot][q] = mfma16x16x4(a2, gl[q][r], acc2[ot][q]);
          }
      };
      auto act = [&](const f32x4(&a1)[4], f32x4(&gl)[4]) {
#pragma unroll
        for (int q = 0; q < 4; ++q) gl[q] = a1[q];
        gelu_erf8(gl[0], gl[1]);
        gelu_erf8(gl[2], gl[3]);
      };
      f32x4 a_cur[4], a_nxt[4], g_prev[4], g_new[4];
      fc1(0, a_cur);
      fc1(ntile > 1 ? 1 : 0, a_nxt);
      act(a_cur, g_prev);
#pragma unroll
      for (int q = 0; q < 4; ++q) a_cur[q] = a_nxt[q];
      for (int t = 1; t < ntile; ++t) {
        // Hand-interleaved trip: 16 slots, slot i = GELU of element i of tile t (VALU) + its share
        // of the matrix work, i.e. layer 1 of tile t+1 and layer 2 of tile t-1 (both independent of
        // the GELU in flight).  sched_barrier keeps hipcc from re-bunching the MFMAs: an in-order
        // wave that issues them back to back stalls on the matrix pipe before any VALU can issue.
        const int tn = (t + 1 < ntile) ? t + 1 : t;  // last trip: recompute tile t, result unused
        constexpr int kN1 = 4 * CIN_STEPS, kNM = kN1 + 16 * COUT_TILES;
        float w1r[CIN_STEPS], w2r[4][COUT_TILES];
#pragma unroll
        for (int s = 0; s < CIN_STEPS; ++s) w1r[s] = s_w1[(tn * CIN_STEPS + s) * 64 + lane];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int ot = 0; ot < COUT_TILES; ++ot) w2r[r][ot] = s_w2[(((t - 1) * 4 + r) * COUT_TILES + ot) * 64 + lane];
        {
          const f32x4 bb = *reinterpret_cast<const f32x4*>(s_b1 + 16 * tn + 4 * g);
#pragma unroll
          for (int q = 0; q < 4; ++q) a_nxt[q] = bb;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
          for (int m = (i * kNM) / 2; m < ((i + 1) * kNM) / 2; ++m) {
            if (m < kN1) {
              const int sidx = m / 4, q = m % 4;
              a_nxt[q] = mfma16x16x4(w1r[sidx], xs[sidx][q], a_nxt[q]);
            } else {
              const int mm = m - kN1;
              const int r = mm / (4 * COUT_TILES), ot = (mm / 4) % COUT_TILES, q = mm % 4;
              acc2[ot][q] = mfma16x16x4(w2r[r][ot], g_prev[q][r], acc2[ot][q]);
            }
          }
          g_new[2 * i] = a_cur[2 * i];
          g_new[2 * i + 1] = a_cur[2 * i + 1];
          gelu_erf8(g_new[2 * i], g_new[2 * i + 1]);
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          g_prev[q] = g_new[q];
          a_cur[q] = a_nxt[q];
        }
      }
      fc2(ntile - 1, g_prev);

      // epilogue: acc2[ot][q][r] = out[co = 16 ot + 4 g + r][pixel 4 j + q]
#pragma unroll
      for (int ot = 0; ot < COUT_TILES; ++ot)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = 16 * ot + 4 * g + r;
          f32x4 v = {acc2[ot][0][r], acc2[ot][1][r], acc2[ot][2][r], acc2[ot][3][r]};
          if (co < p.cout) {
            if (RESID) v += *reinterpret_cast<const f32x4*>(p.resid + (long long)b * p.resid_bstride +
                                                            (long long)co * HW + pix);
            *reinterpret_cast<f32x4*>(p.out + (long long)b * p.out_bstride + (long long)co * HW + pix) = v;
          }
          if (EMIT_Y) *reinterpret_cast<f32x4*>(s_tr + co * kTrStride + 4 * j) = v;
        }
      if (EMIT_Y) {
        wave_lds_fence();
        fwd_dft_accumulate<COUT_TILES, KP>(s_tr, p.tt, w0, lane, yacc);
        wave_lds_fence();
      }
    }
    if (EMIT_Y) store_y<COUT_TILES, KP>(p.ybuf, row, COUT_TILES * 16, lane, yacc);
  }
}

// ---------------------------------------------------------------------------------------------
// lifting, bf16x6 variant: out[32] = W2 * gelu(W1 * x + b1) + b2, plus the W-direction DFT of out.
// Layer 1 (Cin <= 32 -> hid) stays on fp32 MFMA (K is tiny); layer 2 (hid -> 32, K = hid) runs on the
// bf16 matrix pipe.  Hidden tiles are processed in PAIRS: the GELU outputs of tiles (2u, 2u+1) are
// exactly the 8 k-slots a lane supplies to one v_mfma_f32_16x16x32_bf16 -- k-slot (g, jj) = hidden
// channel 16*(2u + jj/4) + 4g + jj%4, i.e. the accumulator registers as they stand (no lane movement).
//   p.w2p here is W2 split and packed as [hid/32][3 parts][2 out tiles][64 lanes][4 dwords].
// ---------------------------------------------------------------------------------------------
template <int CIN_STEPS, int KP>
__global__ __launch_bounds__(512) void pw_lift_bf16x6_kernel(const MlpParams p) {
  extern __shared__ __align__(16) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int ntile = p.hid >> 4, npair = ntile >> 1;
  u32x4* s_w2 = reinterpret_cast<u32x4*>(smem);                      // [npair][3][2][64]
  float* s_w1 = reinterpret_cast<float*>(s_w2 + npair * 6 * 64);     // [ntile][CIN_STEPS][64]
  float* s_b1 = s_w1 + ntile * CIN_STEPS * 64;                       // [hid]
  float* s_tr = s_b1 + p.hid + wave * (kC * kTrStride);
  {
    const u32x4* src = reinterpret_cast<const u32x4*>(p.w2p);
    for (int i = tid; i < npair * 6 * 64; i += blockDim.x) s_w2[i] = src[i];
    for (int i = tid; i < ntile * CIN_STEPS * 64; i += blockDim.x) s_w1[i] = p.w1p[i];
    for (int i = tid; i < p.hid; i += blockDim.x) s_b1[i] = p.b1[i];
  }
  __syncthreads();
  const int HW = p.H * p.W, segs = p.W >> 6, nrow = p.B * p.H;
  f32x4 bias2[2];
  bias2[0] = *reinterpret_cast<const f32x4*>(p.b2 + 4 * g);
  bias2[1] = *reinterpret_cast<const f32x4*>(p.b2 + 16 + 4 * g);

  for (int row = blockIdx.x * nw + wave; row < nrow; row += gridDim.x * nw) {
    const int h = row % p.H, b = row / p.H;
    f32x4 yacc[2][KP / 16];
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
      for (int kt = 0; kt < KP / 16; ++kt) yacc[ot][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ws = 0; ws < segs; ++ws) {
      const int w0 = ws * 64;
      const long long pix = (long long)h * p.W + w0 + 4 * j;
      f32x4 xs[CIN_STEPS];
#pragma unroll
      for (int s = 0; s < CIN_STEPS; ++s) {
        const float* cp = chan_ptr(p.x, 4 * s + g, b, HW);
        xs[s] = cp ? *reinterpret_cast<const f32x4*>(cp + pix) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
      f32x4 acc2[2][4];
      lift_segment<CIN_STEPS>(xs, s_w1, s_b1, s_w2, npair, lane, bias2, acc2);

      // epilogue: acc2[ot][q][r] = out[co = 16 ot + 4 g + r][pixel 4 j + q]
#pragma unroll
      for (int ot = 0; ot < 2; ++ot)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = 16 * ot + 4 * g + r;
          const f32x4 v = {acc2[ot][0][r], acc2[ot][1][r], acc2[ot][2][r], acc2[ot][3][r]};
          *reinterpret_cast<f32x4*>(p.out + (long long)b * p.out_bstride + (long long)co * HW + pix) = v;
          *reinterpret_cast<f32x4*>(s_tr + co * kTrStride + 4 * j) = v;
        }
      wave_lds_fence();
      fwd_dft_accumulate<2, KP>(s_tr, p.tt, w0, lane, yacc);
      wave_lds_fence();
    }
    store_y<2, KP>(p.ybuf, row, kC, lane, yacc);
  }
}

// ---------------------------------------------------------------------------------------------
// projection with few outputs (CO <= 4):  out = W2 * gelu(W1 * h + b1) + b2 (+ residual)
// Layer 1 (32 -> hid) stays on fp32 MFMA; layer 2 (hid -> CO) would waste 12+ of 16 MFMA rows, and
// fp32 MFMA shares the fp32 lanes with the VALU on gfx950 (tools/ubench_fp32.hip: the two do not
// overlap), so it is done with CO*16 plain FMAs per hidden tile and one 4-lane-group reduction at
// the end.  Same software pipeline as pw_mlp2_kernel.
//   p.w2p here is W2 re-tiled as [hid/16][CO][16].
// ---------------------------------------------------------------------------------------------
template <int CO, bool RESID>
__global__ __launch_bounds__(256) void pw_proj_small_kernel(const MlpParams p) {
  extern __shared__ __align__(16) float smem[];
  constexpr int CS = 8;  // 32 input channels
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int ntile = p.hid >> 4;
  float* s_w1 = smem;
  float* s_b1 = s_w1 + ntile * CS * 64;
  float* s_w2 = s_b1 + p.hid;  // [ntile][CO][16]
  {
    const int n1 = ntile * CS * 64, n2 = ntile * CO * 16;
    for (int i = tid * 4; i < n1; i += blockDim.x * 4)
      *reinterpret_cast<f32x4*>(s_w1 + i) = *reinterpret_cast<const f32x4*>(p.w1p + i);
    for (int i = tid; i < p.hid; i += blockDim.x) s_b1[i] = p.b1[i];
    for (int i = tid; i < n2; i += blockDim.x) s_w2[i] = p.w2p[i];
  }
  __syncthreads();
  const int HW = p.H * p.W, segs = p.W >> 6, nrow = p.B * p.H;
  for (int row = blockIdx.x * nw + wave; row < nrow; row += gridDim.x * nw) {
    const int h = row % p.H, b = row / p.H;
    for (int ws = 0; ws < segs; ++ws) {
      const int w0 = ws * 64;
      const long long pix = (long long)h * p.W + w0 + 4 * j;
      f32x4 xs[CS];
#pragma unroll
      for (int s = 0; s < CS; ++s)
        xs[s] = *reinterpret_cast<const f32x4*>(p.x.seg[0].ptr + (long long)b * p.x.seg[0].bstride +
                                                (long long)(4 * s + g) * HW + pix);
      float po[CO][4];
#pragma unroll
      for (int co = 0; co < CO; ++co)
#pragma unroll
        for (int q = 0; q < 4; ++q) po[co][q] = 0.f;
      auto fc1 = [&](int t, f32x4(&a1)[4]) {
        const f32x4 bb = *reinterpret_cast<const f32x4*>(s_b1 + 16 * t + 4 * g);
#pragma unroll
        for (int q = 0; q < 4; ++q) a1[q] = bb;
#pragma unroll
        for (int s = 0; s < CS; ++s) {
          const float a = s_w1[(t * CS + s) * 64 + lane];
#pragma unroll
          for (int q = 0; q < 4; ++q) a1[q] = mfma16x16x4(a, xs[s][q], a1[q]);
        }
      };
      f32x4 a_cur[4], a_nxt[4], g_prev[4], g_new[4];
      fc1(0, a_cur);
      fc1(ntile > 1 ? 1 : 0, a_nxt);
#pragma unroll
      for (int q = 0; q < 4; ++q) g_prev[q] = a_cur[q];
      gelu_erf8(g_prev[0], g_prev[1]);
      gelu_erf8(g_prev[2], g_prev[3]);
#pragma unroll
      for (int q = 0; q < 4; ++q) a_cur[q] = a_nxt[q];
      for (int t = 1; t < ntile; ++t) {
        const int tn = (t + 1 < ntile) ? t + 1 : t;
        float w1r[CS];
#pragma unroll
        for (int s = 0; s < CS; ++s) w1r[s] = s_w1[(tn * CS + s) * 64 + lane];
        f32x4 w2v[CO];
#pragma unroll
        for (int co = 0; co < CO; ++co)
          w2v[co] = *reinterpret_cast<const f32x4*>(s_w2 + ((t - 1) * CO + co) * 16 + 4 * g);
        {
          const f32x4 bb = *reinterpret_cast<const f32x4*>(s_b1 + 16 * tn + 4 * g);
#pragma unroll
          for (int q = 0; q < 4; ++q) a_nxt[q] = bb;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
          for (int m = 16 * i; m < 16 * i + 16; ++m) a_nxt[m % 4] = mfma16x16x4(w1r[m / 4], xs[m / 4][m % 4], a_nxt[m % 4]);
          g_new[2 * i] = a_cur[2 * i];
          g_new[2 * i + 1] = a_cur[2 * i + 1];
          gelu_erf8(g_new[2 * i], g_new[2 * i + 1]);
#pragma unroll
          for (int co = 0; co < CO; ++co)
#pragma unroll
            for (int qq = 2 * i; qq < 2 * i + 2; ++qq)
#pragma unroll
              for (int r = 0; r < 4; ++r) po[co][qq] = fmaf(w2v[co][r], g_prev[qq][r], po[co][qq]);
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          g_prev[q] = g_new[q];
          a_cur[q] = a_nxt[q];
        }
      }
      {
        const int t = ntile - 1;
#pragma unroll
        for (int co = 0; co < CO; ++co) {
          const f32x4 w2 = *reinterpret_cast<const f32x4*>(s_w2 + (t * CO + co) * 16 + 4 * g);
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) po[co][q] = fmaf(w2[r], g_prev[q][r], po[co][q]);
        }
      }
      // sum the 4 lane groups (hidden channels 4g+r of every tile live in group g)
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int co = 0; co < CO; ++co)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float x = po[co][q];
          x += __shfl_xor(x, 16);
          x += __shfl_xor(x, 32);
          if (g == co) v[q] = x;
        }
      if (g < CO && g < p.cout) {
        const float bias = p.b2[g];
        v += f32x4{bias, bias, bias, bias};
        if (RESID) v += *reinterpret_cast<const f32x4*>(p.resid + (long long)b * p.resid_bstride + (long long)g * HW + pix);
        *reinterpret_cast<f32x4*>(p.out + (long long)b * p.out_bstride + (long long)g * HW + pix) = v;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// projection, bf16x6 variant: layer 1 (32 -> hid) runs on the bf16 matrix pipe as six
// v_mfma_f32_16x16x32_bf16 per (hidden tile, pixel chain) -- K = 32 input channels is exactly one
// instruction deep -- so the fp32 lanes only do GELU and the CO*16 FMAs of layer 2.
//   lane (j = l&15, g = l>>4) loads channels 8g..8g+7 (the 8 k-slots it supplies) of pixels 4j..4j+3;
//   p.w1p here is W1 split and packed as [hid/16][3 parts][64 lanes][4 dwords].
// ---------------------------------------------------------------------------------------------
template <int CO, bool RESID>
__global__ __launch_bounds__(512) void pw_proj_bf16x6_kernel(const MlpParams p) {
  extern __shared__ __align__(16) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int ntile = p.hid >> 4;
  u32x4* s_w1 = reinterpret_cast<u32x4*>(smem);                   // [ntile][3][64]
  float* s_b1 = reinterpret_cast<float*>(s_w1 + ntile * 3 * 64);  // [hid]
  float* s_w2 = s_b1 + p.hid;                                     // [ntile][CO][16]
  {
    const u32x4* src = reinterpret_cast<const u32x4*>(p.w1p);
    for (int i = tid; i < ntile * 3 * 64; i += blockDim.x) s_w1[i] = src[i];
    for (int i = tid; i < p.hid; i += blockDim.x) s_b1[i] = p.b1[i];
    for (int i = tid; i < ntile * CO * 16; i += blockDim.x) s_w2[i] = p.w2p[i];
  }
  __syncthreads();
  const int HW = p.H * p.W, segs = p.W >> 6, nrow = p.B * p.H;
  for (int row = blockIdx.x * nw + wave; row < nrow; row += gridDim.x * nw) {
    const int h = row % p.H, b = row / p.H;
    for (int ws = 0; ws < segs; ++ws) {
      const int w0 = ws * 64;
      const long long pix = (long long)h * p.W + w0 + 4 * j;
      u32x4 bx[4][3];  // B operands per pixel chain q: (h, m, l) parts of channels 8g..8g+7
      {
        f32x4 xs[8];
#pragma unroll
        for (int c = 0; c < 8; ++c)
          xs[c] = *reinterpret_cast<const f32x4*>(p.x.seg[0].ptr + (long long)b * p.x.seg[0].bstride +
                                                  (long long)(8 * g + c) * HW + pix);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            unsigned hh, mm, ll;
            split3_pair(xs[2 * i][q], xs[2 * i + 1][q], hh, mm, ll);
            bx[q][0][i] = hh;
            bx[q][1][i] = mm;
            bx[q][2][i] = ll;
          }
      }
      float po[CO][4];
      proj_segment<CO>(bx, s_w1, s_b1, s_w2, ntile, lane, po);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int co = 0; co < CO; ++co)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float x = po[co][q];
          x += __shfl_xor(x, 16);
          x += __shfl_xor(x, 32);
          if (g == co) v[q] = x;
        }
      if (g < CO && g < p.cout) {
        const float bias = p.b2[g];
        v += f32x4{bias, bias, bias, bias};
        if (RESID) v += *reinterpret_cast<const f32x4*>(p.resid + (long long)b * p.resid_bstride + (long long)g * HW + pix);
        *reinterpret_cast<f32x4*>(p.out + (long long)b * p.out_bstride + (long long)g * HW + pix) = v;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// spectral layer:  y = act( skip(x) + bias + inverse-W-DFT(Z) ),  optionally Y_next = fwd-W-DFT(y)
//   skip  : neuralop FNOBlocks.fno_skips[l] (1x1 conv, no bias)
//   bias  : SpectralConv.bias[l]
//   Z     : per-row, per-k' coefficients produced by modes_kernel
// Also serves SpectralConv2d (unet.py:46-69) with SKIP=false, ACT=false, EMIT_Y=false.
// ---------------------------------------------------------------------------------------------
// NO = 16-channel output tiles per wave: 2 -> one wave per row segment, 1 -> the row is split between
// two waves (4 waves/SIMD at B*H = 2048 rows: on gfx950 VALU issue and latency hiding both improve
// with occupancy, and the second wave's x loads hit L1/L2).
template <int KP, bool SKIP, bool ACT, bool EMIT_Y, int NO, bool SKIPB = false>
__global__ __launch_bounds__(512) void fno_layer_kernel(const LayerParams p) {
  extern __shared__ __align__(16) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  float* s_tr = smem + wave * (NO * 16 * kTrStride);
  // Stagger: an 8-wave workgroup puts waves w and w+4 on the same SIMD.  Every wave runs
  // load -> MFMA -> store once; started together all waves hit memory, then the fp32 pipe, then memory
  // again (PMC: ~45 % of wave life in s_waitcnt).  Delaying the second half by about one load phase
  // lets its loads overlap the first half's MFMAs and its MFMAs the first half's stores.
  if (p.stagger > 0 && __builtin_amdgcn_readfirstlane(wave) >= 4) {
    for (int i = 0; i < p.stagger; ++i) __builtin_amdgcn_s_sleep(32);
  }
  const int HW = p.H * p.W;
  const int segs = p.W >> 6;
  constexpr int SPLIT = 2 / NO;
  const int nunit = p.B * p.H * SPLIT;

  for (int unit = blockIdx.x * nw + wave; unit < nunit; unit += gridDim.x * nw) {
    const int row = unit / SPLIT, ot0 = (unit % SPLIT) * NO;   // first 16-channel output tile of this wave
    const int h = row % p.H, b = row / p.H;
    float wa[SKIPB ? 1 : 8][NO];
    u32x4 wb[SKIPB ? NO : 1][3];
    if (SKIP && !SKIPB) {
#pragma unroll
      for (int s = 0; s < 8; ++s)
#pragma unroll
        for (int ot = 0; ot < NO; ++ot) wa[s][ot] = p.wsp[(s * 2 + ot0 + ot) * 64 + lane];
    }
    if (SKIP && SKIPB) {
#pragma unroll
      for (int ot = 0; ot < NO; ++ot)
#pragma unroll
        for (int pp = 0; pp < 3; ++pp) wb[ot][pp] = p.wsb[((ot0 + ot) * 3 + pp) * 64 + lane];
    }
    f32x4 bias4[NO];
#pragma unroll
    for (int ot = 0; ot < NO; ++ot) bias4[ot] = *reinterpret_cast<const f32x4*>(p.bias + 16 * (ot0 + ot) + 4 * g);
    // Z operands of this row: A[i = o][k = k'] -> lane reads Z[k' = 4 s + g][o = 16 ot + j]
    float z[KP / 4][NO];
    {
      const float* zr = p.zbuf + (long long)row * KP * kC;
#pragma unroll
      for (int s = 0; s < KP / 4; ++s)
#pragma unroll
        for (int ot = 0; ot < NO; ++ot) z[s][ot] = zr[(4 * s + g) * kC + 16 * (ot0 + ot) + j];
    }
    f32x4 yacc[NO][KP / 16];
    if (EMIT_Y) {
#pragma unroll
      for (int ot = 0; ot < NO; ++ot)
#pragma unroll
        for (int kt = 0; kt < KP / 16; ++kt) yacc[ot][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int ws = 0; ws < segs; ++ws) {
      const int w0 = ws * 64;
      const long long pix = (long long)h * p.W + w0 + 4 * j;
      f32x4 acc[NO][4];
#pragma unroll
      for (int ot = 0; ot < NO; ++ot)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[ot][q] = bias4[ot];
      if (SKIP && !SKIPB) {
        f32x4 xs[8];
#pragma unroll
        for (int s = 0; s < 8; ++s)
          xs[s] = *reinterpret_cast<const f32x4*>(p.x + ((long long)b * kC + 4 * s + g) * HW + pix);
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int ot = 0; ot < NO; ++ot) acc[ot][q] = mfma16x16x4(wa[s][ot], xs[s][q], acc[ot][q]);
      }
      if (SKIP && SKIPB) {
        // 1x1 skip convolution on the bf16 matrix pipe (bf16x6): K = 32 channels is one instruction deep;
        // this lane supplies channels 8g..8g+7 of its 4 pixels
        f32x4 xs[8];
#pragma unroll
        for (int c = 0; c < 8; ++c)
          xs[c] = *reinterpret_cast<const f32x4*>(p.x + ((long long)b * kC + 8 * g + c) * HW + pix);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          u32x4 bx[3];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            unsigned hh, mm, ll;
            split3_pair(xs[2 * i][q], xs[2 * i + 1][q], hh, mm, ll);
            bx[0][i] = hh;
            bx[1][i] = mm;
            bx[2][i] = ll;
          }
#pragma unroll
          for (int ot = 0; ot < NO; ++ot) acc[ot][q] = mfma_bf16x6(wb[ot], bx, acc[ot][q]);
        }
      }
#pragma unroll
      for (int s = 0; s < KP / 4; ++s) {
        const f32x4 tw = *reinterpret_cast<const f32x4*>(p.t + (long long)(4 * s + g) * p.W + w0 + 4 * j);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int ot = 0; ot < NO; ++ot) acc[ot][q] = mfma16x16x4(z[s][ot], tw[q], acc[ot][q]);
      }
      f32x4 vv[NO][4];
#pragma unroll
      for (int ot = 0; ot < NO; ++ot)
#pragma unroll
        for (int r = 0; r < 4; ++r) vv[ot][r] = f32x4{acc[ot][0][r], acc[ot][1][r], acc[ot][2][r], acc[ot][3][r]};
      if (ACT) {
#pragma unroll
        for (int ot = 0; ot < NO; ++ot) {
          gelu_erf8(vv[ot][0], vv[ot][1]);
          gelu_erf8(vv[ot][2], vv[ot][3]);
        }
      }
#pragma unroll
      for (int ot = 0; ot < NO; ++ot)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int cl = 16 * ot + 4 * g + r;
          *reinterpret_cast<f32x4*>(p.y + ((long long)b * kC + 16 * ot0 + cl) * HW + pix) = vv[ot][r];
          if (EMIT_Y) *reinterpret_cast<f32x4*>(s_tr + cl * kTrStride + 4 * j) = vv[ot][r];
        }
      if (EMIT_Y) {
        wave_lds_fence();
        fwd_dft_accumulate<NO, KP>(s_tr, p.tt, w0, lane, yacc);
        wave_lds_fence();
      }
    }
    if (EMIT_Y) store_y<NO, KP>(p.ybuf, row, kC, lane, yacc, 16 * ot0);
  }
}

// W-direction forward DFT only: x [B][32][H][W] -> Ybuf [B][H][32][KP]   (SpectralConv2d entry)
template <int KP>
__global__ __launch_bounds__(256) void fwd_dft_kernel(const float* __restrict__ x, float* __restrict__ ybuf,
                                                      const float* __restrict__ tt, int B, int H, int W) {
  extern __shared__ __align__(16) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  float* s_tr = smem + wave * (kC * kTrStride);
  const int HW = H * W, segs = W >> 6, nrow = B * H;
  for (int row = blockIdx.x * nw + wave; row < nrow; row += gridDim.x * nw) {
    const int h = row % H, b = row / H;
    f32x4 yacc[2][KP / 16];
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
      for (int kt = 0; kt < KP / 16; ++kt) yacc[ot][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ws = 0; ws < segs; ++ws) {
      const int w0 = ws * 64;
      const long long pix = (long long)h * W + w0 + 4 * j;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const int c = 4 * s + g;
        *reinterpret_cast<f32x4*>(s_tr + c * kTrStride + 4 * j) =
            *reinterpret_cast<const f32x4*>(x + ((long long)b * kC + c) * HW + pix);
      }
      wave_lds_fence();
      fwd_dft_accumulate<2, KP>(s_tr, tt, w0, lane, yacc);
      wave_lds_fence();
    }
    store_y<2, KP>(ybuf, row, kC, lane, yacc);
  }
}

// ---------------------------------------------------------------------------------------------
// modes kernel: one workgroup (256 threads) per (sample b, rfft column ky)
//   P1  X[r][c] = fwd_scale * sum_h EF[r][h] * Y[h][c]        (H-direction pruned DFT, M1 rows)
//   P2  O[r][o] = sum_c X[r][c] * Wt[ky][r][c][o]             (einsum 'bixy,ioxy->boxy')
//   P3  Z[h][o] = ck[ky] * sum_r EI[r][h] * O[r][o]           (inverse H-direction)
// Thread (lo = tid & 31, hi = tid >> 5): lo is the channel, hi splits h (P1, P3) or r (P2) 8 ways.
// The (ky) weight slice [M1][C][C] complex is pulled into LDS by LDS-DMA at kernel entry and is
// only waited for before P2, so its L2 latency hides behind P1.  Blocks with ky >= M2 zero the
// padding rows of Z.
// ---------------------------------------------------------------------------------------------
struct ModesParams {
  const float* ybuf;   // [B][H][KP][C]
  float* zbuf;         // [B][H][KP][C]
  const float2* wt;    // [M2][M1][C][C]
  const float2* ef;    // [M1][H]  (cos, -sin) of 2 pi kx_in h / H
  const float2* ei;    // [M1][H]  (cos, +sin) of 2 pi kx_out h / H
  const float* ck;     // [M2]  Hermitian weight (1 or 2) * inv_scale
  float fwd_scale;
  int B, H, M1, M2, KP;
};

// 1024 threads = 16 waves = 4 per SIMD: on gfx950 a lone wave issues one VALU op per ~6 cycles, four
// waves per SIMD one per ~2.8 (tools/ubench_fp32.hip), and this kernel is pure VALU + latency.
// Thread (lo = tid & 31, hi = tid >> 5 in 0..31): lo = channel; hi splits h 32 ways in P1 / P3 and
// (r, half of the c-sum) in P2.  HC = ceil(H / 32).  RG = 16 or 32 row slots (M1 <= RG).
// The weights a thread needs in P2 (32*16/RG float2) are requested right after the Y loads and first
// used in P2, so their L2 latency hides behind P1.
template <int HC, int RG>
__global__ __launch_bounds__(1024) void fno_modes_kernel(const ModesParams p) {
  extern __shared__ __align__(16) float smem[];
  constexpr int C = kC, CP = 32 / RG, CN = C / CP;  // CP c-parts, CN channels summed per thread in P2
  const int ky = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int lo = tid & 31, hi = tid >> 5;
  const int H = p.H, M1 = p.M1, KP = p.KP;
  float* zb = p.zbuf + (long long)b * H * KP * C;
  if (ky >= p.M2) {
    for (int i = tid; i < H * C; i += 1024) {
      const int o = i & 31, h = i >> 5;
      zb[((long long)h * KP + 2 * ky) * C + o] = 0.f;
      zb[((long long)h * KP + 2 * ky + 1) * C + o] = 0.f;
    }
    return;
  }
  float2* s_ef = reinterpret_cast<float2*>(smem);   // [M1][H]
  float2* s_ei = s_ef + M1 * H;                     // [M1][H]
  float2* s_part = s_ei + M1 * H;                   // [16 waves][M1][C]  P1 partials, reused as [CP][M1][C] in P2
  float2* s_x = s_part + 16 * M1 * C;               // [M1][C]
  float2* s_o = s_x + M1 * C;                       // [M1][C]

  float2 yv[HC];
  {
    const float* yb = p.ybuf + (long long)b * H * KP * C;
#pragma unroll
    for (int i = 0; i < HC; ++i) {
      const int h = hi * HC + i;
      if (h < H) {
        yv[i].x = yb[((long long)h * KP + 2 * ky) * C + lo];
        yv[i].y = yb[((long long)h * KP + 2 * ky + 1) * C + lo];
      } else {
        yv[i] = float2{0.f, 0.f};
      }
    }
  }
  for (int i = tid; i < M1 * H; i += 1024) {
    s_ef[i] = p.ef[i];
    s_ei[i] = p.ei[i];
  }
  const int r2 = hi % RG, cpart = hi / RG;
  float2 wreg[CN];
  {
    const float2* w = p.wt + ((long long)ky * M1 + (r2 < M1 ? r2 : 0)) * C * C + (size_t)cpart * CN * C + lo;
#pragma unroll
    for (int c = 0; c < CN; ++c) wreg[c] = w[c * C];
  }
  __syncthreads();
  // P1: X[r][c] partial over this thread's h slice
  for (int r = 0; r < M1; ++r) {
    float2 acc = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < HC; ++i) {
      const int h = hi * HC + i;
      acc = cfma(yv[i], s_ef[r * H + (h < H ? h : 0)], acc);
    }
    acc.x += __shfl_xor(acc.x, 32);
    acc.y += __shfl_xor(acc.y, 32);
    if ((tid & 32) == 0) s_part[((tid >> 6) * M1 + r) * C + lo] = acc;
  }
  __syncthreads();
  for (int i = tid; i < M1 * C; i += 1024) {
    float2 a = s_part[i];
#pragma unroll
    for (int w = 1; w < 16; ++w) {
      const float2 t = s_part[w * M1 * C + i];
      a.x += t.x;
      a.y += t.y;
    }
    s_x[i] = float2{a.x * p.fwd_scale, a.y * p.fwd_scale};
  }
  __syncthreads();
  // P2: O[r][o] partial over this thread's c slice
  if (r2 < M1) {
    float2 acc = {0.f, 0.f};
#pragma unroll
    for (int c = 0; c < CN; ++c) acc = cfma(s_x[r2 * C + cpart * CN + c], wreg[c], acc);
    s_part[(cpart * M1 + r2) * C + lo] = acc;
  }
  __syncthreads();
  for (int i = tid; i < M1 * C; i += 1024) {
    float2 a = s_part[i];
#pragma unroll
    for (int cp = 1; cp < CP; ++cp) {
      const float2 t = s_part[cp * M1 * C + i];
      a.x += t.x;
      a.y += t.y;
    }
    s_o[i] = a;
  }
  __syncthreads();
  // P3
  {
    float2 acc[HC];
#pragma unroll
    for (int i = 0; i < HC; ++i) acc[i] = float2{0.f, 0.f};
    for (int r = 0; r < M1; ++r) {
      const float2 ov = s_o[r * C + lo];
#pragma unroll
      for (int i = 0; i < HC; ++i) {
        const int h = hi * HC + i;
        acc[i] = cfma(ov, s_ei[r * H + (h < H ? h : 0)], acc[i]);
      }
    }
    const float ck = p.ck[ky];
#pragma unroll
    for (int i = 0; i < HC; ++i) {
      const int h = hi * HC + i;
      if (h < H) {
        zb[((long long)h * KP + 2 * ky) * C + lo] = acc[i].x * ck;
        zb[((long long)h * KP + 2 * ky + 1) * C + lo] = acc[i].y * ck;
      }
    }
  }
}

// Spectral weights [Ci][Co][R][K][2] (reference / PyTorch layout, device) -> the kernels' [K][R][Ci'][Co'] float2.
// adjoint: the conjugate transpose (Ci' = Co, Co' = Ci), i.e. the weights of the backward-data convolution.
__global__ __launch_bounds__(256) void pack_spectral_kernel(const float2* __restrict__ src, float2* __restrict__ dst,
                                                            int Ci, int Co, int R, int K, int adjoint) {
  const long long total = (long long)Ci * Co * R * K;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int ky = (int)(i % K);
    const int r = (int)((i / K) % R);
    const int o = (int)((i / ((long long)K * R)) % Co);
    const int c = (int)(i / ((long long)K * R * Co));
    const float2 v = src[i];
    if (adjoint) dst[(((long long)ky * R + r) * Co + o) * Ci + c] = float2{v.x, -v.y};
    else dst[(((long long)ky * R + r) * Ci + c) * Co + o] = v;
  }
}

// ---------------------------------------------------------------------------------------------
// host side: the launches
// ---------------------------------------------------------------------------------------------
static int grid_rows(int nrow, int waves_per_block) {
  int blocks = (nrow + waves_per_block - 1) / waves_per_block;
  const int cap = 256 * 8;
  return blocks < cap ? (blocks > 0 ? blocks : 1) : cap;
}

template <int HC>
static int32_t launch_modes_hc(const ModesParams& mp, size_t lds, dim3 grid, hipStream_t s) {
  if (mp.M1 <= 16) {
    DLWP_HIP_CHECK(allow_lds(fno_modes_kernel<HC, 16>, lds));
    hipLaunchKernelGGL((fno_modes_kernel<HC, 16>), grid, dim3(1024), lds, s, mp);
  } else if (mp.M1 <= 32) {
    DLWP_HIP_CHECK(allow_lds(fno_modes_kernel<HC, 32>, lds));
    hipLaunchKernelGGL((fno_modes_kernel<HC, 32>), grid, dim3(1024), lds, s, mp);
  } else {
    return fail(DLWP_ERR_UNSUPPORTED, "more than 32 kept spectral rows (%d) not supported", mp.M1);
  }
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

int32_t launch_modes(const SpectralCore& sc, const float* ybuf, float* zbuf, const float2* wt, int B, hipStream_t s) {
  ModesParams mp;
  mp.ybuf = ybuf; mp.zbuf = zbuf; mp.wt = wt;
  mp.ef = sc.ef.as<float2>(); mp.ei = sc.ei.as<float2>(); mp.ck = sc.ck.as<float>();
  mp.fwd_scale = sc.fwd_scale;
  mp.B = B; mp.H = sc.H; mp.M1 = sc.M1; mp.M2 = sc.M2; mp.KP = sc.KP;
  const size_t lds = sc.modes_lds_bytes();
  DLWP_REQUIRE(lds <= 160 * 1024, DLWP_ERR_UNSUPPORTED, "modes kernel needs %zu bytes of LDS", lds);
  const dim3 grid(sc.KP / 2, B);
  const int hc = (sc.H + 31) / 32;
  if (hc <= 1) return launch_modes_hc<1>(mp, lds, grid, s);
  if (hc <= 2) return launch_modes_hc<2>(mp, lds, grid, s);
  if (hc <= 4) return launch_modes_hc<4>(mp, lds, grid, s);
  if (hc <= 8) return launch_modes_hc<8>(mp, lds, grid, s);
  return fail(DLWP_ERR_UNSUPPORTED, "grid height %d > 256 not supported by the modes kernel", sc.H);
}

template <bool SKIP, bool ACT, bool EMIT_Y>
static int32_t launch_layer_form(const SpectralCore& sc, const LayerParams& lp, hipStream_t s, bool bf16x6) {
  // NO = 1 (row split between two waves, 4 waves/SIMD at the headline size) measured SLOWER than one
  // wave per row (16.6 vs 13.7 us event-timed: the duplicated x / Z / weight loads cost more than the
  // occupancy buys), so it stays off; kept as a template parameter for larger grids.
  const int nrow = lp.B * lp.H;
  const bool split = false;
  const size_t lds = EMIT_Y ? (size_t)8 * (split ? 16 : 32) * kTrStride * sizeof(float) : 0;
  const int grid = grid_rows(nrow * (split ? 2 : 1), 8);
  if (lds > 48 * 1024) {
    DLWP_HIP_CHECK(allow_lds((fno_layer_kernel<16, SKIP, ACT, EMIT_Y, 2, false>), lds));
    DLWP_HIP_CHECK(allow_lds((fno_layer_kernel<32, SKIP, ACT, EMIT_Y, 2, false>), lds));
    DLWP_HIP_CHECK(allow_lds((fno_layer_kernel<16, SKIP, ACT, EMIT_Y, 1, false>), lds));
    DLWP_HIP_CHECK(allow_lds((fno_layer_kernel<32, SKIP, ACT, EMIT_Y, 1, false>), lds));
    DLWP_HIP_CHECK(allow_lds((fno_layer_kernel<16, SKIP, ACT, EMIT_Y, 2, SKIP>), lds));
    DLWP_HIP_CHECK(allow_lds((fno_layer_kernel<32, SKIP, ACT, EMIT_Y, 2, SKIP>), lds));
    DLWP_HIP_CHECK(allow_lds((fno_layer_kernel<16, SKIP, ACT, EMIT_Y, 1, SKIP>), lds));
    DLWP_HIP_CHECK(allow_lds((fno_layer_kernel<32, SKIP, ACT, EMIT_Y, 1, SKIP>), lds));
  }
  const bool skipb = SKIP && lp.wsb != nullptr && bf16x6;
#define DLWP_LAUNCH_LAYER(KP_, NO_)                                                                                \
  do {                                                                                                             \
    if (skipb)                                                                                                     \
      hipLaunchKernelGGL((fno_layer_kernel<KP_, SKIP, ACT, EMIT_Y, NO_, SKIP>), dim3(grid), dim3(512), lds, s, lp); \
    else                                                                                                           \
      hipLaunchKernelGGL((fno_layer_kernel<KP_, SKIP, ACT, EMIT_Y, NO_, false>), dim3(grid), dim3(512), lds, s, lp); \
  } while (0)
  if (sc.KP == 16) {
    if (split) DLWP_LAUNCH_LAYER(16, 1); else DLWP_LAUNCH_LAYER(16, 2);
  } else {
    if (split) DLWP_LAUNCH_LAYER(32, 1); else DLWP_LAUNCH_LAYER(32, 2);
  }
#undef DLWP_LAUNCH_LAYER
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

int32_t launch_layer(const SpectralCore& sc, const LayerParams& lp, LayerForm form, hipStream_t s, bool bf16x6) {
  switch (form) {
    case LayerForm::kFnoHidden: return launch_layer_form<true, true, true>(sc, lp, s, bf16x6);
    case LayerForm::kFnoLast: return launch_layer_form<true, false, false>(sc, lp, s, bf16x6);
    default: return launch_layer_form<false, false, false>(sc, lp, s, bf16x6);
  }
}

// W-direction forward DFT alone: x [B][32][H][W] -> ybuf (SpectralConv2d entry)
int32_t launch_fwd_dft(const SpectralCore& sc, const float* x, float* ybuf, int B, hipStream_t s) {
  const int grid = grid_rows(B * sc.H, 4);
  const size_t lds = (size_t)4 * kC * kTrStride * sizeof(float);
  if (sc.KP == 16) hipLaunchKernelGGL((fwd_dft_kernel<16>), dim3(grid), dim3(256), lds, s, x, ybuf, sc.tt.as<float>(), B, sc.H, sc.W);
  else hipLaunchKernelGGL((fwd_dft_kernel<32>), dim3(grid), dim3(256), lds, s, x, ybuf, sc.tt.as<float>(), B, sc.H, sc.W);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

// src is [Ci][Co][R][K][2] of the FORWARD operator in both cases (pack_spectral_kernel)
int32_t launch_pack_spectral(const float2* src, float2* dst, int Ci, int Co, int R, int K, bool adjoint, hipStream_t s) {
  const long long total = (long long)Ci * Co * R * K;
  long long blocks = (total + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(pack_spectral_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, dst, Ci, Co, R, K, adjoint ? 1 : 0);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

template <int CS>
static int32_t launch_lift_cs(const MlpParams& mp, int kp, int grid, size_t lds, hipStream_t s, bool bf, size_t lds_bf) {
  if (bf) {
    if (kp == 16) {
      DLWP_HIP_CHECK(allow_lds(pw_lift_bf16x6_kernel<CS, 16>, lds_bf));
      hipLaunchKernelGGL((pw_lift_bf16x6_kernel<CS, 16>), dim3((grid + 1) / 2), dim3(512), lds_bf, s, mp);
    } else {
      DLWP_HIP_CHECK(allow_lds(pw_lift_bf16x6_kernel<CS, 32>, lds_bf));
      hipLaunchKernelGGL((pw_lift_bf16x6_kernel<CS, 32>), dim3((grid + 1) / 2), dim3(512), lds_bf, s, mp);
    }
  } else if (kp == 16) {
    DLWP_HIP_CHECK(allow_lds(pw_mlp2_kernel<CS, 2, 16, true, false>, lds));
    hipLaunchKernelGGL((pw_mlp2_kernel<CS, 2, 16, true, false>), dim3(grid), dim3(256), lds, s, mp);
  } else {
    DLWP_HIP_CHECK(allow_lds(pw_mlp2_kernel<CS, 2, 32, true, false>, lds));
    hipLaunchKernelGGL((pw_mlp2_kernel<CS, 2, 32, true, false>), dim3(grid), dim3(256), lds, s, mp);
  }
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

// lifting (+ W-direction DFT of its output) as a launch of its own: xt -> ws.h0, ws.ybuf
int32_t fno_lift(const dlwp_fno2d_plan* p, const ChanTable& xt, int B, const FnoWorkspace& ws, hipStream_t s, KernelTimer* timer) {
  const int nrow = B * p->H;
  {
    MlpParams mp;
    mp.x = xt; mp.hid = p->hid_l; mp.cout = kC;
    mp.w1p = p->lift_w1p.as<float>(); mp.b1 = p->lift_b1.as<float>();
    mp.w2p = p->lift_w2p.as<float>(); mp.b2 = p->lift_b2.as<float>();
    mp.out = ws.h0; mp.out_bstride = (long long)kC * p->H * p->W;
    mp.resid = nullptr; mp.resid_bstride = 0;
    mp.ybuf = ws.ybuf; mp.tt = p->sc.tt.as<float>();
    mp.B = B; mp.H = p->H; mp.W = p->W;
    const int nt = p->hid_l / 16;
    const size_t lds = ((size_t)nt * p->cin_steps * 64 + p->hid_l + (size_t)nt * 4 * 2 * 64 + 4 * kC * kTrStride) * 4;
    const bool bf = !p->k.fp32_mfma && p->lift_w2b.p != nullptr;
    // 8-wave workgroups: the ~53 KB of staged weights are shared by 8 rows and one workgroup per CU
    // keeps 2 waves per SIMD resident (4-wave workgroups at 88 KB of LDS ran one per CU, in two rounds)
    const size_t lds_bf = ((size_t)(nt / 2) * 6 * 64 * 4 + (size_t)nt * p->cin_steps * 64 + p->hid_l + 8 * kC * kTrStride) * 4;
    if (bf) mp.w2p = p->lift_w2b.as<float>();
    const int grid = grid_rows(nrow, 4);
    int32_t rc;
    if (timer) DLWP_HIP_CHECK(timer->begin(KernelTimer::LIFT));
    switch (p->cin_steps) {
      case 1: rc = launch_lift_cs<1>(mp, p->sc.KP, grid, lds, s, bf, lds_bf); break;
      case 2: rc = launch_lift_cs<2>(mp, p->sc.KP, grid, lds, s, bf, lds_bf); break;
      case 3: rc = launch_lift_cs<3>(mp, p->sc.KP, grid, lds, s, bf, lds_bf); break;
      case 4: rc = launch_lift_cs<4>(mp, p->sc.KP, grid, lds, s, bf, lds_bf); break;
      case 5: rc = launch_lift_cs<5>(mp, p->sc.KP, grid, lds, s, bf, lds_bf); break;
      case 6: rc = launch_lift_cs<6>(mp, p->sc.KP, grid, lds, s, bf, lds_bf); break;
      case 7: rc = launch_lift_cs<7>(mp, p->sc.KP, grid, lds, s, bf, lds_bf); break;
      default: rc = launch_lift_cs<8>(mp, p->sc.KP, grid, lds, s, bf, lds_bf); break;
    }
    if (rc != DLWP_OK) return rc;
    if (timer) DLWP_HIP_CHECK(timer->end(KernelTimer::LIFT));
  }
  return DLWP_OK;
}

// projection (+ residual) as a launch of its own
int32_t fno_project(const dlwp_fno2d_plan* p, const float* hin, int B, float* out, long long out_bstride,
                    const float* resid, long long resid_bstride, hipStream_t s, KernelTimer* timer) {
  const int nrow = B * p->H;
  // projection (+ residual)
  {
    MlpParams mp;
    mp.x.seg[0] = ChanSeg{hin, (long long)kC * p->H * p->W, kC, 0};
    for (int i = 1; i < 4; ++i) mp.x.seg[i] = ChanSeg{nullptr, 0, 0, 0};
    mp.hid = p->hid_p; mp.cout = p->cout;
    mp.w1p = p->proj_w1p.as<float>(); mp.b1 = p->proj_b1.as<float>();
    mp.w2p = p->proj_w2p.as<float>(); mp.b2 = p->proj_b2.as<float>();
    mp.out = out; mp.out_bstride = out_bstride; mp.resid = resid; mp.resid_bstride = resid_bstride;
    mp.ybuf = nullptr; mp.tt = nullptr;
    mp.B = B; mp.H = p->H; mp.W = p->W;
    const int nt = p->hid_p / 16;
    const size_t lds = ((size_t)nt * 8 * 64 + p->hid_p + (size_t)nt * 4 * 1 * 64) * 4;
    const int grid = grid_rows(nrow, 4);
    if (timer) DLWP_HIP_CHECK(timer->begin(KernelTimer::PROJ));
    if (p->proj_co > 0) {
      mp.w2p = p->proj_w2v.as<float>();
      const bool bf = !p->k.fp32_mfma;
      if (bf) mp.w1p = p->proj_w1b.as<float>();
      const size_t lds2 = bf ? ((size_t)nt * 3 * 64 * 4 + p->hid_p + (size_t)nt * p->proj_co * 16) * 4
                             : ((size_t)nt * 8 * 64 + p->hid_p + (size_t)nt * p->proj_co * 16) * 4;
#define DLWP_LAUNCH_PROJ(CO_, RES_)                                                                     \
  do {                                                                                                  \
    if (bf) {                                                                                           \
      DLWP_HIP_CHECK(allow_lds(pw_proj_bf16x6_kernel<CO_, RES_>, lds2));                                \
      hipLaunchKernelGGL((pw_proj_bf16x6_kernel<CO_, RES_>), dim3((grid + 1) / 2), dim3(512), lds2, s, mp); \
    } else {                                                                                            \
      DLWP_HIP_CHECK(allow_lds(pw_proj_small_kernel<CO_, RES_>, lds2));                                 \
      hipLaunchKernelGGL((pw_proj_small_kernel<CO_, RES_>), dim3(grid), dim3(256), lds2, s, mp);        \
    }                                                                                                   \
  } while (0)
      if (p->proj_co == 1) { if (resid) DLWP_LAUNCH_PROJ(1, true); else DLWP_LAUNCH_PROJ(1, false); }
      else if (p->proj_co == 2) { if (resid) DLWP_LAUNCH_PROJ(2, true); else DLWP_LAUNCH_PROJ(2, false); }
      else { if (resid) DLWP_LAUNCH_PROJ(4, true); else DLWP_LAUNCH_PROJ(4, false); }
#undef DLWP_LAUNCH_PROJ
    } else if (resid) {
      DLWP_HIP_CHECK(allow_lds(pw_mlp2_kernel<8, 1, 16, false, true>, lds));
      hipLaunchKernelGGL((pw_mlp2_kernel<8, 1, 16, false, true>), dim3(grid), dim3(256), lds, s, mp);
    } else {
      DLWP_HIP_CHECK(allow_lds(pw_mlp2_kernel<8, 1, 16, false, false>, lds));
      hipLaunchKernelGGL((pw_mlp2_kernel<8, 1, 16, false, false>), dim3(grid), dim3(256), lds, s, mp);
    }
    DLWP_HIP_CHECK(hipGetLastError());
    if (timer) DLWP_HIP_CHECK(timer->end(KernelTimer::PROJ));
  }
  return DLWP_OK;
}

}  // namespace fno
}  // namespace dlwp
