// FNO2d rollout + SpectralConv2d for MI355X (gfx950).
//
// Replaces, on the device:
//   * reference models/fno/fno.py:64-106  (FNO2DModule.forward: rollout loop, _prepare_inputs,
//     self.fno(x_t), residual, stack) -- arithmetic of neuralop.models.FNO restated in
//     oracle/restate/fno.py (parity unpinned: third-party, absent from the reference tree);
//   * reference models/unet/unet.py:15-69 (SpectralConv2d + batchmul2d) -- pinned.
//
// Design (DESIGN.md has the long form):
//   The spectral convolution keeps only M1 x M2 modes (12 x 7 of 64 x 33 at the headline
//   config), so instead of a full FFT the transform is a *pruned DFT*, factored as
//       W-direction: Y[h, k'] = sum_w x[h, w] T[k'][w]      (k' = (ky, re/im), KP <= 32 reals)
//       H-direction + channel mixing + inverse H-direction: tiny, per (sample, ky)
//       W-direction back: y[h, w] += sum_k' Z[h, k'] T[k'][w]
//   The two W-direction products and the 1x1 convolutions are per-pixel channel contractions
//   -> fp32 MFMA (v_mfma_f32_16x16x4_f32, bit-exact fp32 FMA chains), one wave per grid row
//   segment of 64 pixels, operands loaded straight from NCHW memory as 16-byte vectors.
//   Per FNO layer:   modes_kernel (Y -> Z)   then   layer_kernel (x, Z -> y, Y_next)
//   i.e. one read and one write of the activation per layer; lifting and projection MLPs are one
//   fused kernel each (hidden 256-wide activation never leaves registers).
#include "common.hpp"
#include "spectral_any.hpp"
#include <atomic>
#include <memory>

// GELU form per phase of the fused step kernel (A/B switch: -DDLWP_GELU8_LIFT=gelu_erf8_fma etc.)
#ifndef DLWP_GELU8_LIFT
#define DLWP_GELU8_LIFT gelu_erf8
#endif
#ifndef DLWP_GELU8_PROJ
#define DLWP_GELU8_PROJ gelu_erf8
#endif
#ifndef DLWP_GELU8_TRUNK
#define DLWP_GELU8_TRUNK gelu_erf8
#endif

namespace dlwp {
namespace fno {

constexpr int kC = 32;          // hidden channels the kernels are specialised for
constexpr int kTrStride = 68;   // LDS row stride (floats) of the per-wave transpose tile

// ---------------------------------------------------------------------------------------------
// logical input tensor assembled from up to 4 channel segments (folds _prepare_inputs,
// fno.py:49-62, into the consumer's loads: no concat copy)
// ---------------------------------------------------------------------------------------------
struct ChanSeg {
  const float* ptr;     // channel 0 of sample 0
  long long bstride;    // elements between samples
  int nchan;            // channels in this segment (plane stride = H*W)
  int pad;
};
struct ChanTable {
  ChanSeg seg[4];
};

__device__ __forceinline__ const float* chan_ptr(const ChanTable& t, int c, int b, int HW) {
  const float* p = nullptr;
  int base = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = t.seg[i].nchan;
    if (c >= base && c < base + n)
      p = t.seg[i].ptr + (long long)b * t.seg[i].bstride + (long long)(c - base) * HW;
    base += n;
  }
  return p;
}

__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// Forward W-direction pruned DFT of a [NT*16 channels][64 pixels] tile held in the wave's LDS
// transpose area: yacc[ct][kt] += tile[ct] (16 x 64) * TT[w0.., kt] (64 x 16).
template <int NT, int KP>
__device__ __forceinline__ void fwd_dft_accumulate(const float* s_tr, const float* __restrict__ tt,
                                                   int w0, int lane, f32x4 (&yacc)[NT][KP / 16]) {
  const int j = lane & 15, g = lane >> 4;
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    float bt[KP / 16];
#pragma unroll
    for (int kt = 0; kt < KP / 16; ++kt) bt[kt] = tt[(long long)(w0 + 4 * s + g) * KP + kt * 16 + j];
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) {
      const float a = s_tr[(16 * ct + j) * kTrStride + 4 * s + g];
#pragma unroll
      for (int kt = 0; kt < KP / 16; ++kt) yacc[ct][kt] = mfma16x16x4(a, bt[kt], yacc[ct][kt]);
    }
  }
}

// Y layout [B][H][KP][C] (c fastest): one 16-byte store per (ct, kt) per lane.
template <int NT, int KP>
__device__ __forceinline__ void store_y(float* __restrict__ ybuf, long long row, int nchan, int lane,
                                        const f32x4 (&yacc)[NT][KP / 16], int c0 = 0) {
  const int j = lane & 15, g = lane >> 4;
#pragma unroll
  for (int ct = 0; ct < NT; ++ct)
#pragma unroll
    for (int kt = 0; kt < KP / 16; ++kt)
      *reinterpret_cast<f32x4*>(ybuf + (row * KP + kt * 16 + j) * nchan + c0 + 16 * ct + 4 * g) = yacc[ct][kt];
}

// ---------------------------------------------------------------------------------------------
// pointwise 2-layer channel MLP:  out = W2 * gelu(W1 * x + b1) + b2  (+ residual)
//   lifting   (neuralop FNO.lifting,    in -> 256 -> 32)  EMIT_Y: also the W-direction DFT of out
//   projection(neuralop FNO.projection, 32 -> 256 -> out) RESID: adds prognostic_t[:, -1]
// One wave = one grid row; per 64-pixel segment lane (j = l&15, g = l>>4) owns pixels 4j..4j+3
// (one 16-byte vector per channel) and k-slot g of every 4-deep MFMA step.
// ---------------------------------------------------------------------------------------------
struct MlpParams {
  ChanTable x;
  int hid;          // hidden width, multiple of 16
  int cout;         // real output channels
  const float* w1p; // [hid/16][CIN_STEPS][64]   A operands of layer 1
  const float* b1;  // [hid]
  const float* w2p; // [hid/16][4][COUT_TILES][64] A operands of layer 2
  const float* b2;  // [COUT_TILES*16]
  float* out;       // out + b*out_bstride + co*H*W + h*W + w
  long long out_bstride;
  const float* resid;
  long long resid_bstride;
  float* ybuf;      // [B][H][COUT_TILES*16][KP]
  const float* tt;  // TT[W][KP]
  int B, H, W;
};

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

// Lifting MLP of one 64-pixel row segment, bf16x6 layer 2 (see pw_lift_bf16x6_kernel): xs = the input channels
// (f32x4 per 4-deep k-step, rows 4 s + g), acc2[ot][q][r] = out[co = 16 ot + 4 g + r][pixel 4 j + q].
// ns = how many of the CIN_STEPS k-steps are populated (uniform; the fused step kernel is instantiated once for
// CIN_STEPS = 4 and runs any in_channels <= 16 with it).
template <int CIN_STEPS, bool F16 = false>
__device__ __forceinline__ void lift_segment(const f32x4 (&xs)[CIN_STEPS], const float* s_w1, const float* s_b1,
                                             const u32x4* s_w2, int npair, int lane, const f32x4 (&bias2)[2],
                                             f32x4 (&acc2)[2][4], int ns = CIN_STEPS, bool cin1 = false, float f16_up = 1.f,
                                             float f16_down = 1.f) {
  // F16: the three products of a layer-2 term sit at 2^(11+s) times the true scale (common.hpp; s = the shift the host packed
  // W2 with): the accumulators start from bias2 * f16_up and are multiplied by f16_down = 1 / f16_up when the last unit is in
  const int g = lane >> 4;
  // cin1 (ONE input channel, uniform): layer 1 is w1[c] * x + b1[c] -- 16 plain FMAs per unit instead of four fp32 matrix
  // instructions that would multiply three zero k-slots each (the fp32 MFMA holds the vector lanes for 32 cycles).  Bit-identical:
  // the matrix instruction is the same FMA chain with exact zeros added.  The channel's pixels sit in lane group g = 0;
  // the other groups hold zeros, so two xor-shuffles + adds broadcast them exactly.
  f32x4 xbc = {0.f, 0.f, 0.f, 0.f};
  if (cin1) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v = xs[0][q];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      xbc[q] = v;
    }
  }
#pragma unroll
  for (int ot = 0; ot < 2; ++ot)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc2[ot][q] = F16 ? bias2[ot] * f16_up : bias2[ot];

  // Software pipeline over units (tile pair u, pixel-chain pair qp): while the fp32 lanes do layer 1,
  // GELU and the 3-way bf16 split of unit n (-> B operands bg), the bf16 matrix pipe does layer 2 of
  // unit n-1.  Three slots per trip, 8 bf16 MFMAs each, fenced so hipcc keeps the interleave (an
  // in-order wave that issues its MFMAs back to back cannot issue VALU work meanwhile).
  // (every index into bg / acc2 / xs below is a compile-time constant: runtime-indexed register
  // arrays go to scratch)
  u32x4 bg0[2][3], bg1[2][3];   // ping-pong B operands: [q in pair][part]
  f32x4 a1[2][2];               // [tile in pair][q in pair]
  u32x4 wa[2][3];               // layer-2 A operands of the unit in flight on the matrix pipe
  const int nunit = npair * 2;  // unit n = (tile pair n >> 1, chain pair n & 1)
  auto unit_valu_fc1 = [&](int u, auto qpc) {
    constexpr int qp = decltype(qpc)::value;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      const int t = 2 * u + tt;
      const f32x4 bb = *reinterpret_cast<const f32x4*>(s_b1 + 16 * t + 4 * g);
      if (cin1) {   // s_w1 [tile][ns = 1][64]: lanes 0..15 of a tile hold w1[16 t + lane][0]
        const f32x4 wv = *reinterpret_cast<const f32x4*>(s_w1 + t * 64 + 4 * g);
#pragma unroll
        for (int qq = 0; qq < 2; ++qq)
#pragma unroll
          for (int r = 0; r < 4; ++r) a1[tt][qq][r] = __builtin_fmaf(wv[r], xbc[2 * qp + qq], bb[r]);
        continue;
      }
#pragma unroll
      for (int qq = 0; qq < 2; ++qq) a1[tt][qq] = bb;
#pragma unroll
      for (int s = 0; s < CIN_STEPS; ++s) {
        if (s >= ns) break;
        const float a = s_w1[(t * ns + s) * 64 + lane];
#pragma unroll
        for (int qq = 0; qq < 2; ++qq) a1[tt][qq] = mfma16x16x4(a, xs[s][2 * qp + qq], a1[tt][qq]);
      }
    }
  };
  auto unit_split = [&](u32x4(&bg)[2][3]) {
#pragma unroll
    for (int qq = 0; qq < 2; ++qq)
#pragma unroll
      for (int i = 0; i < 4; ++i) {   // dword i: k-slots 2i, 2i+1 -> tile i/2, registers 2(i%2), 2(i%2)+1
        unsigned hh, mm, ll;
        split_pair_x<F16>(a1[i / 2][qq][2 * (i % 2)], a1[i / 2][qq][2 * (i % 2) + 1], hh, mm, ll);
        bg[qq][0][i] = hh;
        bg[qq][1][i] = mm;
        bg[qq][2][i] = ll;
      }
  };
  auto load_wa = [&](int u) {
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
      for (int pp = 0; pp < 3; ++pp) wa[ot][pp] = s_w2[((u * 3 + pp) * 2 + ot) * 64 + lane];
  };
  // 8 of the 24 bf16 MFMAs of a unit: terms {2 slot, 2 slot + 1} of every (ot, q) accumulator,
  // smallest terms first: (l,h) (h,l) (m,m) (m,h) (h,m) (h,h)
  auto unit_mfma = [&](const u32x4(&bg)[2][3], auto qpc, auto slotc) {
    constexpr int qp = decltype(qpc)::value, slot = decltype(slotc)::value;
    if constexpr (F16) {   // one f16 term per slot, all at one scale: (wm', xh) (wh, xm') (whB, xh)
      constexpr int PA[3] = {1, 0, 2}, PB[3] = {0, 1, 0};
#pragma unroll
      for (int ot = 0; ot < 2; ++ot)
#pragma unroll
        for (int qq = 0; qq < 2; ++qq)
          acc2[ot][2 * qp + qq] = mfma16x16x32_f16(wa[ot][PA[slot]], bg[qq][PB[slot]], acc2[ot][2 * qp + qq]);
    } else {
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
    for (int term = 2 * slot; term < 2 * slot + 2; ++term)
#ifdef DLWP_KO_SPLIT
      if (term == 5)
#endif
#pragma unroll
      for (int ot = 0; ot < 2; ++ot)
#pragma unroll
        for (int qq = 0; qq < 2; ++qq)
          acc2[ot][2 * qp + qq] = mfma16x16x32_bf16(wa[ot][PA[term]], bg[qq][PB[term]], acc2[ot][2 * qp + qq]);
    }
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  // one trip: matrix pipe = layer 2 of the previous unit (chain pair QM, operands bgm),
  //           fp32 lanes  = layer 1 + GELU + split of this unit (chain pair QV -> bgv)
  auto trip = [&](int u_m, int u_v, const u32x4(&bgm)[2][3], u32x4(&bgv)[2][3], auto qm, auto qv) {
    load_wa(u_m);
    unit_valu_fc1(u_v, qv);
    unit_mfma(bgm, qm, I0{});
    DLWP_GELU8_LIFT(a1[0][0], a1[0][1]);
    __builtin_amdgcn_sched_barrier(0);
    unit_mfma(bgm, qm, I1{});
    DLWP_GELU8_LIFT(a1[1][0], a1[1][1]);
    __builtin_amdgcn_sched_barrier(0);
    unit_mfma(bgm, qm, I2{});
    unit_split(bgv);
    __builtin_amdgcn_sched_barrier(0);
  };
  // prologue: unit 0 (tile pair 0, chains 0-1) on the fp32 lanes only
  unit_valu_fc1(0, I0{});
  DLWP_GELU8_LIFT(a1[0][0], a1[0][1]);
  DLWP_GELU8_LIFT(a1[1][0], a1[1][1]);
  unit_split(bg0);
  for (int u = 0; u < npair; ++u) {
    trip(u, u, bg0, bg1, I0{}, I1{});                            // MFMA unit (u,0) | VALU unit (u,1)
    if (u + 1 < npair) trip(u, u + 1, bg1, bg0, I1{}, I0{});      // MFMA unit (u,1) | VALU unit (u+1,0)
  }
  load_wa(npair - 1);
  unit_mfma(bg1, I1{}, I0{});
  unit_mfma(bg1, I1{}, I1{});
  unit_mfma(bg1, I1{}, I2{});
  (void)nunit;
  if constexpr (F16) {
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc2[ot][q] *= f16_down;
  }

}

// ---------------------------------------------------------------------------------------------
// Lifting MLP of ONE input channel from a table.  With one input channel
//   lift(x)[o] = b2[o] + sum_c W2[o][c] gelu(w1[c] x + b1[c])
// is 32 smooth functions of one scalar.  The plan tabulates them once: per interval of width h = 2^-log2_inv_h over
// [-range, range) and output channel a quintic Hermite interpolant (f, f', f'' matched at both ends, fp64 with erfc),
// written in the coordinate v in [0, 1) measured from the interval's end NEARER zero -- so c0 = lift(knot) and the
// polynomial keeps its RELATIVE accuracy as x -> 0 (zero biases make lift(x) proportional to x there).
// Layout: fp32 [interval][coef 0..5][32 channels]; a lane's channels 4g.. and 16+4g.. are two 16-byte loads per coefficient.
// ---------------------------------------------------------------------------------------------
constexpr int kLiftTabRange = 32, kLiftTabLog2 = 4;   // the plans' table: 1024 intervals, 768 KB
constexpr int kLiftTabCoefs = 6;
constexpr int kLiftTabStride = kLiftTabCoefs * kC;    // floats per interval

// Interval of x and its coordinate v.  n_side = intervals per sign, scale = 1 / h (a power of two): |x| scale, its floor
// and their difference are all exact in fp32.  The caller has checked |x| < range; the index is clamped regardless.
__host__ __device__ __forceinline__ int lift_tab_locate(float x, int n_side, float scale, float& v) {
  const float a = fabsf(x) * scale;
  const float fl = floorf(a);
  v = a - fl;
  int k = (int)fl;
  k = k < 0 ? 0 : (k > n_side - 1 ? n_side - 1 : k);
  return x < 0.f ? n_side - 1 - k : n_side + k;
}

// Lifting output from the table: xbc = four pixel values, g = channel group; vv[ot][r][q] = channel 16 ot + 4 g + r of pixel q
// (the trunk's resident layout for the lane that holds these pixels).  Two pixels at a time: 24 loads in flight, then 2 x 8
// Horner chains.
__device__ __forceinline__ void lift_from_table(const float* __restrict__ tab, const f32x4& xbc, int g, f32x4 (&vv)[2][4]) {
#pragma unroll
  for (int qp = 0; qp < 2; ++qp) {
    f32x4 c[2][kLiftTabCoefs][2];
    float v[2];
#pragma unroll
    for (int qq = 0; qq < 2; ++qq) {
      const int idx = lift_tab_locate(xbc[2 * qp + qq], kLiftTabRange << kLiftTabLog2, (float)(1 << kLiftTabLog2), v[qq]);
      const f32x4* src = reinterpret_cast<const f32x4*>(tab + (size_t)idx * kLiftTabStride + 4 * g);
#pragma unroll
      for (int k = kLiftTabCoefs - 1; k >= 0; --k) {
        c[qq][k][0] = src[k * (kC / 4)];
        c[qq][k][1] = src[k * (kC / 4) + 4];
      }
    }
#pragma unroll
    for (int qq = 0; qq < 2; ++qq)
#pragma unroll
      for (int ot = 0; ot < 2; ++ot) {
        f32x4 acc = c[qq][kLiftTabCoefs - 1][ot];
#pragma unroll
        for (int k = kLiftTabCoefs - 2; k >= 0; --k)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[r] = __builtin_fmaf(acc[r], v[qq], c[qq][k][ot][r]);
#pragma unroll
        for (int r = 0; r < 4; ++r) vv[ot][r][2 * qp + qq] = acc[r];
      }
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

// Projection MLP of one 64-pixel row segment (see pw_proj_bf16x6_kernel): bx = the 32 input channels of the
// lane's 4 pixels as bf16x3 B operands (k order = whatever s_w1 was packed for), po[co][q] = this lane group's
// partial sum of output co at pixel 4 j + q (to be reduced over the 4 lane groups).
template <int CO, bool F16 = false>
__device__ __forceinline__ void proj_segment(const u32x4 (&bx)[4][3], const u32x4* s_w1, const float* s_b1,
                                             const float* s_w2, int ntile, int lane, float (&po)[CO][4], float f16_down = 1.f) {
  // F16: s_b1 holds b1 * 2^(11+s) and layer 1 comes out at that scale (common.hpp): one multiply per element in front of the GELU
  const int g = lane >> 4;
#pragma unroll
  for (int co = 0; co < CO; ++co)
#pragma unroll
    for (int q = 0; q < 4; ++q) po[co][q] = 0.f;
  auto fc1 = [&](int t, f32x4(&a1)[4]) {
    const f32x4 bb = *reinterpret_cast<const f32x4*>(s_b1 + 16 * t + 4 * g);
    u32x4 wa[3];
#pragma unroll
    for (int pp = 0; pp < 3; ++pp) wa[pp] = s_w1[(t * 3 + pp) * 64 + lane];
#pragma unroll
    for (int q = 0; q < 4; ++q) a1[q] = mfma_x<F16>(wa, bx[q], bb);
  };
  f32x4 a_cur[4], a_nxt[4], g_prev[4], g_new[4];
  fc1(0, a_cur);
  fc1(ntile > 1 ? 1 : 0, a_nxt);
#pragma unroll
  for (int q = 0; q < 4; ++q) g_prev[q] = F16 ? a_cur[q] * f16_down : a_cur[q];
  DLWP_GELU8_PROJ(g_prev[0], g_prev[1]);
  DLWP_GELU8_PROJ(g_prev[2], g_prev[3]);
#pragma unroll
  for (int q = 0; q < 4; ++q) a_cur[q] = a_nxt[q];
  // LDS operands are fetched ONE TILE AHEAD of the MFMAs / FMAs that consume them (the matrix instructions at the top
  // of an iteration would otherwise wait out the LDS latency every tile)
  u32x4 wa[3], wa_n[3];
  f32x4 w2v[CO], w2v_n[CO], bb, bb_n;
  {
    const int tn = ntile > 2 ? 2 : ntile - 1;
#pragma unroll
    for (int pp = 0; pp < 3; ++pp) wa[pp] = s_w1[(tn * 3 + pp) * 64 + lane];
#pragma unroll
    for (int co = 0; co < CO; ++co) w2v[co] = *reinterpret_cast<const f32x4*>(s_w2 + co * 16 + 4 * g);
    bb = *reinterpret_cast<const f32x4*>(s_b1 + 16 * tn + 4 * g);
  }
  for (int t = 1; t < ntile; ++t) {
    {   // operands of iteration t + 1: tile min(t + 2, ntile - 1) for layer 1, tile t for layer 2
      const int tn2 = (t + 2 < ntile) ? t + 2 : ntile - 1;
#pragma unroll
      for (int pp = 0; pp < 3; ++pp) wa_n[pp] = s_w1[(tn2 * 3 + pp) * 64 + lane];
#pragma unroll
      for (int co = 0; co < CO; ++co) w2v_n[co] = *reinterpret_cast<const f32x4*>(s_w2 + (t * CO + co) * 16 + 4 * g);
      bb_n = *reinterpret_cast<const f32x4*>(s_b1 + 16 * tn2 + 4 * g);
    }
    // two slots: the bf16 MFMAs of tile tn for two pixel chains (matrix pipe), then GELU of two
    // accumulator fragments of tile t and the layer-2 FMAs of tile t-1 (fp32 lanes)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      a_nxt[2 * i] = mfma_x<F16>(wa, bx[2 * i], bb);
      a_nxt[2 * i + 1] = mfma_x<F16>(wa, bx[2 * i + 1], bb);
      g_new[2 * i] = F16 ? a_cur[2 * i] * f16_down : a_cur[2 * i];
      g_new[2 * i + 1] = F16 ? a_cur[2 * i + 1] * f16_down : a_cur[2 * i + 1];
      DLWP_GELU8_PROJ(g_new[2 * i], g_new[2 * i + 1]);
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
#pragma unroll
    for (int pp = 0; pp < 3; ++pp) wa[pp] = wa_n[pp];
#pragma unroll
    for (int co = 0; co < CO; ++co) w2v[co] = w2v_n[co];
    bb = bb_n;
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
struct LayerParams {
  const float* x;     // [B][32][H][W]
  float* y;           // [B][32][H][W]
  const float* wsp;   // [8][2][64] packed skip weights (fp32 MFMA operands)
  const u32x4* wsb;   // [2 halves][3 parts][64] bf16x6 A operands of the skip weights, or null
  const float* bias;  // [32]
  const float* zbuf;  // [B][H][KP][32]
  const float* t;     // T[KP][W]
  const float* tt;    // TT[W][KP]
  float* ybuf;        // [B][H][32][KP]
  int B, H, W;
  int stagger;        // delay of waves 4-7 in units of s_sleep(32) = 2048 cycles
};

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

__device__ __forceinline__ float2 cfma(float2 a, float2 b, float2 c) {
  return float2{fmaf(a.x, b.x, fmaf(-a.y, b.y, c.x)), fmaf(a.x, b.y, fmaf(a.y, b.x, c.y))};
}

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

// ---------------------------------------------------------------------------------------------
// Fused trunk: ALL spectral layers of one backbone step in one launch (W = 64, H % 8 == 0, KP = 16).
//
// One workgroup = 8 consecutive grid rows of one sample, one wave per row; the G = H/8 workgroups of a
// sample form a group and every workgroup of the grid is resident at once (one per CU).  The hidden
// activation of a row (32 channels x 64 pixels) lives in 32 VGPRs of its wave from the first layer to the
// last: it is read from HBM/Infinity Cache once and written once per STEP instead of once per layer.
// What crosses workgroups is only the spectrum, M1 x M2 x 32 complex numbers per sample and layer:
//
//   per layer   P1  X_part[r][ky][c] = sum over this workgroup's 8 rows of EF[r][h] * Y[h][ky][c]   (MFMA, LDS)
//               -- group barrier --                 (X_part published with agent-scope sc1 stores)
//               P2  the group's M1*M2 modes are dealt out to its workgroups: sum the G partials,
//                   O[r][ky][o] = fwd_scale * sum_c X[r][ky][c] * Wt[ky][r][c][o]
//               -- group barrier --
//               P3  Z[h][ky][o] = ck[ky] * sum_r EI[r][h] * O[r][ky][o] for the 8 own rows          (MFMA -> LDS)
//               row y = act(bias + Wskip * x + Z * T)   skip conv on the bf16 pipe (bf16x6, B operand
//                   taken straight from the resident registers), inverse W-DFT on fp32 MFMA, packed GELU;
//                   forward W-DFT of the result -> Y row in LDS for the next layer
//
// The group barrier is an agent-scope counter: stores drained (s_waitcnt vmcnt(0)) + workgroup barrier,
// one lane adds and polls (bounded: a timeout poisons the output with NaN instead of hanging the GPU).
// Handed-off data is written and read with relaxed agent-scope atomics (sc1: write-through, L1 bypass);
// tools/ubench_groupsync.hip measures 1.3-1.6 us per barrier, 2.1 us with the payload when the group shares
// an XCD (workgroup i runs on XCD i % 8, so a sample's workgroups are i, i+8, ...).
// ---------------------------------------------------------------------------------------------
constexpr int kTrunkMaxLayers = 8;
// W-direction DFTs of the fused kernel's row phase on the bf16 matrix pipe (bf16x6) instead of fp32 MFMA.  Built,
// parity-green (rel-L2 3.7e-7 after 20 steps) and measured: NO gain (inverse 0.77 vs 0.88 us, forward 0.72 vs 0.76 us for
// the first wave of a SIMD, launch 1.891 vs 1.887 ms) -- K is only 16 / 64 deep, so the extra LDS reads, the operand
// splits and the six dependent MFMAs per accumulator cost what the freed fp32 lanes give back.  Default: the fp32 form
// (exact fp32 FMA chains); -DDLWP_TRUNK_DFT_BF16=1 rebuilds the bf16x6 form.
#ifndef DLWP_TRUNK_DFT_BF16
#define DLWP_TRUNK_DFT_BF16 0
#endif
constexpr bool kDftBf16 = DLWP_TRUNK_DFT_BF16 != 0;
// f16x3 step kernel: the two W-direction DFTs of the row phase on the f16 matrix instructions too (data split on the fly,
// twiddles pre-split).  The bf16x6 attempt above was a wash (six dependent products + 11-slot splits); f16x3 halves both.
#ifndef DLWP_F16_DFT
#define DLWP_F16_DFT 1
#endif
#ifndef DLWP_PREFETCH_EARLY
#define DLWP_PREFETCH_EARLY 0   // measured: 1 (the next step's lifting weights requested BEFORE the projection) spills 38 registers
#endif                          // per lane and loses 8 % (1.501 vs 1.385 ms per rollout); 0 = right before the end-of-step barrier
// f16x3 products of the trunk's row phase (skip convolution + inverse W-DFT into ONE accumulator, forward W-DFT): the skip
// weights and the twiddles are packed with the SAME shift s = 3 (twiddles: max |t| = 1 -> [8, 16); skip weights must stay below 2,
// checked when the plan is made -- a plan with larger ones takes the bf16x6 form), so everything sits at 2^14 times the true scale
constexpr int kTrunkF16Shift = 3;
constexpr float kTrunkF16Up = 16384.0f, kTrunkF16Down = 1.0f / 16384.0f;
// Seam between two steps of the fused kernel when the lifting MLP is read from the plan's table:
// the exact path's weights are staged only in a step in which some wave of the workgroup falls back to it (the "vote").
// A/B switches (tools/ab_build.sh): -DDLWP_LIFT_STAGE_ALWAYS = the earlier seam (request before the end-of-step barrier, LDS
// write and a second barrier behind it, a third one behind the lifting); -DDLWP_LIFT_GATHER_EARLY = a wave gathers its
// next row from the table BEFORE the barrier of the seam (tried: 304 instead of 184 bytes of scratch per lane).
#if defined(DLWP_LIFT_STAGE_ALWAYS) || defined(DLWP_NO_LIFT_TABLE)
constexpr bool kLiftVote = false;
#else
constexpr bool kLiftVote = true;
#endif
#ifdef DLWP_LIFT_GATHER_EARLY
constexpr bool kLiftGatherEarly = true;
#else
constexpr bool kLiftGatherEarly = false;
#endif
constexpr int kSyStride = 528;   // floats per Y row in LDS: 16 k' x 32 c + 16 (bank spread for the P1 B reads)

struct TrunkParams {
  const float* x;      // [B][32][H][64] hidden activation from the lifting kernel
  float* y;            // [B][32][H][64] output for the projection kernel
  const float* ybuf;   // [B][H][16][32] W-direction DFT of x (emitted by the lifting kernel)
  const float* t;      // T[16][64]
  const float* tt;     // TT[64][16]
  const u32x4* tb;     // [4 q][3][64]   bf16x3 B operands of the inverse W-DFT
  const u32x4* ttb;    // [2 kb][3][64]  bf16x3 B operands of the forward W-DFT
  const float2* ef;    // [M1][H]
  const float2* ei;    // [M1][H]
  const float* ck;     // [M2]
  const u32x4* wsb[kTrunkMaxLayers];   // skip weights, bf16x3 A operands with the k order of the resident layout
  const float* bias[kTrunkMaxLayers];
  const float2* wt[kTrunkMaxLayers];   // [M2][M1][32][32]
  float* xpart;        // [S][G][M2][M1][2][32]
  float* obuf;         // [S][M2][M1][2][32]
  long long xpart_par, obuf_par;   // LL protocol: distance (floats) to the second (odd-layer) copy of each buffer
  unsigned layer0;     // LL protocol: spectral layers already run on these buffers since they were armed
  unsigned* xcc_tab;   // LL protocol: [S][32] (tag << 4 | XCC id) of every workgroup of a sample's group
  unsigned* ctr;       // one counter per sample, 32 dwords apart
  unsigned epoch;      // barriers already counted on these counters
  float fwd_scale;
  int S, H, L, M1, M2, G, sample0;
  unsigned long long* trace;   // diagnostics (DLWP_TRUNK_TRACE): [workgroup][64] s_memrealtime stamps, or null
  int trace_tid;               // the thread that stamps (DLWP_TRUNK_TRACE_WAVE * 64)
  // STEP variant (lifting and projection inside the same launch):
  ChanTable in;            // the step's input channels (folds _prepare_inputs)
  int lift_ns, lift_hid;   // populated 4-deep k-steps of the input (<= 4), lifting width (<= 256, multiple of 32)
  int lift_cin1;           // exactly one input channel: lifting layer 1 as plain FMAs (lift_segment)
  const float* lift_w1p;   // [hid/16][ns][64]
  const float* lift_b1;    // [hid]
  const u32x4* lift_w2b;   // [hid/32][3][2][64]
  const float* lift_b2;    // [32]
  const float* lift_tab;   // one input channel: the lifting MLP tabulated (lift_from_table), or null = evaluate it (lift_segment)
  float lift_up, lift_down, proj_up, proj_down;   // f16x3 form: 2^(11+s) of the lifting W2 / projection W1 images and its inverse
  int proj_hid, proj_co, cout;   // projection width (<= 256), outputs the FMA layer 2 is built for (1, 2, 4), real outputs
  const u32x4* proj_w1b;   // [hid/16][3][64], k order of the resident activation
  const float* proj_b1;    // [hid]
  const float* proj_w2v;   // [hid/16][proj_co][16]
  const float* proj_b2;    // [16]
  float* out;              // out + b * out_bstride + co * H * W
  long long out_bstride;
  const float* resid;      // or null
  long long resid_bstride;
  // several steps in this launch (n_steps > 1): the per-step tables above are rebuilt on the device from
  const float* r_const;    // constants  [B, 1, n_const, H, W] or null
  const float* r_presc;    // prescribed [B, T, n_presc, H, W] or null
  const float* r_prog;     // prognostic [B, T, n_prog, H, W]
  float* r_out;            // out        [B, T - ctx, n_prog, H, W]
  int r_nconst, r_npresc, r_nprog, r_T, r_ctx, r_t0;   // first time index of this launch (ctx + step_begin)
  int feed_regs;           // n_steps > 1, no constants / prescribed channels, context 1, <= 4 prognostic channels: a step's whole
                           // input (and its residual) is the output the SAME lanes have just computed -- it stays in registers
  int n_steps;             // 0 / 1: one step described by in / out / resid
  // hand-off bounds (plan knobs): polls of a counter barrier / re-loads of a flag-in-data block before the workgroup
  // gives up; a workgroup that gives up poisons its outputs with NaN AND sets *fail_word (checked by the host)
  int spin_limit, try_limit;
  unsigned* fail_word;     // workspace word, zeroed at the start of every call (per-call check)
  unsigned* sticky_fails;  // plan-owned counter, only reset by dlwp_fno2d_status (deferred check of asynchronous calls)
};

__device__ __forceinline__ void trunk_group_barrier(unsigned* ctr, unsigned target, int* s_fail, int spin_limit) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_waitcnt(0);   // this wave's sc1 stores have reached the coherence point
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int spins = 0;
    while ((int)(__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) < 0) {
      __builtin_amdgcn_s_sleep(1);
      if (++spins > spin_limit) {   // default ~ 0.1 s: a peer workgroup never arrived; give up loudly, never hang
        *s_fail = 1;
        break;
      }
    }
  }
  __syncthreads();
}

// Split form: arrive (stores drained, one lane adds) ... independent work ... wait.
__device__ __forceinline__ void trunk_group_arrive(unsigned* ctr) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void trunk_group_wait(unsigned* ctr, unsigned target, int* s_fail, int spin_limit) {
  if (threadIdx.x == 0) {
    int spins = 0;
    while ((int)(__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) < 0) {
      __builtin_amdgcn_s_sleep(1);
      if (++spins > spin_limit) {
        *s_fail = 1;
        break;
      }
    }
  }
  __syncthreads();
}

__device__ __forceinline__ float ld_sc1(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_sc1(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Four independent 16-byte agent-scope (sc1: L1 bypass) loads in flight at once, then one wait.  hipcc puts
// `s_waitcnt vmcnt(0)` behind EVERY relaxed atomic load, which turned the 12-16 hand-off loads of a phase into
// as many serialized round trips to the Infinity Cache (first version of this kernel: P2 4.3 us, P3 2.9 us).
__device__ __forceinline__ void ld4_sc1_x4(const float* base, unsigned o0, unsigned o1, unsigned o2, unsigned o3,
                                           f32x4& v0, f32x4& v1, f32x4& v2, f32x4& v3) {
  // s_nop 4: the base may have just been restored into SGPRs by v_readlane / v_readfirstlane (SGPR spills), and a
  // VALU-written SGPR needs 5 wait states before a VMEM instruction reads it; the compiler's hazard recognizer
  // does not look inside inline asm (a build without this faulted with a garbage address).
  asm volatile(
      "s_nop 4\n\t"
      "global_load_dwordx4 %0, %4, %8 sc1\n\t"
      "global_load_dwordx4 %1, %5, %8 sc1\n\t"
      "global_load_dwordx4 %2, %6, %8 sc1\n\t"
      "global_load_dwordx4 %3, %7, %8 sc1\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3)
      : "v"(o0), "v"(o1), "v"(o2), "v"(o3), "s"(base)
      : "memory");
}
// Flag-in-data hand-off ("LL" protocol): the exchange buffers are armed with a sentinel bit pattern (a quiet NaN with a
// payload no arithmetic produces); a consumer re-loads until none of the dwords it needs is the sentinel, so the data
// itself is the flag: no store drain, no counter round trip, no workgroup barrier on the producer side.
constexpr unsigned kSentinel = 0x7fc0deadu;
__device__ __forceinline__ bool has_sentinel(const f32x4& v) {
  return __float_as_uint(v[0]) == kSentinel || __float_as_uint(v[1]) == kSentinel ||
         __float_as_uint(v[2]) == kSentinel || __float_as_uint(v[3]) == kSentinel;
}
// The closing `s_nop 1`: a 16-byte store reads its data registers late, and the compiler -- which sees the statement as one
// opaque instruction -- may overwrite them in the very next instruction (cdna_hip_programming.md 5.7 item 1).  Found in
// this file by tools/asm_hazard_check.py (rule C) in round 2: the re-arming sentinel stores were followed one wait state
// later by a VALU write to one of the four data registers.
__device__ __forceinline__ void st4_sc1(const float* base, unsigned off, const f32x4& v) {
  asm volatile("s_nop 4\n\tglobal_store_dwordx4 %0, %1, %2 sc1\n\ts_nop 1" : : "v"(off), "v"(v), "s"(base) : "memory");
}
__device__ __forceinline__ void st4_l2(const float* base, unsigned off, const f32x4& v) {   // stays in this XCD's L2
  asm volatile("s_nop 4\n\tglobal_store_dwordx4 %0, %1, %2\n\ts_nop 1" : : "v"(off), "v"(v), "s"(base) : "memory");
}
// Exchange stores of the flag-in-data protocol.  `fast` = every workgroup of the sample's group was FOUND to sit on the
// same XCD (HW_REG_XCC_ID exchanged during the first layer): a plain store keeps the line in that XCD's L2, where the
// group's L1-bypassing (sc1) loads hit it after ~0.2 us instead of going to the Infinity Cache (~0.9 us round trip).
// Otherwise the write-through sc1 form that is correct across XCDs.
__device__ __forceinline__ void st_xchg(float* p, float v, bool fast) {
  if (fast) *p = v;   // (not volatile: hipcc turns volatile stores into sc0 sc1 + a wait each, 6x slower)
  else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains vmcnt, i.e. it would wait for the
// weight prefetches that are meant to stay in flight across the barrier.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
__device__ __forceinline__ f32x4 shfl_xor4(f32x4 v, int m) {
  return f32x4{__shfl_xor(v[0], m), __shfl_xor(v[1], m), __shfl_xor(v[2], m), __shfl_xor(v[3], m)};
}

// ROWS = grid rows (= waves) per workgroup, G = workgroups per sample = H / ROWS (see trunk_rows() for the choice).
// Input table / output slot / residual of rollout step t, exactly as fno_rollout_impl builds them on the host
// (fno.py:49-62, :79-103): window of constants, prescribed[t-ctx:t], prognostic frames still taken from the input,
// then frames already produced.
__device__ __forceinline__ void rollout_step_io(const TrunkParams& p, int t, long long HW, ChanTable& in, float*& out,
                                                long long& out_bs, const float*& resid, long long& resid_bs) {
  const int T = p.r_T, ctx = p.r_ctx, To = T - ctx;
  const long long prog_bs = (long long)T * p.r_nprog * HW;
  out_bs = (long long)To * p.r_nprog * HW;
  int k = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) in.seg[i] = ChanSeg{nullptr, 0, 0, 0};
  if (p.r_nconst) in.seg[k++] = ChanSeg{p.r_const, (long long)p.r_nconst * HW, p.r_nconst, 0};
  if (p.r_npresc)
    in.seg[k++] = ChanSeg{p.r_presc + (long long)(t - ctx) * p.r_npresc * HW, (long long)T * p.r_npresc * HW, p.r_npresc * ctx, 0};
  const int f0 = t - ctx;
  const int n_in = (f0 < ctx) ? (ctx - f0 < ctx ? ctx - f0 : ctx) : 0;
  if (n_in > 0) in.seg[k++] = ChanSeg{p.r_prog + (long long)f0 * p.r_nprog * HW, prog_bs, p.r_nprog * n_in, 0};
  if (ctx - n_in > 0) {
    const int fo = f0 + n_in - ctx;
    in.seg[k++] = ChanSeg{p.r_out + (long long)fo * p.r_nprog * HW, out_bs, p.r_nprog * (ctx - n_in), 0};
  }
  if (t - 1 < ctx) { resid = p.r_prog + (long long)(t - 1) * p.r_nprog * HW; resid_bs = prog_bs; }
  else { resid = p.r_out + (long long)(t - 1 - ctx) * p.r_nprog * HW; resid_bs = out_bs; }
  out = p.r_out + (long long)(t - ctx) * p.r_nprog * HW;
}

// STEP: the whole backbone step in this launch -- the lifting MLP produces the resident activation and its first Y row,
// the projection MLP (+ residual) consumes the last one; their staged weights time-share the transpose tiles' LDS.
// Forward W-direction DFT of the wave's 32 x 64 tile in its transpose area, bf16x6: A = 8 consecutive pixels of a channel
// row (two 16-byte LDS reads, split into three bf16 parts), B = the pre-split twiddles.
template <bool F16 = false>
__device__ __forceinline__ void fwd_dft_bf16x6(const float* s_tr, const u32x4* s_ttb, int lane, f32x4 (&yacc)[2]) {
  const int j = lane & 15, g = lane >> 4;
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
    u32x4 tb[3];
#pragma unroll
    for (int pp = 0; pp < 3; ++pp) tb[pp] = s_ttb[(kb * 3 + pp) * 64 + lane];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const float* src = s_tr + (16 * ct + j) * kTrStride + 32 * kb + 8 * g;
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(src), a1 = *reinterpret_cast<const f32x4*>(src + 4);
      u32x4 xa[3];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        unsigned hh, mm, ll;
        const float v0 = i < 2 ? a0[2 * i] : a1[2 * i - 4], v1 = i < 2 ? a0[2 * i + 1] : a1[2 * i - 3];
        split_pair_x<F16>(v0, v1, hh, mm, ll);
        xa[0][i] = hh;
        xa[1][i] = mm;
        xa[2][i] = ll;
      }
      if constexpr (F16) {   // data on the A side, 2^(11+3) times the true scale (kTrunkF16Down): (xh, tm') (xm', th) (xh, thB)
        yacc[ct] = mfma16x16x32_f16(xa[0], tb[1], yacc[ct]);
        yacc[ct] = mfma16x16x32_f16(xa[1], tb[0], yacc[ct]);
        yacc[ct] = mfma16x16x32_f16(xa[0], tb[2], yacc[ct]);
      } else {
        yacc[ct] = mfma_bf16x6(xa, tb, yacc[ct]);
      }
    }
  }
}

template <int ROWS, int G, bool LL, bool STEP = false, bool F16 = false>
__global__ __launch_bounds__(64 * ROWS, 2) void fno_trunk_kernel(const TrunkParams p) {
  extern __shared__ __align__(16) float smem[];
  constexpr int W = 64, KP = 16, C = kC, NT = 64 * ROWS;
  constexpr bool kDftF16 = F16 && (DLWP_F16_DFT != 0);
  static_assert(!F16 || kDftF16, "f16x3: the skip convolution and the inverse W-DFT share one SCALED accumulator (common.hpp)");
  constexpr bool kDftMx = kDftBf16 || kDftF16;            // W-direction DFTs on the bf16 / f16 matrix instructions
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, g = lane >> 4;
  float* s_tr = smem + wave * (C * kTrStride);            // [8][32][68]   per-wave transpose tile
  float* s_y = smem + ROWS * C * kTrStride;               // [ROWS][528]   Y rows of this workgroup
  float* s_z = s_y + ROWS * kSyStride;                    // [ROWS][16][32] Z rows of this workgroup
  float* s_x = s_z + ROWS * KP * C;                       // [ROWS][2][64] per-wave reduced X of two modes
  float* s_t = s_x + ROWS * 128;                             // [16][64]      T  (inverse W-DFT twiddles)
  float* s_tt = s_t + KP * W;                             // [64][16]      TT (forward W-DFT twiddles)
  int* s_fail = reinterpret_cast<int*>(s_tt + W * KP);
  int* s_fast = s_fail + 1;                               // LL: the sample's group shares one XCD (found in layer 0)
  int* s_lflag = s_fail + 2;                              // STEP: [2] some wave evaluates the exact lifting MLP (by step parity)
  float2* s_ef = reinterpret_cast<float2*>(s_fail + 4);   // [16][ROWS]  EF rows of this workgroup's grid rows (0 beyond M1)
  float2* s_ei = s_ef + 16 * ROWS;                        // [16][ROWS]  EI likewise
  u32x4* s_tb = reinterpret_cast<u32x4*>(s_ei + 16 * ROWS);   // [4][3][64]  inverse W-DFT B operands (bf16x3)
  u32x4* s_ttb = s_tb + 4 * 3 * 64;                           // [2][3][64]  forward W-DFT B operands (bf16x3)
  const int H = p.H, M1 = p.M1, M2 = p.M2, NM = M1 * M2;
  int sample, member;
  {
    const int i = blockIdx.x;
    if ((p.S & 7) == 0) {          // a sample's workgroups share an XCD (workgroup i -> XCD i % 8)
      const int slot = i >> 3;
      sample = (i & 7) + 8 * (slot / G);
      member = slot % G;
    } else {
      sample = i / G;
      member = i % G;
    }
  }
  const int h = member * ROWS + wave;
  const long long HW = (long long)H * W;
  const int gs = p.sample0 + sample;                      // sample index in the activation tensors
  const long long pix = (long long)h * W + 4 * j;
  unsigned* ctr = p.ctr + sample * 32;
  if (tid == 0) {
    *s_fail = 0;
    *s_fast = 0;
    s_lflag[0] = s_lflag[1] = 0;
    if (LL) {
      const unsigned xcc = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11)) & 0xFu;   // HW_REG_XCC_ID
      __hip_atomic_store(p.xcc_tab + sample * 32 + member, ((p.layer0 + 1u) << 4) | xcc, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  for (int i = tid; i < ROWS * KP * C; i += NT) s_z[i] = 0.f;   // k' slots beyond 2*M2 stay zero
  for (int i = tid; i < KP * W; i += NT) {
    s_t[i] = p.t[i];
    s_tt[i] = p.tt[i];
  }
  for (int i = tid; i < 16 * ROWS; i += NT) {   // the persistent form re-derives its MFMA operands from these every step
    const int r = i / ROWS, hl = i % ROWS;
    s_ef[i] = r < M1 ? p.ef[r * H + member * ROWS + hl] : float2{0.f, 0.f};
    s_ei[i] = r < M1 ? p.ei[r * H + member * ROWS + hl] : float2{0.f, 0.f};
  }
  for (int i = tid; i < 4 * 3 * 64; i += NT) s_tb[i] = p.tb[i];
  for (int i = tid; i < 2 * 3 * 64; i += NT) s_ttb[i] = p.ttb[i];
  lds_barrier();   // the tables above are read by every wave right away

  // STEP: the steps of this launch (one, or a whole rollout range without the host in the loop: a row's next input
  // is what the same wave has just written, so steps need no synchronisation beyond the spectrum hand-offs)
  int n_stamp = 0;
  const int n_steps = (STEP && p.n_steps > 1) ? p.n_steps : 1;
  f32x4 vfeed = {0.f, 0.f, 0.f, 0.f};   // feed_regs: the previous step's output of this lane (channel g, pixels 4j..4j+3)
  // no live table: the lifting weights of the NEXT step are requested before the end-of-step barrier and written to LDS
  // behind it (staged = they are already there when the step starts)
  bool staged = false;
  for (int st = 0; st < n_steps; ++st) {
  // Everything lane-dependent is re-derived from an OPAQUE copy of the thread index inside the step loop: otherwise
  // hipcc hoists the step-invariant address arithmetic and MFMA operands of all phases out of the loop, keeps them
  // live across the lifting MLP and spills ~160 VGPRs per lane to scratch (664 bytes/lane in the first version).
  int tid_o = threadIdx.x;
  asm volatile("" : "+v"(tid_o));
  const int tid = tid_o, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  float* s_tr = smem + wave * (C * kTrStride);
  const int h = member * ROWS + wave;
  const long long pix = (long long)h * W + 4 * j;
  ChanTable in = p.in;
  float* out_p = p.out;
  long long out_bs = p.out_bstride, resid_bs = p.resid_bstride;
  const float* resid_p = p.resid;
  if (STEP && p.n_steps > 1) rollout_step_io(p, p.r_t0 + st, HW, in, out_p, out_bs, resid_p, resid_bs);
  // resident activation: vv[ot][r] = channel 16 ot + 4 g + r, pixels 4j..4j+3
  f32x4 vv[2][4];
  if constexpr (STEP) {
    // ---- lifting: weights staged where the transpose tiles will live (they are not needed before the first DFT)
    if (p.trace && tid == p.trace_tid && n_stamp < 64) p.trace[blockIdx.x * 64 + n_stamp++] = __builtin_amdgcn_s_memrealtime();
    const int ntile_l = p.lift_hid >> 4, npair = ntile_l >> 1;
    u32x4* l_w2 = reinterpret_cast<u32x4*>(smem);                          // [npair][3][2][64]
    float* l_w1 = reinterpret_cast<float*>(l_w2 + npair * 6 * 64);         // [ntile][ns][64]
    float* l_b1 = l_w1 + ntile_l * p.lift_ns * 64;                         // [hid]
    auto lift_stage = [&]() {
      for (int i = tid; i < npair * 6 * 64; i += NT) l_w2[i] = p.lift_w2b[i];
      for (int i = tid; i < ntile_l * p.lift_ns * 64; i += NT) l_w1[i] = p.lift_w1p[i];
      for (int i = tid; i < p.lift_hid; i += NT) l_b1[i] = p.lift_b1[i];
    };
    auto lift_stage_voted = [&]() {   // the same copy, rolled: rare, its latency is exposed anyway, and the step's input is live
#pragma unroll 1
      for (int i = tid; i < npair * 6 * 64; i += NT) l_w2[i] = p.lift_w2b[i];
#pragma unroll 1
      for (int i = tid; i < ntile_l * p.lift_ns * 64; i += NT) l_w1[i] = p.lift_w1p[i];
#pragma unroll 1
      for (int i = tid; i < p.lift_hid; i += NT) l_b1[i] = p.lift_b1[i];
    };
    // vote: with a live table the exact path's weights are staged only in a step in which some wave of the workgroup
    // falls back to it.  Every wave knows its next input row BEFORE the barrier of the step seam (the one that ends the
    // previous projection's reads of this LDS region), so a wave that will fall back raises a flag in front of that barrier
    // and every wave reads it behind it.  No flag: no weight request, no LDS write, and this barrier is the only one
    // between the projection and the transpose tiles.  Two flag words alternate by step: the word of step s is written
    // before and read behind the seam barrier of step s, and cleared behind the seam barrier of step s - 1 -- the
    // barriers of the spectral layers and of the projection lie between that clear and the next write.
    const bool vote = kLiftVote && p.lift_tab != nullptr;
    if (!vote && !staged) lift_stage();
    f32x4 xs[4];
    if (p.feed_regs && st > 0) {
      xs[0] = vfeed;
#pragma unroll
      for (int s = 1; s < 4; ++s) xs[s] = f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float* cp = s < p.lift_ns ? chan_ptr(in, 4 * s + g, gs, (int)HW) : nullptr;
        xs[s] = cp ? *reinterpret_cast<const f32x4*>(cp + pix) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    f32x4 bias2[2];
    bias2[0] = *reinterpret_cast<const f32x4*>(p.lift_b2 + 4 * g);
    bias2[1] = *reinterpret_cast<const f32x4*>(p.lift_b2 + 16 + 4 * g);
    // One input channel and a table from the plan: the wave reads lift(x) from it when EVERY pixel of its row lies inside the
    // table's domain (one ballot; NaN and +-inf fail the test) and evaluates the MLP as before otherwise -- the decision
    // depends on the row's own data only, and no load address is formed from an unchecked x.
    bool from_table = false;
    f32x4 xp = {0.f, 0.f, 0.f, 0.f};
    auto lift_pick = [&]() {
      // The gather runs in a PERMUTED lane order: lane 4 j' + g' reads what resident lane (j', g') needs, so the four lanes
      // of a pixel are neighbours and their 16-byte loads cover 64 contiguous bytes of one line (one tag look-up instead of
      // four: in the resident order every lane of a 16-lane pass touched a line of its own and the phase ran at the L1's
      // look-up rate, 11 us instead of the 2.6 us its bytes need).  The channel's pixels sit in lane group g = 0.
      bool inside = true;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        xp[q] = __shfl(xs[0][q], lane >> 2);
        inside = inside && (fabsf(xp[q]) < (float)kLiftTabRange);
      }
      from_table = __all(inside) != 0;
    };
    auto lift_gather = [&]() {
      f32x4 vp[2][4];
      lift_from_table(p.lift_tab, xp, lane & 3, vp);
#pragma unroll
      for (int ot = 0; ot < 2; ++ot)   // back to the resident order: lane (j, g) takes its values from lane 4 j + g
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int q = 0; q < 4; ++q) vv[ot][r][q] = __shfl(vp[ot][r][q], 4 * j + g);
    };
    auto lift_exact = [&]() {
      f32x4 acc2[2][4];
      lift_segment<4, F16>(xs, l_w1, l_b1, l_w2, npair, lane, bias2, acc2, p.lift_ns, p.lift_cin1 != 0, p.lift_up, p.lift_down);
#pragma unroll
      for (int ot = 0; ot < 2; ++ot)
#pragma unroll
        for (int r = 0; r < 4; ++r) vv[ot][r] = f32x4{acc2[ot][0][r], acc2[ot][1][r], acc2[ot][2][r], acc2[ot][3][r]};
    };
#define DLWP_LIFT_STAMP()                                                                              \
  do {                                                                                                 \
    if (p.trace && tid == p.trace_tid && n_stamp < 64) p.trace[blockIdx.x * 64 + n_stamp++] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
    if (vote) {
      lift_pick();
      if (!from_table) s_lflag[st & 1] = 1;
    }
    if (kLiftGatherEarly && vote && from_table) {
      // The gather needs no LDS: a wave that is early runs it while the slower waves finish their projection.  (A branch
      // of its own, with the same barriers as the other one: in a shared one vv would stay live across lift_exact.)
      lift_gather();
      DLWP_LIFT_STAMP();
      lds_barrier();   // the seam: every wave is done with the projection weights, every flag of this step is up
      DLWP_LIFT_STAMP();
      const bool fallback = __builtin_amdgcn_readfirstlane(s_lflag[st & 1]) != 0;
      if (tid == 0) s_lflag[(st + 1) & 1] = 0;
      if (fallback) {   // other waves of the workgroup evaluate the MLP: help to stage its weights, wait until they are done
        lift_stage_voted();
        lds_barrier();
        lds_barrier();
      }
      DLWP_LIFT_STAMP();
    } else {
      bool weights_used = true;   // the exact path's weights are in LDS (or on their way) and some wave may read them
      if (vote) {
        DLWP_LIFT_STAMP();
        lds_barrier();   // the seam: every wave is done with the projection weights, every flag of this step is up
        weights_used = __builtin_amdgcn_readfirstlane(s_lflag[st & 1]) != 0;
        if (tid == 0) s_lflag[(st + 1) & 1] = 0;
      }
      if (vote && weights_used) lift_stage_voted();
      if (weights_used) lds_barrier();
      DLWP_LIFT_STAMP();
#if defined(DLWP_LIFT_STAGE_ALWAYS) && !defined(DLWP_NO_LIFT_TABLE)
      if (p.lift_tab) lift_pick();
#endif
      if (!from_table) lift_exact();
      else if (!kLiftVote || !kLiftGatherEarly) lift_gather();
      if (!vote) DLWP_LIFT_STAMP();
      if (weights_used) lds_barrier();   // every wave is done with the lifting weights: the region turns into transpose tiles
      DLWP_LIFT_STAMP();
    }
#undef DLWP_LIFT_STAMP
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        *reinterpret_cast<f32x4*>(s_tr + (16 * ot + 4 * g + r) * kTrStride + 4 * j) = vv[ot][r];
    wave_lds_fence();
    f32x4 yacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    if constexpr (kDftMx) {
      fwd_dft_bf16x6<kDftF16>(s_tr, s_ttb, lane, yacc);
    } else {
#pragma unroll
      for (int s = 0; s < 16; ++s)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
          yacc[ct] = mfma16x16x4(s_tr[(16 * ct + j) * kTrStride + 4 * s + g], s_tt[(4 * s + g) * KP + j], yacc[ct]);
    }
    wave_lds_fence();
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
      *reinterpret_cast<f32x4*>(s_y + wave * kSyStride + j * C + 16 * ct + 4 * g) = kDftF16 ? yacc[ct] * kTrunkF16Down : yacc[ct];
    if (p.trace && tid == p.trace_tid && n_stamp < 64) p.trace[blockIdx.x * 64 + n_stamp++] = __builtin_amdgcn_s_memrealtime();
  } else {
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        vv[ot][r] = *reinterpret_cast<const f32x4*>(p.x + ((long long)gs * C + 16 * ot + 4 * g + r) * HW + pix);
    const float* yr = p.ybuf + ((long long)gs * H + h) * KP * C;
#pragma unroll
    for (int u = 0; u < 2; ++u)
      *reinterpret_cast<f32x4*>(s_y + wave * kSyStride + 4 * lane + 256 * u) =
          *reinterpret_cast<const f32x4*>(yr + 4 * lane + 256 * u);
  }
  // loop-invariant operands
  constexpr int KS1 = ROWS / 2;   // k-steps of P1: K = (ROWS rows) x (re, im)
  float a_re[KS1], a_im[KS1];   // P1: A[(r = j)][k = (hl, ri)], hl = 2s + (g >> 1), ri = g & 1
#pragma unroll
  for (int s = 0; s < KS1; ++s) {
    const int hl = 2 * s + (g >> 1);
    float2 e = {0.f, 0.f};
    if (j < M1) e = s_ef[j * ROWS + hl];
    a_re[s] = (g & 1) ? -e.y : e.x;
    a_im[s] = (g & 1) ? e.x : e.y;
  }
  float a3[8];              // P3: A[m = (hl = j >> 1, ro = j & 1)][k = (r, ri)], r = 2s + (g >> 1), ri = g & 1
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const int r = 2 * s + (g >> 1);
    float2 e = {0.f, 0.f};
    if (r < M1 && (j >> 1) < ROWS) e = s_ei[r * ROWS + (j >> 1)];
    a3[s] = (j & 1) ? ((g & 1) ? e.x : e.y) : ((g & 1) ? -e.y : e.x);
  }
  const int ks3 = (2 * M1 + 3) / 4;
  const int per = (NM + G - 1) / G;                       // modes per workgroup in P2
  const int m_lo = member * per, m_hi = (m_lo + per < NM) ? m_lo + per : NM;
  // LL: the exchange buffers exist twice (layer parity), p.xpart / p.obuf point at parity 0 and the second copy
  // lies p.xpart_par / p.obuf_par floats further
  float* xp_mine0 = p.xpart + ((long long)sample * G + member) * NM * 64;
  const float* xp_grp0 = p.xpart + (long long)sample * G * NM * 64;
  float* ob0 = p.obuf + (long long)sample * NM * 64;
  unsigned target = p.epoch * (unsigned)G;

#define DLWP_STAMP()                                                                                   \
  do {                                                                                                 \
    if (p.trace && tid == p.trace_tid && n_stamp < 64) p.trace[blockIdx.x * 64 + n_stamp++] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
  DLWP_STAMP();

  for (int l = 0; l < p.L; ++l) {
    const int par = LL ? (int)((p.layer0 + (unsigned)(st * p.L + l)) & 1u) : 0;
    float* xp_mine = xp_mine0 + par * p.xpart_par;
    const float* xp_grp = xp_grp0 + par * p.xpart_par;
    float* ob = ob0 + par * p.obuf_par;
    float* ob_other = ob0 + (par ^ 1) * p.obuf_par;
    if (LL) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's re-arming stores of the previous layer are done
    const bool fast = LL && (l > 0 || st > 0) && (*s_fast != 0);
    // operands that do not depend on data are requested before the barriers: the skip weights / bias of the row
    // phase and the weights of this wave's first two modes
    u32x4 wb[2][3];
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
      for (int pp = 0; pp < 3; ++pp) wb[ot][pp] = p.wsb[l][(ot * 3 + pp) * 64 + lane];
    f32x4 bias4[2];
#pragma unroll
    for (int ot = 0; ot < 2; ++ot) bias4[ot] = *reinterpret_cast<const f32x4*>(p.bias[l] + 16 * ot + 4 * g);
    float2 wreg[2][16];
    {
      const int m = m_lo + wave;
      const float2* w = p.wt[l] + ((long long)(m < m_hi ? m : 0) * C + (lane >> 5) * 16) * C + (lane & 31);
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) wreg[0][cc] = w[cc * C];
    }
    lds_barrier();   // s_y complete (all rows of the workgroup)
    DLWP_STAMP();
    // ---- P1: partial H-direction DFT of the own rows, columns (ky = wave, wave + ROWS, ..; c)
    for (int ky = wave; ky < M2; ky += ROWS) {
      // the four accumulator chains (2 channel halves x re / im) interleaved: a dependent fp32 matrix instruction waits ~40 cycles
      f32x4 dre[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}}, dim[2] = {dre[0], dre[0]};
#pragma unroll
      for (int s = 0; s < KS1; ++s) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          const float b = s_y[(2 * s + (g >> 1)) * kSyStride + (2 * ky + (g & 1)) * C + 16 * nt + j];
          dre[nt] = mfma16x16x4(a_re[s], b, dre[nt]);
          dim[nt] = mfma16x16x4(a_im[s], b, dim[nt]);
        }
      }
      // one wave-uniform decision for all 16 stores of the wave (st_xchg branched per store)
      auto publish = [&](auto fastc) {
        constexpr bool FAST = decltype(fastc)::value;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) {
            const int r = 4 * g + r4;
            if (r < M1) {
              float* dst = xp_mine + (long long)(ky * M1 + r) * 64 + 16 * nt + j;
              if constexpr (!LL) {
                st_sc1(dst, dre[nt][r4]);
                st_sc1(dst + 32, dim[nt][r4]);
              } else if constexpr (FAST) {
                dst[0] = dre[nt][r4];
                dst[32] = dim[nt][r4];
              } else {
                __hip_atomic_store(dst, dre[nt][r4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(dst + 32, dim[nt][r4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              }
            }
          }
      };
      if (fast) publish(std::true_type{}); else publish(std::false_type{});
    }
    DLWP_STAMP();
    target += (unsigned)G;
    if (!LL) trunk_group_arrive(ctr);
    // in the shadow of the barrier: the part of the row that does not need the spectrum, bias + 1x1 skip
    // convolution of the resident activation on the bf16 pipe (bf16x6)
    f32x4 acc[2][4];
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[ot][q] = F16 ? bias4[ot] * kTrunkF16Up : bias4[ot];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      u32x4 bx[3];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        unsigned hh, mm, ll;
        split_pair_x<F16>(vv[i >> 1][2 * (i & 1)][q], vv[i >> 1][2 * (i & 1) + 1][q], hh, mm, ll);
        bx[0][i] = hh;
        bx[1][i] = mm;
        bx[2][i] = ll;
      }
#pragma unroll
      for (int ot = 0; ot < 2; ++ot) acc[ot][q] = mfma_x<F16>(wb[ot], bx, acc[ot][q]);
    }
    if (!LL) trunk_group_wait(ctr, target, s_fail, p.spin_limit);
    DLWP_STAMP();
    {   // weights of the wave's second mode: requested now, they arrive while the partials are awaited
      const int m = m_lo + wave + ROWS;
      const float2* w = p.wt[l] + ((long long)(m < m_hi ? m : 0) * C + (lane >> 5) * 16) * C + (lane & 31);
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) wreg[1][cc] = w[cc * C];
    }
    // ---- P2: channel mixing of this workgroup's share of the modes, two modes per pass.
    // lane (q4 = lane >> 4, quad = lane & 15) fetches floats 4 quad..4 quad+3 of the partials q4, q4+4, ...
    for (int up = 0; up < 2; ++up) {
      const int ma = m_lo + wave + 2 * ROWS * up, mb = ma + ROWS;
      if (ma >= m_hi) break;
      const bool has_b = mb < m_hi;
      const int q4 = lane >> 4, quad = lane & 15;
      f32x4 sa = {0.f, 0.f, 0.f, 0.f}, sb = sa;
      constexpr int NI = (G + 3) / 4;   // partials per lane and mode
#pragma unroll
      for (int i0 = 0; i0 < NI; i0 += 2) {
        const int qa = q4 + 4 * i0, qb = q4 + 4 * (i0 + 1);
        const bool va = qa < G, vb = (i0 + 1 < NI) && qb < G;
        const unsigned oa0 = (unsigned)((((va ? qa : 0) * NM + ma) * 64 + 4 * quad) * 4);
        const unsigned oa1 = (unsigned)((((vb ? qb : 0) * NM + ma) * 64 + 4 * quad) * 4);
        const unsigned obo0 = (unsigned)((((va ? qa : 0) * NM + (has_b ? mb : ma)) * 64 + 4 * quad) * 4);
        const unsigned obo1 = (unsigned)((((vb ? qb : 0) * NM + (has_b ? mb : ma)) * 64 + 4 * quad) * 4);
        f32x4 v0, v1, v2, v3;
        ld4_sc1_x4(xp_grp, oa0, oa1, obo0, obo1, v0, v1, v2, v3);
        if (LL) {
          int tries = 0;
          while (__any((va && (has_sentinel(v0) || has_sentinel(v2))) || (vb && (has_sentinel(v1) || has_sentinel(v3))))) {
            if (++tries > p.try_limit) {
              *s_fail = 1;
              break;
            }
            __builtin_amdgcn_s_sleep(2);
            ld4_sc1_x4(xp_grp, oa0, oa1, obo0, obo1, v0, v1, v2, v3);
          }
          // re-arm what was consumed (this wave is the only reader of these modes' partials)
          const f32x4 sent4 = {__uint_as_float(kSentinel), __uint_as_float(kSentinel), __uint_as_float(kSentinel),
                               __uint_as_float(kSentinel)};
          if (fast) {
            if (va) {
              st4_l2(xp_grp, oa0, sent4);
              if (has_b) st4_l2(xp_grp, obo0, sent4);
            }
            if (vb) {
              st4_l2(xp_grp, oa1, sent4);
              if (has_b) st4_l2(xp_grp, obo1, sent4);
            }
          } else {
            if (va) {
              st4_sc1(xp_grp, oa0, sent4);
              if (has_b) st4_sc1(xp_grp, obo0, sent4);
            }
            if (vb) {
              st4_sc1(xp_grp, oa1, sent4);
              if (has_b) st4_sc1(xp_grp, obo1, sent4);
            }
          }
        }
        if (va) { sa += v0; sb += v2; }
        if (vb) { sa += v1; sb += v3; }
      }
      sa += shfl_xor4(sa, 16);
      sb += shfl_xor4(sb, 16);
      sa += shfl_xor4(sa, 32);
      sb += shfl_xor4(sb, 32);
      if (lane < 16) {
        *reinterpret_cast<f32x4*>(s_x + wave * 128 + 4 * quad) = sa * p.fwd_scale;
        *reinterpret_cast<f32x4*>(s_x + wave * 128 + 64 + 4 * quad) = sb * p.fwd_scale;
      }
      wave_lds_fence();
      const int c0 = (lane >> 5) * 16;
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int m = a ? mb : ma;
        if (a && !has_b) break;
        const float* xr = s_x + wave * 128 + a * 64;
        float2 acc = {0.f, 0.f};
        if (up == 0) {
#pragma unroll
          for (int cc = 0; cc < 16; ++cc) acc = cfma(float2{xr[c0 + cc], xr[32 + c0 + cc]}, wreg[a][cc], acc);
        } else {
          const float2* w = p.wt[l] + ((long long)m * C + c0) * C + (lane & 31);
#pragma unroll
          for (int cc = 0; cc < 16; ++cc) acc = cfma(float2{xr[c0 + cc], xr[32 + c0 + cc]}, w[cc * C], acc);
        }
        acc.x += __shfl_xor(acc.x, 32);
        acc.y += __shfl_xor(acc.y, 32);
        if (LL) {
          st_xchg(ob_other + (long long)m * 64 + lane, __uint_as_float(kSentinel), fast);   // every reader of the older O is done
          st_xchg(ob + (long long)m * 64 + lane, lane < 32 ? acc.x : acc.y, fast);
        } else {
          st_sc1(ob + (long long)m * 64 + lane, lane < 32 ? acc.x : acc.y);
        }
      }
      wave_lds_fence();
    }
    DLWP_STAMP();
    target += (unsigned)G;
    if (!LL) trunk_group_barrier(ctr, target, s_fail, p.spin_limit);
    DLWP_STAMP();
    // ---- P3: inverse H-direction DFT for the own rows, columns (ky = wave, wave + ROWS, ..; o) -> s_z
    for (int ky = wave; ky < M2; ky += ROWS) {
      const float ckw = p.ck[ky];
      // O[ky = wave][r][re/im][o]: M1 * 64 floats, fetched with coalesced 16-byte loads into the (idle) transpose tile
      {
        const int nflt = M1 * 64;
        unsigned o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int f = 4 * lane + 256 * i;
          o[i] = (unsigned)((ky * nflt + (f < nflt ? f : 0)) * 4);
        }
        f32x4 v0, v1, v2, v3;
        ld4_sc1_x4(ob, o[0], o[1], o[2], o[3], v0, v1, v2, v3);
        if (LL) {
          const bool k0 = 4 * lane < nflt, k1 = 4 * lane + 256 < nflt, k2 = 4 * lane + 512 < nflt, k3 = 4 * lane + 768 < nflt;
          int tries = 0;
          while (__any((k0 && has_sentinel(v0)) || (k1 && has_sentinel(v1)) || (k2 && has_sentinel(v2)) ||
                       (k3 && has_sentinel(v3)))) {
            if (++tries > p.try_limit) {
              *s_fail = 1;
              break;
            }
            __builtin_amdgcn_s_sleep(2);
            ld4_sc1_x4(ob, o[0], o[1], o[2], o[3], v0, v1, v2, v3);
          }
        }
        if (LL && l == 0 && st == 0 && wave == 0 && ky == 0) {
          // O of layer 0 has arrived, so every workgroup of the group has run and published its XCC id: does the
          // whole group share this XCD?  (decides the store flavour of all later exchanges, see st_xchg)
          const unsigned want = (p.layer0 + 1u) << 4;
          unsigned id = __hip_atomic_load(p.xcc_tab + sample * 32 + (lane < G ? lane : 0), __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT);
          int tries = 0;
          while (__any((id & ~0xFu) != want) && ++tries < 64)
            id = __hip_atomic_load(p.xcc_tab + sample * 32 + (lane < G ? lane : 0), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
          const unsigned id0 = (unsigned)__builtin_amdgcn_readfirstlane((int)id);
          const bool same = !__any(id != id0);
          if (lane == 0) *s_fast = same ? 1 : 0;
        }
        *reinterpret_cast<f32x4*>(s_tr + 4 * lane) = v0;
        *reinterpret_cast<f32x4*>(s_tr + 4 * lane + 256) = v1;
        *reinterpret_cast<f32x4*>(s_tr + 4 * lane + 512) = v2;
        *reinterpret_cast<f32x4*>(s_tr + 4 * lane + 768) = v3;
        wave_lds_fence();
      }
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          if (s < ks3) {
            const int r = 2 * s + (g >> 1);
            const float b = r < M1 ? s_tr[r * 64 + (g & 1) * 32 + 16 * nt + j] : 0.f;
            d = mfma16x16x4(a3[s], b, d);
          }
        }
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4)
          if (2 * g + (r4 >> 1) < ROWS) {
            const int kq = 2 * ky + (r4 & 1), o = 16 * nt + j;   // bf16 form keeps Z as [row][o][k'], fp32 form as [row][k'][o]
            s_z[(2 * g + (r4 >> 1)) * (KP * C) + (kDftMx ? o * KP + kq : kq * C + o)] = d[r4] * ckw;
          }
      }
      wave_lds_fence();   // the transpose tile is reused for the next ky
    }
    lds_barrier();
    DLWP_STAMP();
    // ---- the row itself
    if constexpr (kDftMx) {
      // inverse W-DFT, bf16x6: A = Z[o = 16 ot + j][k' = 8g .. 8g+7] (lane groups 2, 3 carry zeros: K = 16 of 32)
      u32x4 za[2][3];
#pragma unroll
      for (int ot = 0; ot < 2; ++ot) {
        f32x4 z0 = {0.f, 0.f, 0.f, 0.f}, z1 = z0;
        if (g < 2) {
          const float* src = s_z + wave * (KP * C) + (16 * ot + j) * KP + 8 * g;
          z0 = *reinterpret_cast<const f32x4*>(src);
          z1 = *reinterpret_cast<const f32x4*>(src + 4);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          unsigned hh, mm, ll;
          const float v0 = i < 2 ? z0[2 * i] : z1[2 * i - 4], v1 = i < 2 ? z0[2 * i + 1] : z1[2 * i - 3];
          split_pair_x<kDftF16>(v0, v1, hh, mm, ll);
          za[ot][0][i] = hh;
          za[ot][1][i] = mm;
          za[ot][2][i] = ll;
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        u32x4 tb[3];
#pragma unroll
        for (int pp = 0; pp < 3; ++pp) tb[pp] = s_tb[(q * 3 + pp) * 64 + lane];
#pragma unroll
        for (int ot = 0; ot < 2; ++ot) {
          if constexpr (kDftF16) {   // data on the A side, at the accumulator's scale 2^14: (zh, tm') (zm', th) (zh, thB)
            acc[ot][q] = mfma16x16x32_f16(za[ot][0], tb[1], acc[ot][q]);
            acc[ot][q] = mfma16x16x32_f16(za[ot][1], tb[0], acc[ot][q]);
            acc[ot][q] = mfma16x16x32_f16(za[ot][0], tb[2], acc[ot][q]);
          } else {
            acc[ot][q] = mfma_bf16x6(za[ot], tb, acc[ot][q]);
          }
        }
      }
    } else {
      float z[KP / 4][2];
#pragma unroll
      for (int s = 0; s < KP / 4; ++s)
#pragma unroll
        for (int ot = 0; ot < 2; ++ot) z[s][ot] = s_z[wave * (KP * C) + (4 * s + g) * C + 16 * ot + j];
#pragma unroll
      for (int s = 0; s < KP / 4; ++s) {
        const f32x4 tw = *reinterpret_cast<const f32x4*>(s_t + (4 * s + g) * W + 4 * j);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int ot = 0; ot < 2; ++ot) acc[ot][q] = mfma16x16x4(z[s][ot], tw[q], acc[ot][q]);
      }
    }
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        vv[ot][r] = f32x4{acc[ot][0][r], acc[ot][1][r], acc[ot][2][r], acc[ot][3][r]};
        if constexpr (F16) vv[ot][r] *= kTrunkF16Down;     // skip convolution + inverse DFT + bias, back at the true scale
      }
    DLWP_STAMP();
    if (l < p.L - 1) {
      // neuralop FNOBlocks.forward_with_postactivation: GELU after every layer but the last
#pragma unroll
      for (int ot = 0; ot < 2; ++ot) {
        DLWP_GELU8_TRUNK(vv[ot][0], vv[ot][1]);
        DLWP_GELU8_TRUNK(vv[ot][2], vv[ot][3]);
      }
      DLWP_STAMP();
#pragma unroll
      for (int ot = 0; ot < 2; ++ot)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          *reinterpret_cast<f32x4*>(s_tr + (16 * ot + 4 * g + r) * kTrStride + 4 * j) = vv[ot][r];
      wave_lds_fence();
      DLWP_STAMP();
      f32x4 yacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      if constexpr (kDftMx) {
        fwd_dft_bf16x6<kDftF16>(s_tr, s_ttb, lane, yacc);
      } else {
#pragma unroll
        for (int s = 0; s < 16; ++s)
#pragma unroll
          for (int ct = 0; ct < 2; ++ct)
            yacc[ct] = mfma16x16x4(s_tr[(16 * ct + j) * kTrStride + 4 * s + g], s_tt[(4 * s + g) * KP + j], yacc[ct]);
      }
      wave_lds_fence();
      DLWP_STAMP();
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
        *reinterpret_cast<f32x4*>(s_y + wave * kSyStride + j * C + 16 * ct + 4 * g) = kDftF16 ? yacc[ct] * kTrunkF16Down : yacc[ct];
    }
  }
  DLWP_STAMP();
#undef DLWP_STAMP
  if (*s_fail) {
    // loud failure: the host reads this word after the launch (DLWP_ERR_TIMEOUT / re-run on the unfused kernels)
    if (tid == 0 && p.fail_word) {
      atomicOr(p.fail_word, 1u);
      atomicAdd(p.sticky_fails, 1u);   // (per poisoned step of a workgroup: any non-zero value means failure)
    }
    const float nanv = __uint_as_float(0x7fc00000u);
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
      for (int r = 0; r < 4; ++r) vv[ot][r] = f32x4{nanv, nanv, nanv, nanv};
  }
  if (STEP && p.proj_hid > 0) {
    // ---- projection (+ residual): weights staged over the transpose tiles, B operand straight from the registers
    // the projection weights are requested BEFORE the barrier that frees their LDS (they travel while the slower waves
    // finish their rows) and written behind it
    const int ntile_p = p.proj_hid >> 4;
    const int n_q1 = ntile_p * 3 * 64, n_q2 = ntile_p * p.proj_co * 16;
    u32x4 pq1[6];
    float pq2[2], pqb;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int i = tid + k * NT;
      pq1[k] = p.proj_w1b[i < n_q1 ? i : 0];
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int i = tid + k * NT;
      pq2[k] = p.proj_w2v[i < n_q2 ? i : 0];
    }
    pqb = p.proj_b1[tid < p.proj_hid ? tid : 0];
    lds_barrier();
    u32x4* q_w1 = reinterpret_cast<u32x4*>(smem);                          // [ntile][3][64]
    float* q_b1 = reinterpret_cast<float*>(q_w1 + ntile_p * 3 * 64);       // [hid]
    float* q_w2 = q_b1 + p.proj_hid;                                       // [ntile][co][16]
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int i = tid + k * NT;
      if (i < n_q1) q_w1[i] = pq1[k];
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int i = tid + k * NT;
      if (i < n_q2) q_w2[i] = pq2[k];
    }
    if (tid < p.proj_hid) q_b1[tid] = F16 ? pqb * p.proj_up : pqb;
    u32x4 bx[4][3];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        unsigned hh, mm, ll;
        split_pair_x<F16>(vv[i >> 1][2 * (i & 1)][q], vv[i >> 1][2 * (i & 1) + 1][q], hh, mm, ll);
        bx[q][0][i] = hh;
        bx[q][1][i] = mm;
        bx[q][2][i] = ll;
      }
    lds_barrier();
    // the lifting weights of the next step, requested into registers: DLWP_PREFETCH_EARLY = 1 before the projection (they
    // travel under its 16 us), 0 right before the end-of-step barrier (~2 us of L2 latency stay exposed behind it)
    u32x4 pre_w2[6];
    float pre_w1[8], pre_b1 = 0.f;
    auto lift_prefetch = [&]() {
      const int n_w2p = (p.lift_hid >> 5) * 6 * 64, n_w1p = (p.lift_hid >> 4) * p.lift_ns * 64;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const int i = tid + k * NT;
        pre_w2[k] = p.lift_w2b[i < n_w2p ? i : 0];
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int i = tid + k * NT;
        pre_w1[k] = p.lift_w1p[i < n_w1p ? i : 0];
      }
      pre_b1 = p.lift_b1[tid < p.lift_hid ? tid : 0];
    };
#if DLWP_PREFETCH_EARLY
    if (st + 1 < n_steps && !(kLiftVote && p.lift_tab != nullptr)) lift_prefetch();
#endif
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    auto run = [&](auto coc) {
      constexpr int CO = decltype(coc)::value;
      float po[CO][4];
      proj_segment<CO, F16>(bx, q_w1, q_b1, q_w2, ntile_p, lane, po, p.proj_down);
#pragma unroll
      for (int co = 0; co < CO; ++co)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float x = po[co][q];
          x += __shfl_xor(x, 16);
          x += __shfl_xor(x, 32);
          if (g == co) v[q] = x;
        }
    };
    if (p.proj_co == 1) run(std::integral_constant<int, 1>{});
    else if (p.proj_co == 2) run(std::integral_constant<int, 2>{});
    else run(std::integral_constant<int, 4>{});
    if (g < p.cout) {
      const float b2 = p.proj_b2[g];
      v += f32x4{b2, b2, b2, b2};
      if (p.feed_regs && st > 0) v += vfeed;      // the residual is the previous output: still in this lane's registers
      else if (resid_p) v += *reinterpret_cast<const f32x4*>(resid_p + (long long)gs * resid_bs + (long long)g * HW + pix);
      if (*s_fail) v = f32x4{__uint_as_float(0x7fc00000u), __uint_as_float(0x7fc00000u), __uint_as_float(0x7fc00000u),
                             __uint_as_float(0x7fc00000u)};
      *reinterpret_cast<f32x4*>(out_p + (long long)gs * out_bs + (long long)g * HW + pix) = v;
      if constexpr (F16) {
        // f16x3 range guard: an activation beyond the f16 range (|x| >= 65520) turns into inf and then NaN; a non-finite
        // OUTPUT sets bit 1 of the fail word (and the second sticky counter) and the host repeats the range on the
        // bf16x6 kernels, whose operands have the fp32 exponent range.  (Non-finite INPUTS take the same detour.)
        const float mag = fabsf(v[0]) + fabsf(v[1]) + fabsf(v[2]) + fabsf(v[3]);
        if (!(mag < 3.0e38f) && p.fail_word) {
          atomicOr(p.fail_word, 2u);
          atomicAdd(p.sticky_fails + 1, 1u);
        }
      }
    }
    if (p.trace && tid == p.trace_tid && n_stamp < 64) p.trace[blockIdx.x * 64 + n_stamp++] = __builtin_amdgcn_s_memrealtime();
    if (st + 1 < n_steps) {
      const int npair_n = p.lift_hid >> 5, n_w2 = npair_n * 6 * 64, n_w1 = (p.lift_hid >> 4) * p.lift_ns * 64;
      auto feed_next = [&]() {
        if (p.feed_regs) {
          vfeed = (g < p.cout) ? v : f32x4{0.f, 0.f, 0.f, 0.f};   // next input + residual: no store -> load round trip, no drain
        } else {
          // the next step's input rows are the ones this wave has just written: drain the stores, drop any L1 copy
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
      };
      if (kLiftVote && p.lift_tab != nullptr) {
        feed_next();   // the next step votes: no weight request here, and the barrier of the seam is the one behind its vote
      } else {
#if !DLWP_PREFETCH_EARLY
        lift_prefetch();
#endif
        feed_next();
        lds_barrier();   // every wave is done with the projection weights: the lifting weights may overwrite them
        u32x4* l_w2n = reinterpret_cast<u32x4*>(smem);
        float* l_w1n = reinterpret_cast<float*>(l_w2n + n_w2);
        float* l_b1n = l_w1n + n_w1;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          const int i = tid + k * NT;
          if (i < n_w2) l_w2n[i] = pre_w2[k];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int i = tid + k * NT;
          if (i < n_w1) l_w1n[i] = pre_w1[k];
        }
        if (tid < p.lift_hid) l_b1n[tid] = pre_b1;
        staged = true;
      }
    }
    continue;
  }
#pragma unroll
  for (int ot = 0; ot < 2; ++ot)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      *reinterpret_cast<f32x4*>(p.y + ((long long)gs * C + 16 * ot + 4 * g + r) * HW + pix) = vv[ot][r];
  }   // steps
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
// host side
// ---------------------------------------------------------------------------------------------
struct SpectralCore {  // what one spectral convolution stage needs on the device
  int H = 0, W = 0, M1 = 0, M2 = 0, KP = 0;
  float fwd_scale = 1.f;
  DevBuf t, tt, ef, ei, ck;
  DevBuf tb, ttb;   // bf16x3 B operands of the W-direction DFTs for the fused kernel (W == 64, KP == 16 only)
  DevBuf tbh, ttbh; // the same twiddles as f16x3 parts (th, tm' = (t - th) * 2^11, 0) for the f16x3 step kernel

  int32_t build(int H_, int W_, int M1_, int M2_, const int32_t* rows_in, const int32_t* rows_out,
                float fwd, float inv, hipStream_t s) {
    H = H_; W = W_; M1 = M1_; M2 = M2_; fwd_scale = fwd;
    KP = (2 * M2 <= 16) ? 16 : 32;
    DLWP_REQUIRE(2 * M2 <= 32, DLWP_ERR_UNSUPPORTED, "kept rfft columns %d > 16 not supported", M2);
    DLWP_REQUIRE(M2 <= W / 2 + 1 && M1 <= H, DLWP_ERR_INVALID_ARGUMENT, "modes exceed the grid");
    const double two_pi = 6.283185307179586476925286766559;
    std::vector<float> ht((size_t)KP * W, 0.f), htt((size_t)W * KP, 0.f);
    for (int ky = 0; ky < M2; ++ky)
      for (int w = 0; w < W; ++w) {
        const long long m = ((long long)ky * w) % W;
        const double a = two_pi * (double)m / (double)W;
        const float c = (float)std::cos(a), sn = (float)(-std::sin(a));
        ht[(size_t)(2 * ky) * W + w] = c;
        ht[(size_t)(2 * ky + 1) * W + w] = sn;
        htt[(size_t)w * KP + 2 * ky] = c;
        htt[(size_t)w * KP + 2 * ky + 1] = sn;
      }
    std::vector<float> hef((size_t)M1 * H * 2), hei((size_t)M1 * H * 2), hck(M2);
    for (int r = 0; r < M1; ++r)
      for (int h = 0; h < H; ++h) {
        const long long mi = ((long long)rows_in[r] * h) % H, mo = ((long long)rows_out[r] * h) % H;
        const double ai = two_pi * (double)mi / (double)H, ao = two_pi * (double)mo / (double)H;
        hef[((size_t)r * H + h) * 2 + 0] = (float)std::cos(ai);
        hef[((size_t)r * H + h) * 2 + 1] = (float)(-std::sin(ai));
        hei[((size_t)r * H + h) * 2 + 0] = (float)std::cos(ao);
        hei[((size_t)r * H + h) * 2 + 1] = (float)std::sin(ao);
      }
    for (int ky = 0; ky < M2; ++ky) {
      const bool self_conj = (ky == 0) || (W % 2 == 0 && ky == W / 2);
      hck[ky] = (self_conj ? 1.f : 2.f) * inv;
    }
    if (W == 64 && KP == 16) {
      // inverse: B[k = k' = 8g + jj][col j -> pixel 4j + q]  -> [q][part][lane][dword]   (lanes g >= 2 supply zeros)
      // forward: B[k = pixel 32kb + 8g + jj][col j -> k' = j] -> [kb][part][lane][dword]
      std::vector<uint32_t> htb((size_t)4 * 3 * 64 * 4, 0u), httb((size_t)2 * 3 * 64 * 4, 0u);
      std::vector<uint32_t> htbh(htb.size(), 0u), httbh(httb.size(), 0u);
      for (int l = 0; l < 64; ++l) {
        const int jj0 = l & 15, gg = l >> 4;
        for (int d = 0; d < 4; ++d) {
          for (int q = 0; q < 4; ++q) {
            uint16_t hh[2], mm[2], ll[2];
            for (int e = 0; e < 2; ++e) {
              const int kp = 8 * gg + 2 * d + e;
              split3_host(kp < KP ? ht[(size_t)kp * W + 4 * jj0 + q] : 0.f, hh[e], mm[e], ll[e]);
            }
            {
              uint16_t fh[2], fm[2], fb[2];   // (th, tm', thB) of t * 2^kTrunkF16Shift
              for (int e = 0; e < 2; ++e) {
                const int kp = 8 * gg + 2 * d + e;
                split2_host_f16((kp < KP ? ht[(size_t)kp * W + 4 * jj0 + q] : 0.f) * (float)(1 << kTrunkF16Shift), fh[e], fm[e]);
                fb[e] = f16_times_2048_host(fh[e]);
              }
              htbh[(((size_t)q * 3 + 0) * 64 + l) * 4 + d] = (uint32_t)fh[0] | ((uint32_t)fh[1] << 16);
              htbh[(((size_t)q * 3 + 1) * 64 + l) * 4 + d] = (uint32_t)fm[0] | ((uint32_t)fm[1] << 16);
              htbh[(((size_t)q * 3 + 2) * 64 + l) * 4 + d] = (uint32_t)fb[0] | ((uint32_t)fb[1] << 16);
            }
            htb[(((size_t)q * 3 + 0) * 64 + l) * 4 + d] = (uint32_t)hh[0] | ((uint32_t)hh[1] << 16);
            htb[(((size_t)q * 3 + 1) * 64 + l) * 4 + d] = (uint32_t)mm[0] | ((uint32_t)mm[1] << 16);
            htb[(((size_t)q * 3 + 2) * 64 + l) * 4 + d] = (uint32_t)ll[0] | ((uint32_t)ll[1] << 16);
          }
          for (int kb = 0; kb < 2; ++kb) {
            uint16_t hh[2], mm[2], ll[2];
            for (int e = 0; e < 2; ++e) {
              const int w = 32 * kb + 8 * gg + 2 * d + e;
              split3_host(htt[(size_t)w * KP + jj0], hh[e], mm[e], ll[e]);
            }
            {
              uint16_t fh[2], fm[2], fb[2];
              for (int e = 0; e < 2; ++e) {
                const int w = 32 * kb + 8 * gg + 2 * d + e;
                split2_host_f16(htt[(size_t)w * KP + jj0] * (float)(1 << kTrunkF16Shift), fh[e], fm[e]);
                fb[e] = f16_times_2048_host(fh[e]);
              }
              httbh[(((size_t)kb * 3 + 0) * 64 + l) * 4 + d] = (uint32_t)fh[0] | ((uint32_t)fh[1] << 16);
              httbh[(((size_t)kb * 3 + 1) * 64 + l) * 4 + d] = (uint32_t)fm[0] | ((uint32_t)fm[1] << 16);
              httbh[(((size_t)kb * 3 + 2) * 64 + l) * 4 + d] = (uint32_t)fb[0] | ((uint32_t)fb[1] << 16);
            }
            httb[(((size_t)kb * 3 + 0) * 64 + l) * 4 + d] = (uint32_t)hh[0] | ((uint32_t)hh[1] << 16);
            httb[(((size_t)kb * 3 + 1) * 64 + l) * 4 + d] = (uint32_t)mm[0] | ((uint32_t)mm[1] << 16);
            httb[(((size_t)kb * 3 + 2) * 64 + l) * 4 + d] = (uint32_t)ll[0] | ((uint32_t)ll[1] << 16);
          }
        }
      }
      DLWP_HIP_CHECK(tb.upload(htb.data(), htb.size() * 4, s));
      DLWP_HIP_CHECK(ttb.upload(httb.data(), httb.size() * 4, s));
      DLWP_HIP_CHECK(tbh.upload(htbh.data(), htbh.size() * 4, s));
      DLWP_HIP_CHECK(ttbh.upload(httbh.data(), httbh.size() * 4, s));
      DLWP_HIP_CHECK(hipStreamSynchronize(s));
    }
    DLWP_HIP_CHECK(t.upload(ht.data(), ht.size() * 4, s));
    DLWP_HIP_CHECK(tt.upload(htt.data(), htt.size() * 4, s));
    DLWP_HIP_CHECK(ef.upload(hef.data(), hef.size() * 4, s));
    DLWP_HIP_CHECK(ei.upload(hei.data(), hei.size() * 4, s));
    DLWP_HIP_CHECK(ck.upload(hck.data(), hck.size() * 4, s));
    DLWP_HIP_CHECK(hipStreamSynchronize(s));  // host staging vectors die at scope exit
    return DLWP_OK;
  }
  size_t modes_lds_bytes() const { return (size_t)(2 * M1 * H + 18 * M1 * kC) * sizeof(float2); }
};

// pack spectral weights [Ci][Co][M1][M2][2] (optionally two row blocks) -> Wt[M2][M1tot][Ci][Co] complex
static void pack_spectral(std::vector<float>& dst, const float* w, int Ci, int Co, int M1blk, int M2,
                          int M1tot, int row_off) {
  for (int c = 0; c < Ci; ++c)
    for (int o = 0; o < Co; ++o)
      for (int r = 0; r < M1blk; ++r)
        for (int ky = 0; ky < M2; ++ky) {
          const size_t src = ((((size_t)c * Co + o) * M1blk + r) * M2 + ky) * 2;
          const size_t d = ((((size_t)ky * M1tot + (r + row_off)) * Ci + c) * Co + o) * 2;
          dst[d] = w[src];
          dst[d + 1] = w[src + 1];
        }
}

static int grid_rows(int nrow, int waves_per_block) {
  int blocks = (nrow + waves_per_block - 1) / waves_per_block;
  const int cap = 256 * 8;
  return blocks < cap ? (blocks > 0 ? blocks : 1) : cap;
}

template <class K>
static hipError_t allow_lds(K kernel, size_t bytes) {
  if (bytes <= 48 * 1024) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)bytes);
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

static int32_t launch_modes(const SpectralCore& sc, const float* ybuf, float* zbuf, const float2* wt, int B,
                            hipStream_t s) {
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
static int32_t launch_layer(const SpectralCore& sc, const LayerParams& lp, hipStream_t s, bool bf16x6 = true) {
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

}  // namespace fno
}  // namespace dlwp

using namespace dlwp;
using namespace dlwp::fno;

// ---------------------------------------------------------------------------------------------
// FNO2d plan
// ---------------------------------------------------------------------------------------------
// Every switch of the FNO path, fixed when the plan is created: the descriptor's fields, with the DLWP_* environment
// variables only as debug defaults read at that moment.  Nothing process-global selects a kernel after that.
struct FnoKnobs {
  bool fp32_mfma = false;     // plain fp32-MFMA kernels + unfused spectral path (cross-check form)
  bool feed_regs = true;      // persistent rollout: a step's input / residual stays in registers when it is the previous output (debug: DLWP_FNO_FEED_REGS=0)
  bool f16x3 = false;         // precision_form 2: the fused step kernel takes its big products as f16x3 (common.hpp)
  bool lift_table = true;     // one input channel: the fused step kernel reads the lifting MLP from a plan-time table (desc.lift_table = 1 or DLWP_FNO_LIFT_TABLE=0: off)
  bool trunk = true;          // fused trunk kernel (DLWP_FNO_TRUNK=0 disables)
  int trunk_rows_forced = 0;  // DLWP_TRUNK_ROWS
  bool step = true;           // whole step in one launch (DLWP_FNO_STEP=0 disables)
  bool persistent = true;     // whole rollout range in one launch (DLWP_FNO_PERSISTENT=0 disables)
  bool ll = true;             // flag-in-data hand-offs (DLWP_TRUNK_LL=0: counter barriers)
  bool lift_only = false;     // diagnostics (DLWP_STEP_LIFT_ONLY)
  int layer_stagger = 0;      // DLWP_LAYER_STAGGER
  int spin_limit = 1 << 17, try_limit = 1 << 16;
  int on_timeout = 0;         // 0: re-run the range on the unfused kernels, 1: return DLWP_ERR_TIMEOUT
  int check = 1;              // 1: synchronise on the fail word after fused launches (default), 0: caller polls dlwp_fno2d_status
  int cus = 0;                // compute units of the plan's device
  int resident_per_cu = 0;    // fused-kernel workgroups the occupancy query admits per CU
};
static int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// ---------------------------------------------------------------------------------------------
// Table of the one-input-channel lifting MLP (see lift_from_table): builder, host evaluation, guard
// ---------------------------------------------------------------------------------------------
namespace {
constexpr double kLiftTabBound = 1.0 / 4194304.0;   // 2^-22: the operand precision the f16x3 form documents and accepts

struct LiftFn {   // lift(x) and its first two derivatives, fp64 (weights as given, fp32)
  const float *w1, *b1, *w2, *b2;
  int hid;
  mutable std::vector<double> g0, g1, g2;
  void operator()(double x, double* f, double* d1, double* d2) const {
    g0.resize(hid); g1.resize(hid); g2.resize(hid);
    for (int c = 0; c < hid; ++c) {
      const double w = w1[c], z = w * x + (double)b1[c];
      const double cdf = 0.5 * std::erfc(-z * 0.70710678118654752440);          // no cancellation in the lower tail
      const double pdf = 0.39894228040143267794 * std::exp(-0.5 * z * z);
      g0[c] = z * cdf;                           // gelu
      g1[c] = (cdf + z * pdf) * w;               // d/dx
      g2[c] = (2.0 - z * z) * pdf * w * w;       // d2/dx2
    }
    for (int o = 0; o < kC; ++o) {
      const float* wr = w2 + (size_t)o * hid;
      double s0 = 0.0, s1 = 0.0, s2 = 0.0;
      for (int c = 0; c < hid; ++c) {
        const double w = wr[c];
        s0 += w * g0[c];
        if (d1) { s1 += w * g1[c]; s2 += w * g2[c]; }
      }
      f[o] = (double)b2[o] + s0;
      if (d1) { d1[o] = s1; d2[o] = s2; }
    }
  }
};

// The table at x, with the device's arithmetic (lift_tab_locate + fp32 fmaf Horner); false outside the domain.
bool lift_table_eval1(const float* tab, int range, int log2_inv_h, float x, float* out, float* v_out, int* idx_out) {
  if (!(std::fabs(x) < (float)range)) return false;
  float v;
  const int idx = lift_tab_locate(x, range << log2_inv_h, (float)(1 << log2_inv_h), v);
  const float* c = tab + (size_t)idx * kLiftTabStride;
  for (int o = 0; o < kC; ++o) {
    float acc = c[(kLiftTabCoefs - 1) * kC + o];
    for (int k = kLiftTabCoefs - 2; k >= 0; --k) acc = std::fmaf(acc, v, c[k * kC + o]);
    out[o] = acc;
  }
  if (v_out) *v_out = v;
  if (idx_out) *idx_out = idx;
  return true;
}

// Fills tab [2 range 2^log2_inv_h][6][32] and returns the guard's figure: the largest ||p(x) - lift(x)||_2 / ||lift(x)||_2 over four
// interior points of every interval and, in the two intervals touching zero, v = 2^-k, k = 1..20 (points whose ||lift|| is
// below 1e-30 count with their absolute error over the largest ||lift|| seen).  NaN if anything is not finite.
double lift_table_fill(const LiftFn& fn, int range, int log2_inv_h, float* tab) {
  const int n_side = range << log2_inv_h, n = 2 * n_side;
  const double h = std::ldexp(1.0, -log2_inv_h);
  std::vector<double> F((size_t)(n + 1) * kC), D(F.size()), E(F.size());
  double fmax = 0.0;
  for (int k = 0; k <= n; ++k) {
    double* f = &F[(size_t)k * kC];
    fn((k - n_side) * h, f, &D[(size_t)k * kC], &E[(size_t)k * kC]);
    double nn = 0.0;
    for (int o = 0; o < kC; ++o) nn += f[o] * f[o];
    fmax = std::fmax(fmax, std::sqrt(nn));
  }
  for (int t = 0; t < n; ++t) {
    // anchor = the end nearer zero; v runs from it towards the far end, so odd derivatives change sign for x < 0
    const bool neg = t < n_side;
    const int a = neg ? t + 1 : t, b = neg ? t : t + 1;
    const double sg = neg ? -h : h;
    for (int o = 0; o < kC; ++o) {
      const double f0 = F[(size_t)a * kC + o], d0 = sg * D[(size_t)a * kC + o], e0 = h * h * E[(size_t)a * kC + o];
      const double f1 = F[(size_t)b * kC + o], d1 = sg * D[(size_t)b * kC + o], e1 = h * h * E[(size_t)b * kC + o];
      const double c0 = f0, c1 = d0, c2 = 0.5 * e0;
      const double ra = f1 - c0 - c1 - c2, rb = d1 - c1 - 2.0 * c2, rc = e1 - 2.0 * c2;
      const double co[kLiftTabCoefs] = {c0, c1, c2, 10.0 * ra - 4.0 * rb + 0.5 * rc, -15.0 * ra + 7.0 * rb - rc,
                                        6.0 * ra - 3.0 * rb + 0.5 * rc};
      for (int k = 0; k < kLiftTabCoefs; ++k) tab[((size_t)t * kLiftTabCoefs + k) * kC + o] = (float)co[k];
    }
  }
  double worst = 0.0;
  bool finite = std::isfinite(fmax);
  double want[kC];
  float got[kC];
  auto probe = [&](float x) {
    if (!lift_table_eval1(tab, range, log2_inv_h, x, got, nullptr, nullptr)) { finite = false; return; }
    fn((double)x, want, nullptr, nullptr);
    double en = 0.0, fnorm = 0.0;
    for (int o = 0; o < kC; ++o) {
      const double e = (double)got[o] - want[o];
      en += e * e;
      fnorm += want[o] * want[o];
    }
    en = std::sqrt(en); fnorm = std::sqrt(fnorm);
    const double rel = fnorm < 1e-30 ? (fmax > 0.0 ? en / fmax : en) : en / fnorm;
    if (!std::isfinite(rel)) finite = false;
    worst = std::fmax(worst, rel);
  };
  for (int t = 0; t < n; ++t) {
    const bool neg = t < n_side;
    const double anchor = ((neg ? t + 1 : t) - n_side) * h;
    for (int m = 0; m < 4; ++m) probe((float)(anchor + (neg ? -h : h) * (2 * m + 1) / 8.0));
  }
  for (int k = 1; k <= 20; ++k) {
    probe((float)std::ldexp(h, -k));
    probe((float)-std::ldexp(h, -k));
  }
  return finite ? worst : std::nan("");
}
}  // namespace

extern "C" int32_t dlwp_fno2d_lift_table_build(const float* lift_w1, const float* lift_b1, const float* lift_w2,
                                               const float* lift_b2, int32_t lifting, int32_t range, int32_t log2_inv_h,
                                               float* table, size_t table_floats, double* guard_err, int32_t* accepted) {
  DLWP_REQUIRE(lift_w1 && lift_b1 && lift_w2 && lift_b2 && table, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(lifting >= 1 && range >= 1 && range <= 1024 && log2_inv_h >= 0 && log2_inv_h <= 8, DLWP_ERR_INVALID_ARGUMENT,
               "need lifting >= 1, range in [1, 1024], log2_inv_h in [0, 8] (got %d, %d, %d)", lifting, range, log2_inv_h);
  const size_t need = (size_t)2 * ((size_t)range << log2_inv_h) * kLiftTabStride;
  DLWP_REQUIRE(table_floats >= need, DLWP_ERR_INVALID_ARGUMENT, "table holds %zu floats, %zu needed", table_floats, need);
  const LiftFn fn{lift_w1, lift_b1, lift_w2, lift_b2, lifting, {}, {}, {}};
  const double err = lift_table_fill(fn, range, log2_inv_h, table);
  if (guard_err) *guard_err = err;
  if (accepted) *accepted = err <= kLiftTabBound ? 1 : 0;   // NaN fails
  return DLWP_OK;
}

extern "C" int32_t dlwp_fno2d_lift_table_eval_host(const float* table, int32_t range, int32_t log2_inv_h, const float* x,
                                                   int64_t n, float* out, float* v_out, int32_t* interval_out) {
  DLWP_REQUIRE(table && x && out && n >= 0, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(range >= 1 && range <= 1024 && log2_inv_h >= 0 && log2_inv_h <= 8, DLWP_ERR_INVALID_ARGUMENT,
               "need range in [1, 1024], log2_inv_h in [0, 8] (got %d, %d)", range, log2_inv_h);
  for (int64_t i = 0; i < n; ++i) {
    float v = std::nanf("");
    int idx = -1;
    if (!lift_table_eval1(table, range, log2_inv_h, x[i], out + i * kC, &v, &idx))   // outside the domain: the kernel evaluates the MLP
      for (int o = 0; o < kC; ++o) out[i * kC + o] = std::nanf("");
    if (v_out) v_out[i] = v;
    if (interval_out) interval_out[i] = idx;
  }
  return DLWP_OK;
}

struct dlwp_fno2d_plan {
  FnoKnobs k;
  mutable std::atomic<unsigned> timeouts{0};   // statistics only: fused launches that timed out (re-run or reported)
  mutable std::atomic<unsigned> range_reruns{0};   // statistics only: f16x3 ranges repeated on the bf16x6 kernels (non-finite output)
  DevBuf sticky;                               // device word the fused kernels add to on a timeout (reset by dlwp_fno2d_status)
  int cin = 0, hid_l = 0, hid_p = 0, cout = 0, L = 0, H = 0, W = 0;
  int cin_steps = 0;
  SpectralCore sc;
  DevBuf lift_w1p, lift_b1, lift_w2p, lift_b2, lift_w2b;
  DevBuf lift_w2h, proj_w1hp;      // f16x3 operands of the fused step kernel (precision_form 2)
  DevBuf lift_tab;                 // fused step kernel, one input channel: table of the lifting MLP (lift_from_table)
  int lift_tab_state = 0;          // dlwp_fno2d_lift_table_state
  double lift_tab_err = 0.0;       // the guard's figure for this plan's weights
  int lift_shift = 0, proj_shift = 0;   // the shift s those two matrices were packed with (common.hpp f16x3_weight_shift)
  std::vector<DevBuf> wshp;        // likewise the skip weights, trunk k order
  DevBuf proj_w1p, proj_b1, proj_w2p, proj_b2, proj_w2v, proj_w1b, proj_w1bp;   // w1bp: k order of the trunk's resident activation
  int proj_co = 0;  // outputs handled by pw_proj_small_kernel (1, 2 or 4), 0 = generic MFMA path
  std::vector<DevBuf> wt, wsp, sbias, wsb, wsbp;   // wsbp: bf16x3 skip weights in the trunk kernel's k order
  sany::Fno* gen = nullptr;   // shapes outside the 32-channel kernels' domain: the width-generic plan (spectral_any.hip)
  ~dlwp_fno2d_plan() { sany::fno_destroy(gen); }
};

// The 32-channel kernels' domain; every other shape gets a width-generic plan.
static bool fno_specialised(const dlwp_fno2d_desc* d) {
  return d->hidden_channels == kC && d->lifting_channels > 0 && d->lifting_channels % 16 == 0 &&
         d->projection_channels > 0 && d->projection_channels % 16 == 0 && d->in_channels >= 1 && d->in_channels <= 32 &&
         d->out_channels >= 1 && d->out_channels <= 16 && 2 * d->n_cols <= 32;
}

static void pack_w1(std::vector<float>& dst, const float* w1, int hid, int cin, int cin_steps) {
  dst.assign((size_t)(hid / 16) * cin_steps * 64, 0.f);
  for (int t = 0; t < hid / 16; ++t)
    for (int s = 0; s < cin_steps; ++s)
      for (int l = 0; l < 64; ++l) {
        const int ch = 16 * t + (l & 15), ci = 4 * s + (l >> 4);
        if (ci < cin) dst[((size_t)t * cin_steps + s) * 64 + l] = w1[(size_t)ch * cin + ci];
      }
}
// bf16x6 A operands of a [rows][K = 32] matrix block: [rows/16][3 parts][64 lanes][4 dwords]
// f16: the same layout holding the f16x3 parts (wh = f16(w 2^s), wm' = (w 2^s - wh) * 2^11, whB = wh * 2^11) -- common.hpp
static void pack_a_bf16x3(std::vector<uint32_t>& dst, const float* w, int rows, int ld, bool f16 = false, float f16_scale = 1.f) {
  dst.assign((size_t)(rows / 16) * 3 * 64 * 4, 0u);
  for (int t = 0; t < rows / 16; ++t)
    for (int l = 0; l < 64; ++l)
      for (int d = 0; d < 4; ++d) {
        uint16_t h[2], m[2], lo[2] = {0, 0};
        for (int e = 0; e < 2; ++e) {
          const float v = w[(size_t)(16 * t + (l & 15)) * ld + 8 * (l >> 4) + 2 * d + e];
          if (f16) {
            split2_host_f16(v * f16_scale, h[e], m[e]);
            lo[e] = f16_times_2048_host(h[e]);
          } else split3_host(v, h[e], m[e], lo[e]);
        }
        const size_t base = ((size_t)t * 3 * 64 + l) * 4 + d;
        dst[base + 0 * 64 * 4] = (uint32_t)h[0] | ((uint32_t)h[1] << 16);
        dst[base + 1 * 64 * 4] = (uint32_t)m[0] | ((uint32_t)m[1] << 16);
        dst[base + 2 * 64 * 4] = (uint32_t)lo[0] | ((uint32_t)lo[1] << 16);
      }
}

// bf16x6 A operands of layer 2 of the lifting MLP: W2 [32][hid] -> [hid/32][3 parts][2 out tiles][64 lanes][4 dwords];
// k-slot (g, jj) of tile pair u is hidden channel 16*(2u + jj/4) + 4g + jj%4 (accumulator order of layer 1)
static void pack_lift_w2_bf16x3(std::vector<uint32_t>& dst, const float* w2, int hid, bool f16 = false, float f16_scale = 1.f) {
  const int npair = hid / 32;
  dst.assign((size_t)npair * 3 * 2 * 64 * 4, 0u);
  for (int u = 0; u < npair; ++u)
    for (int ot = 0; ot < 2; ++ot)
      for (int l = 0; l < 64; ++l)
        for (int d = 0; d < 4; ++d) {
          uint16_t h[2], m[2], lo[2] = {0, 0};
          for (int e = 0; e < 2; ++e) {
            const int jj = 2 * d + e, g = l >> 4;
            const int ch = 16 * (2 * u + jj / 4) + 4 * g + jj % 4;
            const float v = w2[(size_t)(16 * ot + (l & 15)) * hid + ch];
            if (f16) {
              split2_host_f16(v * f16_scale, h[e], m[e]);
              lo[e] = f16_times_2048_host(h[e]);
            } else split3_host(v, h[e], m[e], lo[e]);
          }
          auto at = [&](int part) -> uint32_t& { return dst[((((size_t)u * 3 + part) * 2 + ot) * 64 + l) * 4 + d]; };
          at(0) = (uint32_t)h[0] | ((uint32_t)h[1] << 16);
          at(1) = (uint32_t)m[0] | ((uint32_t)m[1] << 16);
          at(2) = (uint32_t)lo[0] | ((uint32_t)lo[1] << 16);
        }
}

static void pack_w2(std::vector<float>& dst, const float* w2, int hid, int cout, int cout_tiles) {
  dst.assign((size_t)(hid / 16) * 4 * cout_tiles * 64, 0.f);
  for (int t = 0; t < hid / 16; ++t)
    for (int r = 0; r < 4; ++r)
      for (int ot = 0; ot < cout_tiles; ++ot)
        for (int l = 0; l < 64; ++l) {
          const int o = 16 * ot + (l & 15), ch = 16 * t + 4 * (l >> 4) + r;
          if (o < cout) dst[(((size_t)t * 4 + r) * cout_tiles + ot) * 64 + l] = w2[(size_t)o * hid + ch];
        }
}

namespace { int fused_resident_per_cu(int G); bool step_eligible(const dlwp_fno2d_plan* p); }

extern "C" int32_t dlwp_fno2d_plan_create(dlwp_fno2d_plan** out, const dlwp_fno2d_desc* d, void* stream) {
  DLWP_REQUIRE(out && d, DLWP_ERR_INVALID_ARGUMENT, "null plan/desc");
  *out = nullptr;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (!fno_specialised(d)) {
    sany::Fno* gen = nullptr;
    const int32_t rc = sany::fno_create(&gen, d, s);
    if (rc != DLWP_OK) return rc;
    auto* p = new dlwp_fno2d_plan();
    p->gen = gen;
    *out = p;
    return DLWP_OK;
  }
  DLWP_REQUIRE(d->hidden_channels == kC, DLWP_ERR_UNSUPPORTED, "hidden_channels %d: kernels are specialised for %d",
               d->hidden_channels, kC);
  DLWP_REQUIRE(d->lifting_channels > 0 && d->lifting_channels % 16 == 0 && d->projection_channels > 0 &&
                   d->projection_channels % 16 == 0,
               DLWP_ERR_UNSUPPORTED, "lifting/projection channels must be positive multiples of 16");
  DLWP_REQUIRE(d->in_channels >= 1 && d->in_channels <= 32, DLWP_ERR_UNSUPPORTED, "in_channels %d not in [1,32]",
               d->in_channels);
  DLWP_REQUIRE(d->out_channels >= 1 && d->out_channels <= 16, DLWP_ERR_UNSUPPORTED, "out_channels %d not in [1,16]",
               d->out_channels);
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
  DLWP_REQUIRE(d->lift_table == 0 || d->lift_table == 1, DLWP_ERR_INVALID_ARGUMENT, "lift_table %d not in {0, 1}", d->lift_table);
  auto* p = new dlwp_fno2d_plan();
  {
    FnoKnobs& k = p->k;
    // descriptor first; the environment only supplies debug defaults, read HERE and never again
    k.fp32_mfma = d->precision_form == 1 || env_int("DLWP_FP32_MFMA", 0) != 0;
    k.feed_regs = env_int("DLWP_FNO_FEED_REGS", 1) != 0;
    k.lift_table = d->lift_table == 0 && env_int("DLWP_FNO_LIFT_TABLE", 1) != 0;
    k.f16x3 = !k.fp32_mfma && (d->precision_form == 2 || env_int("DLWP_FNO_F16X3", 0) != 0);
    k.trunk = env_int("DLWP_FNO_TRUNK", 1) != 0 && d->launch_form != 3;
    k.trunk_rows_forced = env_int("DLWP_TRUNK_ROWS", 0);
    k.step = env_int("DLWP_FNO_STEP", 1) != 0 && d->launch_form != 2 && d->launch_form != 3;
    k.persistent = env_int("DLWP_FNO_PERSISTENT", 1) != 0 && d->launch_form == 0;
    k.ll = env_int("DLWP_TRUNK_LL", 1) != 0;
    k.lift_only = env_int("DLWP_STEP_LIFT_ONLY", 0) != 0;
    k.layer_stagger = env_int("DLWP_LAYER_STAGGER", 0);
    if (d->debug_spin_limit > 0) k.spin_limit = k.try_limit = d->debug_spin_limit;
    k.on_timeout = d->on_timeout;
    k.check = d->unchecked ? 0 : 1;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&k.cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || k.cus <= 0) {
      delete p;
      return fail(DLWP_ERR_HIP, "cannot query the compute-unit count of the current device");
    }
  }
  p->cin = d->in_channels; p->hid_l = d->lifting_channels; p->hid_p = d->projection_channels;
  p->cout = d->out_channels; p->L = d->n_layers; p->H = d->height; p->W = d->width;
  p->cin_steps = (p->cin + 3) / 4;
  if (p->k.f16x3) {
    // f16x3 (common.hpp): every weight image is packed as w * 2^s with max |w| 2^s in [8, 16) so that neither part of any weight
    // is an f16 subnormal and whB = wh * 2^11 cannot overflow.  Lifting W2 and projection W1 have accumulators of their own and
    // take their own s; the skip weights share an accumulator with the inverse W-DFT, whose twiddles are packed with s = 3:
    // skip weights of 2 or more (never seen; the init is 1 / sqrt(32)) send the plan to the bf16x6 form.
    auto amax = [](const float* w, size_t n) { float m = 0.f; for (size_t i = 0; i < n; ++i) m = std::fmax(m, std::fabs(w[i])); return m; };
    p->lift_shift = f16x3_weight_shift(amax(d->lift_w2, (size_t)kC * p->hid_l));
    p->proj_shift = f16x3_weight_shift(amax(d->proj_w1, (size_t)p->hid_p * kC));
    float skip_max = 0.f;
    for (int l = 0; l < p->L; ++l) skip_max = std::fmax(skip_max, amax(d->skip_w[l], (size_t)kC * kC));
    const bool ok = std::isfinite(skip_max) && skip_max < 2.0f && std::abs(p->lift_shift) <= 40 && std::abs(p->proj_shift) <= 40;
    if (!ok) p->k.f16x3 = false;
  }
  int32_t rc = p->sc.build(d->height, d->width, d->n_rows, d->n_cols, d->rows_in, d->rows_out, d->fwd_scale,
                           d->inv_scale, s);
  if (rc != DLWP_OK) { delete p; return rc; }
  auto up = [&](DevBuf& b, const std::vector<float>& v) -> hipError_t { return b.upload(v.data(), v.size() * 4, s); };
  std::vector<float> tmp;
  hipError_t e = hipSuccess;
  do {
    pack_w1(tmp, d->lift_w1, p->hid_l, p->cin, p->cin_steps);
    if ((e = up(p->lift_w1p, tmp)) != hipSuccess) break;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) break;
    if ((e = p->lift_b1.upload(d->lift_b1, (size_t)p->hid_l * 4, s)) != hipSuccess) break;
    pack_w2(tmp, d->lift_w2, p->hid_l, kC, 2);
    if ((e = up(p->lift_w2p, tmp)) != hipSuccess) break;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) break;
    if ((e = p->lift_b2.upload(d->lift_b2, (size_t)kC * 4, s)) != hipSuccess) break;
    if (p->hid_l % 32 == 0) {
      std::vector<uint32_t> wb;
      pack_lift_w2_bf16x3(wb, d->lift_w2, p->hid_l);
      if ((e = p->lift_w2b.upload(wb.data(), wb.size() * 4, s)) != hipSuccess) break;
      if ((e = hipStreamSynchronize(s)) != hipSuccess) break;
      if (p->k.f16x3) {
        pack_lift_w2_bf16x3(wb, d->lift_w2, p->hid_l, true, std::ldexp(1.f, p->lift_shift));
        if ((e = p->lift_w2h.upload(wb.data(), wb.size() * 4, s)) != hipSuccess) break;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) break;
      }
    }
    pack_w1(tmp, d->proj_w1, p->hid_p, kC, 8);
    if ((e = up(p->proj_w1p, tmp)) != hipSuccess) break;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) break;
    if ((e = p->proj_b1.upload(d->proj_b1, (size_t)p->hid_p * 4, s)) != hipSuccess) break;
    pack_w2(tmp, d->proj_w2, p->hid_p, p->cout, 1);
    if ((e = up(p->proj_w2p, tmp)) != hipSuccess) break;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) break;
    if (p->cout <= 4) {
      p->proj_co = p->cout <= 1 ? 1 : (p->cout <= 2 ? 2 : 4);
      std::vector<float> wv((size_t)(p->hid_p / 16) * p->proj_co * 16, 0.f);
      for (int t = 0; t < p->hid_p / 16; ++t)
        for (int co = 0; co < p->cout; ++co)
          for (int k = 0; k < 16; ++k) wv[((size_t)t * p->proj_co + co) * 16 + k] = d->proj_w2[(size_t)co * p->hid_p + 16 * t + k];
      if ((e = up(p->proj_w2v, wv)) != hipSuccess) break;
      if ((e = hipStreamSynchronize(s)) != hipSuccess) break;
      std::vector<uint32_t> wb;
      pack_a_bf16x3(wb, d->proj_w1, p->hid_p, kC);
      if ((e = p->proj_w1b.upload(wb.data(), wb.size() * 4, s)) != hipSuccess) break;
      if ((e = hipStreamSynchronize(s)) != hipSuccess) break;
      {
        // fused step kernel: the projection's B operand is the resident activation, k-slot 8g + c' = channel
        // 16 (c' >> 2) + 4 g + (c' & 3) (same order as the skip weights wsbp)
        std::vector<float> wperm((size_t)p->hid_p * kC);
        for (int o = 0; o < p->hid_p; ++o)
          for (int k = 0; k < kC; ++k) {
            const int gg = k >> 3, cp = k & 7;
            wperm[(size_t)o * kC + k] = d->proj_w1[(size_t)o * kC + 16 * (cp >> 2) + 4 * gg + (cp & 3)];
          }
        pack_a_bf16x3(wb, wperm.data(), p->hid_p, kC);
        if ((e = p->proj_w1bp.upload(wb.data(), wb.size() * 4, s)) != hipSuccess) break;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) break;
        if (p->k.f16x3) {
          pack_a_bf16x3(wb, wperm.data(), p->hid_p, kC, true, std::ldexp(1.f, p->proj_shift));
          if ((e = p->proj_w1hp.upload(wb.data(), wb.size() * 4, s)) != hipSuccess) break;
          if ((e = hipStreamSynchronize(s)) != hipSuccess) break;
        }
      }
    }
    std::vector<float> b2(16, 0.f);
    for (int i = 0; i < p->cout; ++i) b2[i] = d->proj_b2[i];
    if ((e = up(p->proj_b2, b2)) != hipSuccess) break;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) break;
    p->wt.resize(p->L); p->wsp.resize(p->L); p->sbias.resize(p->L); p->wsb.resize(p->L); p->wsbp.resize(p->L); p->wshp.resize(p->L);
    for (int l = 0; l < p->L && e == hipSuccess; ++l) {
      std::vector<float> w((size_t)d->n_cols * d->n_rows * kC * kC * 2, 0.f);
      pack_spectral(w, d->spec_w[l], kC, kC, d->n_rows, d->n_cols, d->n_rows, 0);
      if ((e = up(p->wt[l], w)) != hipSuccess) break;
      std::vector<float> ws((size_t)8 * 2 * 64);
      for (int st = 0; st < 8; ++st)
        for (int half = 0; half < 2; ++half)
          for (int ln = 0; ln < 64; ++ln)
            ws[((size_t)st * 2 + half) * 64 + ln] = d->skip_w[l][(size_t)(16 * half + (ln & 15)) * kC + 4 * st + (ln >> 4)];
      if ((e = up(p->wsp[l], ws)) != hipSuccess) break;
      std::vector<uint32_t> wsb;
      pack_a_bf16x3(wsb, d->skip_w[l], kC, kC);
      if ((e = p->wsb[l].upload(wsb.data(), wsb.size() * 4, s)) != hipSuccess) break;
      {
        // fno_trunk_kernel takes the B operand from its resident registers: k-slot 8g + c' is channel
        // 16 (c' >> 2) + 4 g + (c' & 3)
        std::vector<float> wperm((size_t)kC * kC);
        for (int o = 0; o < kC; ++o)
          for (int k = 0; k < kC; ++k) {
            const int gg = k >> 3, cp = k & 7;
            wperm[(size_t)o * kC + k] = d->skip_w[l][(size_t)o * kC + 16 * (cp >> 2) + 4 * gg + (cp & 3)];
          }
        std::vector<uint32_t> wsbp;
        pack_a_bf16x3(wsbp, wperm.data(), kC, kC);
        if ((e = p->wsbp[l].upload(wsbp.data(), wsbp.size() * 4, s)) != hipSuccess) break;
        if (p->k.f16x3) {
          if ((e = hipStreamSynchronize(s)) != hipSuccess) break;
          pack_a_bf16x3(wsbp, wperm.data(), kC, kC, true, (float)(1 << kTrunkF16Shift));
          if ((e = p->wshp[l].upload(wsbp.data(), wsbp.size() * 4, s)) != hipSuccess) break;
        }
      }
      if ((e = p->sbias[l].upload(d->spec_b + (size_t)l * kC, (size_t)kC * 4, s)) != hipSuccess) break;
      if ((e = hipStreamSynchronize(s)) != hipSuccess) break;
    }
  } while (0);
  if (e != hipSuccess) {
    delete p;
    return fail(DLWP_ERR_HIP, "plan upload failed: %s", hipGetErrorString(e));
  }
  {
    const unsigned zero[2] = {0, 0};   // [0] hand-off timeouts, [1] f16x3 ranges with a non-finite output
    hipError_t se = p->sticky.upload(zero, 8, s);
    if (se == hipSuccess) se = hipStreamSynchronize(s);
    if (se != hipSuccess) { delete p; return fail(DLWP_ERR_HIP, "plan allocation failed: %s", hipGetErrorString(se)); }
  }
  // Residency of the fused kernels (8-row workgroups, 512 threads, trunk_lds(8) bytes of LDS): the hand-offs spin on
  // peer workgroups, so a launch may only hold as many workgroups as the occupancy query admits per CU x CUs.  A
  // device that admits none (LDS or registers) gets the unfused kernels.
  p->k.resident_per_cu = 0;
  if (p->k.trunk && !p->k.fp32_mfma && p->H % 8 == 0) {
    p->k.resident_per_cu = fused_resident_per_cu(p->H / 8);
    if (p->k.resident_per_cu == 0) p->k.trunk = false;
  }
  // One input channel on the fused step kernel: tabulate the lifting MLP (fixed for the life of the plan) and keep the table
  // only if the guard accepts it for THESE weights; otherwise the kernel evaluates the MLP as it does for wider inputs.
  if (step_eligible(p) && p->cin == 1) {
    if (!p->k.lift_table) {
      p->lift_tab_state = 3;
    } else {
      std::vector<float> tab((size_t)2 * (kLiftTabRange << kLiftTabLog2) * kLiftTabStride);
      const LiftFn fn{d->lift_w1, d->lift_b1, d->lift_w2, d->lift_b2, p->hid_l, {}, {}, {}};
      p->lift_tab_err = lift_table_fill(fn, kLiftTabRange, kLiftTabLog2, tab.data());
      p->lift_tab_state = p->lift_tab_err <= kLiftTabBound ? 1 : 2;
      if (p->lift_tab_state == 1) {
        hipError_t te = p->lift_tab.upload(tab.data(), tab.size() * 4, s);
        if (te == hipSuccess) te = hipStreamSynchronize(s);
        if (te != hipSuccess) { delete p; return fail(DLWP_ERR_HIP, "plan upload failed: %s", hipGetErrorString(te)); }
      }
    }
  }
  *out = p;
  return DLWP_OK;
}

extern "C" int32_t dlwp_fno2d_lift_table_state(const dlwp_fno2d_plan* plan) { return plan ? plan->lift_tab_state : 0; }

extern "C" uint32_t dlwp_fno2d_timeouts(const dlwp_fno2d_plan* plan) { return plan ? plan->timeouts.load() : 0u; }
extern "C" uint32_t dlwp_fno2d_range_reruns(const dlwp_fno2d_plan* plan) { return plan ? plan->range_reruns.load() : 0u; }

extern "C" int32_t dlwp_fno2d_plan_destroy(dlwp_fno2d_plan* plan) {
  delete plan;
  return DLWP_OK;
}

namespace {
// Optional per-kernel-class timing with HIP events on the launch stream (bench.py roofline leg).
struct KernelTimer {
  enum { LIFT = 0, MODES = 1, LAYER = 2, PROJ = 3, EMPTY = 4, NCLASS = 5 };
  std::vector<hipEvent_t> ev[NCLASS];  // start/stop pairs
  hipStream_t s = nullptr;
  hipError_t begin(int cls) {
    hipEvent_t e;
    hipError_t rc = hipEventCreate(&e);
    if (rc != hipSuccess) return rc;
    ev[cls].push_back(e);
    return hipEventRecord(e, s);
  }
  hipError_t end(int cls) { return begin(cls); }
  ~KernelTimer() {
    for (auto& v : ev)
      for (auto e : v) (void)hipEventDestroy(e);
  }
};
struct FnoWorkspace {
  float *h0, *h1, *ybuf, *zbuf;
  float *xpart, *obuf;   // fused trunk: per-workgroup spectrum partials, mixed spectrum (two copies each)
  size_t xpart_half, obuf_half;   // floats per copy
  unsigned* ctr;         // fused trunk: one group counter per sample (128 B apart)
  unsigned* fail;        // fused trunk: set by a workgroup whose hand-off spin ran out (zeroed by trunk_begin)
  size_t total;
};
constexpr size_t kCtrStrideBytes = 128;
constexpr size_t kFailBytes = 256;
FnoWorkspace carve(const dlwp_fno2d_plan* p, int B, void* base) {
  FnoWorkspace w;
  const size_t act = align_up((size_t)B * kC * p->H * p->W * 4, 256);
  const size_t yz = align_up((size_t)B * p->H * kC * p->sc.KP * 4, 256);
  char* c = reinterpret_cast<char*>(base);
  w.h0 = reinterpret_cast<float*>(c);
  w.h1 = reinterpret_cast<float*>(c + act);
  w.ybuf = reinterpret_cast<float*>(c + 2 * act);
  w.zbuf = reinterpret_cast<float*>(c + 2 * act + yz);
  const int G = (p->H + 3) / 4;   // most workgroups per sample the fused trunk uses
  const size_t nm = (size_t)p->sc.M1 * p->sc.M2 * 64 * 4;
  // two copies each (layer parity of the flag-in-data protocol)
  const size_t xp = 2 * align_up((size_t)B * G * nm, 256), ob = 2 * align_up((size_t)B * nm, 256);
  const size_t ct = 2 * align_up((size_t)B * kCtrStrideBytes, 256);   // group counters + XCC-id table
  w.xpart = reinterpret_cast<float*>(c + 2 * act + 2 * yz);
  w.obuf = reinterpret_cast<float*>(c + 2 * act + 2 * yz + xp);
  w.ctr = reinterpret_cast<unsigned*>(c + 2 * act + 2 * yz + xp + ob);
  w.fail = reinterpret_cast<unsigned*>(c + 2 * act + 2 * yz + xp + ob + ct);
  w.xpart_half = xp / 8;
  w.obuf_half = ob / 8;
  w.total = 2 * act + 2 * yz + xp + ob + ct + kFailBytes;
  return w;
}

template <int CS>
int32_t launch_lift_cs(const MlpParams& mp, int kp, int grid, size_t lds, hipStream_t s, bool bf, size_t lds_bf) {
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

// Fused trunk (fno_trunk_kernel): eligibility, counter reset, launch.
constexpr size_t trunk_lds(int rows) {
  return ((size_t)rows * kC * kTrStride + rows * kSyStride + rows * 16 * kC + rows * 128 + 2 * 16 * 64 + 4 + 2 * 2 * 16 * rows +
          6 * 3 * 64 * 4) *
         sizeof(float);
}
// rows (= waves) per workgroup.  8 = one workgroup per CU (default).  4 puts two workgroups on a CU (2 x 61 KB of
// LDS, 2 x 4 waves x 256 VGPRs) so that one can compute rows while the other sits in a group barrier -- measured
// SLOWER at the headline size (68 vs 51 us per launch: twice the partials to publish and sum, two ky columns per
// wave in P1/P3); kept for grids whose height is not a multiple of 8 and selectable with DLWP_TRUNK_ROWS=4.
int trunk_rows(const dlwp_fno2d_plan* p) {
  const int forced = p->k.trunk_rows_forced;
  for (int rows : {8, 4}) {
    if (forced && rows != forced) continue;
    if (p->H % rows) continue;
    const int G = p->H / rows;
    if (G != 4 && G != 8 && G != 16 && G != 32) continue;          // instantiated group sizes
    if (rows == 4 && G == 4) continue;
    if (rows == 8 && G == 32) continue;
    if ((p->sc.M1 * p->sc.M2 + G - 1) / G > 4 * rows) continue;    // at most 4 modes per wave in P2
    if (G > p->k.cus * (8 / rows)) continue;                       // a sample's group must be resident at once
    return rows;
  }
  return 0;
}
bool trunk_eligible(const dlwp_fno2d_plan* p) {
  if (!p->k.trunk || p->k.fp32_mfma) return false;
  if (p->W != 64 || p->sc.KP != 16 || p->sc.M1 > 16 || p->L > kTrunkMaxLayers) return false;
  return trunk_rows(p) != 0;
}
// Whole step in one launch (STEP variant of the trunk kernel): needs the flag-in-data protocol, 8 rows per workgroup,
// bf16x6 MLP weights that fit the transpose-tile LDS (widths <= 256, <= 16 input channels) and the FMA layer 2
// of the projection (<= 4 outputs).  DLWP_FNO_STEP=0 keeps lifting / trunk / projection as three launches.
struct TrunkState {
  bool on = false;
  unsigned epoch = 0;    // group barriers already counted since the counters were zeroed
  unsigned layers = 0;   // spectral layers run since the exchange buffers were armed (flag-in-data protocol)
};
bool step_eligible(const dlwp_fno2d_plan* p) {
  return p->k.step && trunk_eligible(p) && p->k.ll && trunk_rows(p) == 8 && p->cin_steps <= 4 &&
         p->hid_l % 32 == 0 && p->hid_l <= 256 && p->hid_p <= 256 && p->proj_co > 0 && p->lift_w2b.p != nullptr &&
         p->proj_w1bp.p != nullptr;
}
int fused_resident_per_cu(int G) {
  int n = 0;
  hipError_t oe = hipErrorInvalidValue;
  constexpr size_t lds = trunk_lds(8);
  auto query = [&](auto kern) {
    oe = allow_lds(kern, lds);
    if (oe == hipSuccess) oe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kern, 512, lds);
  };
  if (G == 4) query(fno_trunk_kernel<8, 4, true, true>);
  else if (G == 8) query(fno_trunk_kernel<8, 8, true, true>);
  else if (G == 16) query(fno_trunk_kernel<8, 16, true, true>);
  else { oe = hipSuccess; n = 1; }
  if (oe != hipSuccess) { (void)hipGetLastError(); n = 0; }
  // the fused kernels were tuned and verified at ONE workgroup per CU (the query says 1 at ~120 KB of LDS); never
  // size a grid beyond that even if a later compiler build would admit two
  return n >= 1 ? 1 : 0;
}
// xpart copy 0 | xpart copy 1 | obuf copy 0 | obuf copy 1, each as large as the B samples and the G = H / rows workgroups per sample
// in use need; 11 + 1.4 MB at the headline shape instead of the 22 + 1.4 MB the workspace reserves (fill time per rollout)
struct ExchangeLayout {
  float* xpart;
  float* obuf;
  long long xpart_par, obuf_par;
  size_t floats;
};
ExchangeLayout exchange_layout(const dlwp_fno2d_plan* p, const FnoWorkspace& ws, int B) {
  const int rows = trunk_rows(p), G = rows ? p->H / rows : (p->H + 3) / 4;
  const size_t nm = (size_t)p->sc.M1 * p->sc.M2 * 64;                    // floats per (sample, member)
  ExchangeLayout x;
  x.xpart = ws.xpart;
  x.xpart_par = (long long)((size_t)B * G * nm);
  x.obuf = ws.xpart + 2 * (size_t)B * G * nm;
  x.obuf_par = (long long)((size_t)B * nm);
  x.floats = 2 * (size_t)B * G * nm + 2 * (size_t)B * nm;               // <= 2 xpart_half + 2 obuf_half (G <= H / 4)
  return x;
}
__global__ __launch_bounds__(256) void trunk_arm_kernel(u32x4* __restrict__ xch, size_t quads, unsigned* __restrict__ ctr, size_t words) {
  const size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  const u32x4 sent = {kSentinel, kSentinel, kSentinel, kSentinel};
  for (size_t i = i0; i < quads; i += stride) xch[i] = sent;
  for (size_t i = i0; i < words; i += stride) ctr[i] = 0u;
}
int32_t trunk_begin(const dlwp_fno2d_plan* p, const FnoWorkspace& ws, int B, TrunkState& st, hipStream_t s,
                    bool force_unfused = false) {
  st.on = trunk_eligible(p) && !force_unfused;
  st.epoch = 0;
  st.layers = 0;
  if (st.on) {
    // ONE launch: zero the group counters, the XCC-id table and the fail word behind them; arm both copies of both exchange buffers
    // with the sentinel (laid out back to back for the group size in use: exchange_layout()).  A kernel of our own rather than
    // hipMemset*Async: two fills were two more nodes in front of every rollout (~5 us each).
    const size_t zero_words = (2 * align_up((size_t)B * kCtrStrideBytes, 256) + kFailBytes) / 4;
    const ExchangeLayout x = exchange_layout(p, ws, B);
    const size_t arm_quads = p->k.ll ? x.floats / 4 : 0;             // nm is a multiple of 64 floats
    hipLaunchKernelGGL(trunk_arm_kernel, dim3(512), dim3(256), 0, s, reinterpret_cast<u32x4*>(x.xpart), arm_quads, ws.ctr, zero_words);
    DLWP_HIP_CHECK(hipGetLastError());
  }
  return DLWP_OK;
}
template <int G>
hipError_t step_launch_one(const TrunkParams& tp, hipStream_t s, bool f16) {
  constexpr size_t lds = trunk_lds(8);
  if (f16) {
    hipError_t e = allow_lds(fno_trunk_kernel<8, G, true, true, true>, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((fno_trunk_kernel<8, G, true, true, true>), dim3(tp.S * G), dim3(512), lds, s, tp);
    return hipGetLastError();
  }
  hipError_t e = allow_lds(fno_trunk_kernel<8, G, true, true>, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((fno_trunk_kernel<8, G, true, true>), dim3(tp.S * G), dim3(512), lds, s, tp);
  return hipGetLastError();
}
template <int ROWS, int G>
hipError_t trunk_launch_one(const TrunkParams& tp, hipStream_t s, bool ll) {
  constexpr size_t lds = trunk_lds(ROWS);
  if (ll) {
    hipError_t e = allow_lds(fno_trunk_kernel<ROWS, G, true>, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((fno_trunk_kernel<ROWS, G, true>), dim3(tp.S * G), dim3(64 * ROWS), lds, s, tp);
  } else {
    hipError_t e = allow_lds(fno_trunk_kernel<ROWS, G, false>, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((fno_trunk_kernel<ROWS, G, false>), dim3(tp.S * G), dim3(64 * ROWS), lds, s, tp);
  }
  return hipGetLastError();
}
struct StepIO {   // set for the STEP variant: the step's input table, output and residual
  const ChanTable* in = nullptr;
  float* out = nullptr;
  long long out_bstride = 0;
  const float* resid = nullptr;
  long long resid_bstride = 0;
  bool lift_only = false;
  // n_steps > 1: a whole range of rollout steps in one launch, tables rebuilt on the device
  int n_steps = 1, t0 = 0, n_const = 0, n_presc = 0, n_prog = 0, T = 0, ctx = 0;
  const float* constants = nullptr;
  const float* prescribed = nullptr;
  const float* prognostic = nullptr;
  float* rollout_out = nullptr;
};
int32_t launch_trunk(const dlwp_fno2d_plan* p, const FnoWorkspace& ws, int B, const float* hin, float* hout,
                     TrunkState& st, hipStream_t s, const StepIO* io = nullptr) {
  const int rows = trunk_rows(p);
  DLWP_REQUIRE(rows > 0, DLWP_ERR_UNSUPPORTED, "fused trunk not available for this plan");
  const int G = p->H / rows;
  // residency: every workgroup of a launch must be on the chip at once (the hand-offs spin on peers).  The grid is
  // bounded by what the occupancy query admitted for the fused kernel at plan creation x the CU count.
  int per_launch = p->k.cus * (rows == 8 ? p->k.resident_per_cu : 8 / rows) / G;
  if (per_launch >= 8) per_launch &= ~7;   // keeps the same-XCD group mapping
  DLWP_REQUIRE(per_launch > 0, DLWP_ERR_UNSUPPORTED, "a sample needs %d workgroups, more than fit the device", G);
  const size_t nm = (size_t)p->sc.M1 * p->sc.M2 * 64;
  for (int s0 = 0; s0 < B; s0 += per_launch) {
    TrunkParams tp = {};
    tp.x = hin; tp.y = hout; tp.ybuf = ws.ybuf;
    tp.t = p->sc.t.as<float>(); tp.tt = p->sc.tt.as<float>();
    tp.tb = p->sc.tb.as<u32x4>(); tp.ttb = p->sc.ttb.as<u32x4>();
    tp.ef = p->sc.ef.as<float2>(); tp.ei = p->sc.ei.as<float2>(); tp.ck = p->sc.ck.as<float>();
    for (int l = 0; l < kTrunkMaxLayers; ++l) {
      const int ll = l < p->L ? l : 0;
      tp.wsb[l] = p->wsbp[ll].as<u32x4>(); tp.bias[l] = p->sbias[ll].as<float>(); tp.wt[l] = p->wt[ll].as<float2>();
    }
    tp.S = (B - s0 < per_launch) ? B - s0 : per_launch;
    const ExchangeLayout xl = exchange_layout(p, ws, B);
    tp.xpart = xl.xpart + (size_t)s0 * G * nm;
    tp.obuf = xl.obuf + (size_t)s0 * nm;
    tp.ctr = ws.ctr + (size_t)s0 * (kCtrStrideBytes / 4);
    tp.epoch = st.epoch; tp.fwd_scale = p->sc.fwd_scale;
    tp.xpart_par = xl.xpart_par; tp.obuf_par = xl.obuf_par; tp.layer0 = st.layers;
    tp.xcc_tab = ws.ctr + align_up((size_t)B * kCtrStrideBytes, 256) / 4 + (size_t)s0 * 32;
    tp.H = p->H; tp.L = p->L; tp.M1 = p->sc.M1; tp.M2 = p->sc.M2; tp.G = G; tp.sample0 = s0;
    tp.spin_limit = p->k.spin_limit; tp.try_limit = p->k.try_limit; tp.fail_word = ws.fail;
    tp.sticky_fails = p->sticky.as<unsigned>();
    // diagnostics: DLWP_TRUNK_TRACE=<file> dumps per-workgroup phase timestamps of the first few launches
    static const char* trace_path = getenv("DLWP_TRUNK_TRACE");
    static unsigned long long* trace_buf = nullptr;
    static int traced = 0;
    tp.trace = nullptr;
    static const char* trace_wave = getenv("DLWP_TRUNK_TRACE_WAVE");
    tp.trace_tid = trace_wave ? 64 * atoi(trace_wave) : 0;
    if (trace_path && traced < 4) {
      if (!trace_buf) DLWP_HIP_CHECK(hipMalloc(&trace_buf, (size_t)1024 * 64 * 8));
      DLWP_HIP_CHECK(hipMemsetAsync(trace_buf, 0, (size_t)1024 * 64 * 8, s));
      if (tp.S * G <= 1024) tp.trace = trace_buf;
    }
    hipError_t le = hipErrorInvalidValue;
    if (io) {
      tp.in = *io->in;
      tp.lift_ns = p->cin_steps; tp.lift_hid = p->hid_l; tp.lift_cin1 = p->cin == 1 ? 1 : 0;
#ifdef DLWP_NO_CIN1
      tp.lift_cin1 = 0;   // A/B switch (tools/ab_build.sh)
#endif
      tp.lift_w1p = p->lift_w1p.as<float>(); tp.lift_b1 = p->lift_b1.as<float>();
      tp.lift_w2b = p->lift_w2b.as<u32x4>(); tp.lift_b2 = p->lift_b2.as<float>();
      tp.lift_tab = p->lift_tab_state == 1 ? p->lift_tab.as<float>() : nullptr;
      tp.proj_hid = p->hid_p; tp.proj_co = p->proj_co; tp.cout = p->cout;
      if (io->lift_only) { tp.proj_hid = 0; tp.y = hout; }   // diagnostics: the projection stays a launch of its own
      tp.proj_w1b = p->proj_w1bp.as<u32x4>(); tp.proj_b1 = p->proj_b1.as<float>();
      tp.proj_w2v = p->proj_w2v.as<float>(); tp.proj_b2 = p->proj_b2.as<float>();
      tp.out = io->out; tp.out_bstride = io->out_bstride; tp.resid = io->resid; tp.resid_bstride = io->resid_bstride;
      tp.n_steps = io->n_steps;
      if (io->n_steps > 1) {
        tp.r_const = io->constants; tp.r_presc = io->prescribed; tp.r_prog = io->prognostic; tp.r_out = io->rollout_out;
        tp.r_nconst = io->n_const; tp.r_npresc = io->n_presc; tp.r_nprog = io->n_prog; tp.r_T = io->T; tp.r_ctx = io->ctx;
        tp.r_t0 = io->t0;
        tp.feed_regs = (io->n_const == 0 && io->n_presc == 0 && io->ctx == 1 && io->n_prog <= 4 && p->cin_steps == 1 &&
                        p->cin == io->n_prog && p->k.feed_regs) ? 1 : 0;
      }
      const bool f16 = p->k.f16x3 && p->lift_w2h.p && p->proj_w1hp.p && !io->lift_only;
      tp.lift_up = tp.lift_down = tp.proj_up = tp.proj_down = 1.f;
      if (f16) {   // f16x3 operands (the unfused kernels and the plain trunk keep bf16x6)
        tp.lift_up = std::ldexp(1.f, 11 + p->lift_shift); tp.lift_down = std::ldexp(1.f, -(11 + p->lift_shift));
        tp.proj_up = std::ldexp(1.f, 11 + p->proj_shift); tp.proj_down = std::ldexp(1.f, -(11 + p->proj_shift));
        tp.lift_w2b = p->lift_w2h.as<u32x4>();
        tp.proj_w1b = p->proj_w1hp.as<u32x4>();
        tp.tb = p->sc.tbh.as<u32x4>(); tp.ttb = p->sc.ttbh.as<u32x4>();
        for (int l = 0; l < kTrunkMaxLayers; ++l) tp.wsb[l] = p->wshp[l < p->L ? l : 0].as<u32x4>();
      }
      if (G == 4) le = step_launch_one<4>(tp, s, f16);
      else if (G == 8) le = step_launch_one<8>(tp, s, f16);
      else if (G == 16) le = step_launch_one<16>(tp, s, f16);
    } else
    if (rows == 8 && G == 4) le = trunk_launch_one<8, 4>(tp, s, p->k.ll);
    else if (rows == 8 && G == 8) le = trunk_launch_one<8, 8>(tp, s, p->k.ll);
    else if (rows == 8 && G == 16) le = trunk_launch_one<8, 16>(tp, s, p->k.ll);
    else if (rows == 4 && G == 8) le = trunk_launch_one<4, 8>(tp, s, p->k.ll);
    else if (rows == 4 && G == 16) le = trunk_launch_one<4, 16>(tp, s, p->k.ll);
    else if (rows == 4 && G == 32) le = trunk_launch_one<4, 32>(tp, s, p->k.ll);
    DLWP_HIP_CHECK(le);
    if (tp.trace) {
      std::vector<unsigned long long> hbuf((size_t)tp.S * G * 64);
      DLWP_HIP_CHECK(hipStreamSynchronize(s));
      DLWP_HIP_CHECK(hipMemcpy(hbuf.data(), trace_buf, hbuf.size() * 8, hipMemcpyDeviceToHost));
      if (FILE* f = fopen(trace_path, traced ? "a" : "w")) {
        for (int wg = 0; wg < tp.S * G; ++wg) {
          fprintf(f, "%d %d", traced, wg);
          for (int k = 0; k < 64 && hbuf[(size_t)wg * 64 + k]; ++k) fprintf(f, " %llu", hbuf[(size_t)wg * 64 + k]);
          fprintf(f, "\n");
        }
        fclose(f);
      }
      ++traced;
    }
  }
  const unsigned steps = (io && io->n_steps > 1) ? (unsigned)io->n_steps : 1u;
  st.epoch += 2u * (unsigned)p->L * steps;
  st.layers += (unsigned)p->L * steps;
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

// Reads the fail word of the fused launches enqueued so far on `s` (synchronises the stream).  Returns 1 if a hand-off
// timed out (bit 0) and / or an f16x3 range produced a non-finite output (bit 1), 0 if neither, < 0 on a HIP error.
// Skipped (returns 0) while the stream is being captured into a graph.
int read_fail_word(const FnoWorkspace& ws, hipStream_t s) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return 0;
  thread_local unsigned* h_word = nullptr;   // pinned, one per host thread (like dlwp_last_error); never freed
  if (!h_word && hipHostMalloc(reinterpret_cast<void**>(&h_word), 64, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    h_word = nullptr;
    return -1;
  }
  *h_word = 0u;
  if (hipMemcpyAsync(h_word, ws.fail, sizeof(unsigned), hipMemcpyDeviceToHost, s) != hipSuccess) return -1;
  if (hipStreamSynchronize(s) != hipSuccess) return -1;
  return (int)(*h_word & 3u);
}

// one backbone step: x (channel table) -> out (+ resid)
int32_t fno_step(const dlwp_fno2d_plan* p, const ChanTable& xt, int B, const FnoWorkspace& ws, float* out,
                 long long out_bstride, const float* resid, long long resid_bstride, hipStream_t s,
                 TrunkState* trunk, KernelTimer* timer = nullptr) {
  const int nrow = B * p->H;
  if (timer) {  // calibration: an empty bracket measures what the event pair itself adds
    DLWP_HIP_CHECK(timer->begin(KernelTimer::EMPTY));
    DLWP_HIP_CHECK(timer->end(KernelTimer::EMPTY));
  }
  if (trunk && trunk->on && step_eligible(p)) {
    // the whole step in ONE launch (reported in the LAYER class; LIFT / MODES / PROJ stay empty)
    StepIO io;
    io.in = &xt; io.out = out; io.out_bstride = out_bstride; io.resid = resid; io.resid_bstride = resid_bstride;
    if (timer) DLWP_HIP_CHECK(timer->begin(KernelTimer::LAYER));
    const bool lift_only = p->k.lift_only;
    io.lift_only = lift_only;
    const int32_t rc = launch_trunk(p, ws, B, nullptr, lift_only ? ws.h1 : nullptr, *trunk, s, &io);
    if (rc != DLWP_OK) return rc;
    if (timer) DLWP_HIP_CHECK(timer->end(KernelTimer::LAYER));
    if (!lift_only) return DLWP_OK;
    return fno_project(p, ws.h1, B, out, out_bstride, resid, resid_bstride, s, timer);
  }
  // lifting (+ W-direction DFT of its output)
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
  float* hin = ws.h0;
  float* hout = ws.h1;
  if (trunk && trunk->on) {
    // all spectral layers in one launch, activation resident in registers (reported in the LAYER class)
    if (timer) DLWP_HIP_CHECK(timer->begin(KernelTimer::LAYER));
    const int32_t rc = launch_trunk(p, ws, B, hin, hout, *trunk, s);
    if (rc != DLWP_OK) return rc;
    if (timer) DLWP_HIP_CHECK(timer->end(KernelTimer::LAYER));
    hin = hout;
  } else
  for (int l = 0; l < p->L; ++l) {
    if (timer) DLWP_HIP_CHECK(timer->begin(KernelTimer::MODES));
    int32_t rc = launch_modes(p->sc, ws.ybuf, ws.zbuf, p->wt[l].as<float2>(), B, s);
    if (rc != DLWP_OK) return rc;
    if (timer) DLWP_HIP_CHECK(timer->end(KernelTimer::MODES));
    LayerParams lp;
    lp.x = hin; lp.y = hout; lp.wsp = p->wsp[l].as<float>(); lp.wsb = p->wsb[l].as<u32x4>(); lp.bias = p->sbias[l].as<float>();
    lp.zbuf = ws.zbuf; lp.t = p->sc.t.as<float>(); lp.tt = p->sc.tt.as<float>(); lp.ybuf = ws.ybuf;
    lp.B = B; lp.H = p->H; lp.W = p->W;
    lp.stagger = p->k.layer_stagger;
    const bool last = (l == p->L - 1);
    // neuralop FNOBlocks.forward_with_postactivation: GELU after every layer but the last
    if (timer) DLWP_HIP_CHECK(timer->begin(KernelTimer::LAYER));
    rc = last ? launch_layer<true, false, false>(p->sc, lp, s, !p->k.fp32_mfma)
              : launch_layer<true, true, true>(p->sc, lp, s, !p->k.fp32_mfma);
    if (rc != DLWP_OK) return rc;
    if (timer) DLWP_HIP_CHECK(timer->end(KernelTimer::LAYER));
    float* t = hin; hin = hout; hout = t;
  }
  return fno_project(p, hin, B, out, out_bstride, resid, resid_bstride, s, timer);
}
}  // namespace

extern "C" size_t dlwp_fno2d_workspace_bytes(const dlwp_fno2d_plan* plan, int32_t batch) {
  if (!plan || batch <= 0) return 0;
  if (plan->gen) return sany::fno_workspace_bytes(plan->gen, batch);
  return carve(plan, batch, nullptr).total;
}

extern "C" int32_t dlwp_fno2d_forward_f32(const dlwp_fno2d_plan* plan, const float* x, float* y, int32_t batch,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  DLWP_REQUIRE(plan && x && y && workspace, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  if (plan->gen)
    return sany::fno_forward(plan->gen, x, y, batch, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream));
  DLWP_REQUIRE(batch > 0, DLWP_ERR_INVALID_ARGUMENT, "batch must be positive");
  const FnoWorkspace ws = carve(plan, batch, workspace);
  DLWP_REQUIRE(workspace_bytes >= ws.total, DLWP_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, ws.total);
  DLWP_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(workspace) & 255) == 0,
               DLWP_ERR_INVALID_ARGUMENT, "pointers must be 16-byte (workspace 256-byte) aligned");
  const long long HW = (long long)plan->H * plan->W;
  ChanTable xt;
  xt.seg[0] = ChanSeg{x, plan->cin * HW, plan->cin, 0};
  for (int i = 1; i < 4; ++i) xt.seg[i] = ChanSeg{nullptr, 0, 0, 0};
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  for (int attempt = 0; attempt < 2; ++attempt) {
    TrunkState trunk;
    const int32_t rc0 = trunk_begin(plan, ws, batch, trunk, s, /*force_unfused=*/attempt == 1);
    if (rc0 != DLWP_OK) return rc0;
    const int32_t rc = fno_step(plan, xt, batch, ws, y, plan->cout * HW, nullptr, 0, s, &trunk);
    if (rc != DLWP_OK || !trunk.on || !plan->k.check) return rc;
    const int f = read_fail_word(ws, s);
    if (f < 0) return fail(DLWP_ERR_HIP, "reading the fused kernel's fail word failed");
    if (f == 0) return DLWP_OK;
    if (f & 1) {
      plan->timeouts.fetch_add(1);
      if (plan->k.on_timeout == 1)
        return fail(DLWP_ERR_TIMEOUT, "fused FNO step: a workgroup hand-off exceeded its spin bound (output poisoned with NaN)");
    } else {
      plan->range_reruns.fetch_add(1);   // f16x3: non-finite output -> the same step on the bf16x6 kernels
    }
  }
  return fail(DLWP_ERR_TIMEOUT, "unreachable: the unfused kernels have no hand-offs");
}

extern "C" int32_t dlwp_fno2d_status(const dlwp_fno2d_plan* plan, void* stream) {
  DLWP_REQUIRE(plan, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  if (plan->gen) return DLWP_OK;   // the generic path has no hand-offs and no f16 range
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  thread_local unsigned* h_word = nullptr;   // pinned, one per host thread; never freed
  if (!h_word) DLWP_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&h_word), 64, hipHostMallocDefault));
  h_word[0] = h_word[1] = 0u;
  DLWP_HIP_CHECK(hipMemcpyAsync(h_word, plan->sticky.p, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, s));
  DLWP_HIP_CHECK(hipMemsetAsync(plan->sticky.p, 0, 2 * sizeof(unsigned), s));
  DLWP_HIP_CHECK(hipStreamSynchronize(s));
  if (h_word[0]) {
    plan->timeouts.fetch_add(1);
    return fail(DLWP_ERR_TIMEOUT, "fused FNO kernels: %u workgroup(s) exceeded a hand-off spin bound since the last status call "
                "(outputs of those launches are poisoned with NaN)", h_word[0]);
  }
  if (h_word[1])
    return fail(DLWP_ERR_RANGE, "fused FNO kernels (f16x3): %u non-finite output vector(s) since the last status call -- an "
                "activation beyond the f16 range or a non-finite input; repeat with precision_form 0 (bf16x6) or with the "
                "per-call check, which repeats such a range on the bf16x6 kernels by itself", h_word[1]);
  return DLWP_OK;
}

static int32_t fno_rollout_once(const dlwp_fno2d_plan* plan, const float* constants, int32_t n_const,
                                const float* prescribed, int32_t n_presc, const float* prognostic,
                                int32_t n_prog, int32_t batch, int32_t n_time, int32_t context, float* out,
                                void* workspace, size_t workspace_bytes, void* stream, KernelTimer* timer,
                                int32_t step_begin, int32_t step_end, bool force_unfused, bool* used_fused);

// Checked rollout: run the range; if fused kernels were used, read their fail word (one stream synchronisation per
// call); on a timeout either report DLWP_ERR_TIMEOUT (on_timeout = 1) or re-run the SAME range on the unfused
// kernels, which have no inter-workgroup hand-offs and cannot time out (the inputs are untouched: the range only
// writes out[:, step_begin:step_end]).
static int32_t fno_rollout_impl(const dlwp_fno2d_plan* plan, const float* constants, int32_t n_const,
                                const float* prescribed, int32_t n_presc, const float* prognostic,
                                int32_t n_prog, int32_t batch, int32_t n_time, int32_t context, float* out,
                                void* workspace, size_t workspace_bytes, void* stream, KernelTimer* timer,
                                int32_t step_begin = 0, int32_t step_end = -1) {
  if (plan && plan->gen)
    return sany::fno_rollout(plan->gen, constants, n_const, prescribed, n_presc, prognostic, n_prog, batch, n_time,
                             context, out, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream), step_begin,
                             step_end, nullptr, nullptr);
  bool fused = false;
  int32_t rc = fno_rollout_once(plan, constants, n_const, prescribed, n_presc, prognostic, n_prog, batch, n_time, context,
                                out, workspace, workspace_bytes, stream, timer, step_begin, step_end, false, &fused);
  if (rc != DLWP_OK || !fused || !plan->k.check) return rc;
  const FnoWorkspace ws = carve(plan, batch, workspace);
  const int f = read_fail_word(ws, reinterpret_cast<hipStream_t>(stream));
  if (f < 0) return fail(DLWP_ERR_HIP, "reading the fused kernel's fail word failed");
  if (f == 0) return DLWP_OK;
  if (f & 1) {
    plan->timeouts.fetch_add(1);
    if (plan->k.on_timeout == 1)
      return fail(DLWP_ERR_TIMEOUT, "fused FNO rollout: a workgroup hand-off exceeded its spin bound (steps [%d, %d) poisoned "
                  "with NaN); were all %d workgroups of the launch resident?", step_begin, step_end, batch * (plan->H / 8));
  } else {
    plan->range_reruns.fetch_add(1);   // f16x3: non-finite output -> the same range on the bf16x6 kernels
  }
  return fno_rollout_once(plan, constants, n_const, prescribed, n_presc, prognostic, n_prog, batch, n_time, context, out,
                          workspace, workspace_bytes, stream, nullptr, step_begin, step_end, true, &fused);
}

static int32_t fno_rollout_once(const dlwp_fno2d_plan* plan, const float* constants, int32_t n_const,
                                const float* prescribed, int32_t n_presc, const float* prognostic,
                                int32_t n_prog, int32_t batch, int32_t n_time, int32_t context, float* out,
                                void* workspace, size_t workspace_bytes, void* stream, KernelTimer* timer,
                                int32_t step_begin, int32_t step_end, bool force_unfused, bool* used_fused) {
  DLWP_REQUIRE(plan && prognostic && out && workspace, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(batch > 0 && context >= 1 && n_time > context, DLWP_ERR_INVALID_ARGUMENT,
               "need batch > 0, context >= 1, n_time > context (got %d, %d, %d)", batch, context, n_time);
  if (!constants) n_const = 0;
  if (!prescribed) n_presc = 0;
  DLWP_REQUIRE(n_const >= 0 && n_presc >= 0 && n_prog == plan->cout, DLWP_ERR_INVALID_ARGUMENT,
               "prognostic channels %d != plan out_channels %d", n_prog, plan->cout);
  DLWP_REQUIRE(n_const + (n_presc + n_prog) * context == plan->cin, DLWP_ERR_INVALID_ARGUMENT,
               "channel count %d + (%d + %d) * %d != plan in_channels %d", n_const, n_presc, n_prog, context, plan->cin);
  const FnoWorkspace ws = carve(plan, batch, workspace);
  DLWP_REQUIRE(workspace_bytes >= ws.total, DLWP_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, ws.total);
  DLWP_REQUIRE((reinterpret_cast<uintptr_t>(prognostic) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(constants) & 15) == 0 && (reinterpret_cast<uintptr_t>(prescribed) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(workspace) & 255) == 0,
               DLWP_ERR_INVALID_ARGUMENT, "pointers must be 16-byte (workspace 256-byte) aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const long long HW = (long long)plan->H * plan->W;
  const int T = n_time, ctx = context, To = T - ctx;
  const long long prog_bs = (long long)T * n_prog * HW, out_bs = (long long)To * n_prog * HW;
  if (step_end < 0) step_end = To;
  DLWP_REQUIRE(step_begin >= 0 && step_begin <= step_end && step_end <= To, DLWP_ERR_INVALID_ARGUMENT,
               "step range [%d, %d) outside [0, %d]", step_begin, step_end, To);
  TrunkState trunk;
  {
    const int32_t rc0 = trunk_begin(plan, ws, batch, trunk, s, force_unfused);
    if (rc0 != DLWP_OK) return rc0;
  }
  *used_fused = trunk.on;
  if (trunk.on && step_eligible(plan) && plan->k.persistent && step_end - step_begin > 1) {
    // the whole range in ONE launch: no host in the loop, no launch gaps (reported in the LAYER class)
    ChanTable none;
    for (int i = 0; i < 4; ++i) none.seg[i] = ChanSeg{nullptr, 0, 0, 0};
    StepIO io;
    io.in = &none;
    io.n_steps = step_end - step_begin; io.t0 = ctx + step_begin;
    io.n_const = n_const; io.n_presc = n_presc; io.n_prog = n_prog; io.T = T; io.ctx = ctx;
    io.constants = constants; io.prescribed = prescribed; io.prognostic = prognostic; io.rollout_out = out;
    if (timer) {
      DLWP_HIP_CHECK(timer->begin(KernelTimer::EMPTY));
      DLWP_HIP_CHECK(timer->end(KernelTimer::EMPTY));
      DLWP_HIP_CHECK(timer->begin(KernelTimer::LAYER));
    }
    const int32_t rc = launch_trunk(plan, ws, batch, nullptr, nullptr, trunk, s, &io);
    if (rc != DLWP_OK) return rc;
    if (timer) DLWP_HIP_CHECK(timer->end(KernelTimer::LAYER));
    return DLWP_OK;
  }
  for (int t = ctx + step_begin; t < ctx + step_end; ++t) {
    // x_t = cat(constants[:,0], prescribed[:, t-ctx:t], prognostic window)   (fno.py:49-62, :79-100)
    // prognostic window, frame f in [t-ctx, t): input frame f if f < ctx else out[:, f-ctx]
    ChanTable xt;
    int k = 0;
    for (int i = 0; i < 4; ++i) xt.seg[i] = ChanSeg{nullptr, 0, 0, 0};
    if (n_const) xt.seg[k++] = ChanSeg{constants, (long long)n_const * HW, n_const, 0};
    if (n_presc) xt.seg[k++] = ChanSeg{prescribed + (long long)(t - ctx) * n_presc * HW, (long long)T * n_presc * HW, n_presc * ctx, 0};
    const int f0 = t - ctx;
    const int n_in = (f0 < ctx) ? (ctx - f0 < ctx ? ctx - f0 : ctx) : 0;  // frames still taken from the input
    if (n_in > 0) xt.seg[k++] = ChanSeg{prognostic + (long long)f0 * n_prog * HW, prog_bs, n_prog * n_in, 0};
    if (ctx - n_in > 0) {
      const int fo = f0 + n_in - ctx;  // first output frame index used
      xt.seg[k++] = ChanSeg{out + (long long)fo * n_prog * HW, out_bs, n_prog * (ctx - n_in), 0};
    }
    // residual = last frame of the window (fno.py:103: prognostic_t[:, -1])
    const float* resid;
    long long resid_bs;
    if (t - 1 < ctx) { resid = prognostic + (long long)(t - 1) * n_prog * HW; resid_bs = prog_bs; }
    else { resid = out + (long long)(t - 1 - ctx) * n_prog * HW; resid_bs = out_bs; }
    int32_t rc = fno_step(plan, xt, batch, ws, out + (long long)(t - ctx) * n_prog * HW, out_bs, resid, resid_bs, s, &trunk, timer);
    if (rc != DLWP_OK) return rc;
  }
  return DLWP_OK;
}

extern "C" int32_t dlwp_fno2d_rollout_f32(const dlwp_fno2d_plan* plan, const float* constants, int32_t n_const,
                                          const float* prescribed, int32_t n_presc, const float* prognostic,
                                          int32_t n_prog, int32_t batch, int32_t n_time, int32_t context, float* out,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  return fno_rollout_impl(plan, constants, n_const, prescribed, n_presc, prognostic, n_prog, batch, n_time, context,
                          out, workspace, workspace_bytes, stream, nullptr);
}

extern "C" int32_t dlwp_fno2d_rollout_range_f32(const dlwp_fno2d_plan* plan, const float* constants, int32_t n_const,
                                                const float* prescribed, int32_t n_presc, const float* prognostic,
                                                int32_t n_prog, int32_t batch, int32_t n_time, int32_t context,
                                                float* out, void* workspace, size_t workspace_bytes, void* stream,
                                                int32_t step_begin, int32_t step_end) {
  return fno_rollout_impl(plan, constants, n_const, prescribed, n_presc, prognostic, n_prog, batch, n_time, context,
                          out, workspace, workspace_bytes, stream, nullptr, step_begin, step_end);
}

extern "C" int32_t dlwp_fno2d_rollout_profiled_f32(const dlwp_fno2d_plan* plan, const float* constants,
                                                   int32_t n_const, const float* prescribed, int32_t n_presc,
                                                   const float* prognostic, int32_t n_prog, int32_t batch,
                                                   int32_t n_time, int32_t context, float* out, void* workspace,
                                                   size_t workspace_bytes, void* stream, double* class_ms,
                                                   int32_t* class_launches) {
  DLWP_REQUIRE(class_ms && class_launches, DLWP_ERR_INVALID_ARGUMENT, "null profile output");
  if (plan && plan->gen)
    return sany::fno_rollout(plan->gen, constants, n_const, prescribed, n_presc, prognostic, n_prog, batch, n_time,
                             context, out, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream), 0, -1,
                             class_ms, class_launches);
  KernelTimer timer;
  timer.s = reinterpret_cast<hipStream_t>(stream);
  int32_t rc = fno_rollout_impl(plan, constants, n_const, prescribed, n_presc, prognostic, n_prog, batch, n_time,
                                context, out, workspace, workspace_bytes, stream, &timer);
  if (rc != DLWP_OK) return rc;
  DLWP_HIP_CHECK(hipStreamSynchronize(timer.s));
  for (int c = 0; c < KernelTimer::NCLASS; ++c) {
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
  return DLWP_OK;
}



// ---------------------------------------------------------------------------------------------
// SpectralConv2d (unet.py:19-69)
// ---------------------------------------------------------------------------------------------
struct dlwp_spectral_plan {
  int ci = 0, co = 0;
  SpectralCore sc;
  DevBuf wt, zero_bias;
  std::unique_ptr<sany::Geom> gen;   // shapes outside the 32-channel kernels' domain (spectral_any.hip); wt is its image
  // The weight gradient has the generic form only.  A plan of the specialised kernels keeps its own description and
  // builds a Geom from it on the first weight-gradient call (wgen); a generic plan uses gen.  One thread per plan.
  int H = 0, W = 0, n_cols = 0;
  float fwd_scale = 1.f, inv_scale = 1.f;
  std::vector<int32_t> rows_in, rows_out;
  mutable std::unique_ptr<sany::Geom> wgen;
  void describe(int H_, int W_, int nr, int nc, const int32_t* ri, const int32_t* ro, float fwd, float inv) {
    H = H_; W = W_; n_cols = nc; fwd_scale = fwd; inv_scale = inv;
    rows_in.assign(ri, ri + nr);
    rows_out.assign(ro, ro + nr);
  }
};

// The 32-channel kernels' domain; every other shape gets a width-generic plan.
static bool spectral_specialised(int ci, int co, int H, int W, int n_cols) {
  return ci == kC && co == kC && W > 0 && W % 64 == 0 && H > 0 && 2 * n_cols <= 32;
}

static int32_t spectral_generic_create(dlwp_spectral_plan** out, int ci, int co, int H, int W, int n_rows, int n_cols,
                                       const int32_t* rows_in, const int32_t* rows_out, float fwd_scale, float inv_scale,
                                       const float* w1, const float* w2, hipStream_t s) {
  auto* p = new dlwp_spectral_plan();
  p->ci = ci; p->co = co;
  p->gen.reset(new sany::Geom());
  int32_t rc = sany::geom_build(*p->gen, ci, co, H, W, n_rows, n_cols, rows_in, rows_out, fwd_scale, inv_scale, s);
  if (rc != DLWP_OK) { delete p; return rc; }
  hipError_t e;
  if (w1) {   // host weights: rows [0, n_rows / 2) from w1, the rest from w2 (unet.py:60-65)
    std::vector<float> w;
    sany::pack_host(w, *p->gen, w1, n_rows / 2, 0);
    sany::pack_host(w, *p->gen, w2, n_rows / 2, n_rows / 2);
    e = p->wt.upload(w.data(), w.size() * 4, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
  } else {
    e = p->wt.alloc((size_t)n_cols * n_rows * ci * co * 2 * sizeof(float));
    if (e == hipSuccess) e = hipMemsetAsync(p->wt.p, 0, p->wt.bytes, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
  }
  if (e != hipSuccess) { delete p; return fail(DLWP_ERR_HIP, "plan upload failed: %s", hipGetErrorString(e)); }
  *out = p;
  return DLWP_OK;
}

extern "C" int32_t dlwp_spectral_conv2d_plan_create(dlwp_spectral_plan** out, int32_t ci, int32_t co, int32_t H,
                                                    int32_t W, int32_t m1, int32_t m2, const float* w1, const float* w2,
                                                    void* stream) {
  DLWP_REQUIRE(out && w1 && w2, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  if (!spectral_specialised(ci, co, H, W, m2)) {
    DLWP_REQUIRE(m1 >= 1 && 2 * m1 <= H && m2 >= 1 && m2 <= W / 2 + 1, DLWP_ERR_INVALID_ARGUMENT, "bad mode counts");
    std::vector<int32_t> rows(2 * m1);
    for (int r = 0; r < m1; ++r) { rows[r] = r; rows[m1 + r] = H - m1 + r; }
    return spectral_generic_create(out, ci, co, H, W, 2 * m1, m2, rows.data(), rows.data(), 1.0f,
                                   1.0f / ((float)H * (float)W), w1, w2, reinterpret_cast<hipStream_t>(stream));
  }
  DLWP_REQUIRE(ci == kC && co == kC, DLWP_ERR_UNSUPPORTED, "SpectralConv2d kernels are specialised for %d channels", kC);
  DLWP_REQUIRE(W > 0 && W % 64 == 0 && H > 0, DLWP_ERR_UNSUPPORTED, "width %d must be a positive multiple of 64", W);
  DLWP_REQUIRE(m1 >= 1 && 2 * m1 <= H && m2 >= 1 && m2 <= W / 2 + 1, DLWP_ERR_INVALID_ARGUMENT, "bad mode counts");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  auto* p = new dlwp_spectral_plan();
  p->ci = ci; p->co = co;
  // unet.py:60-65: rows [:m1] use weights1, rows [-m1:] use weights2 (later assignment wins on overlap,
  // excluded above by 2*m1 <= H); un-normalised forward, 1/(H*W) on the inverse (torch default "backward").
  std::vector<int32_t> rows(2 * m1);
  for (int r = 0; r < m1; ++r) { rows[r] = r; rows[m1 + r] = H - m1 + r; }
  int32_t rc = p->sc.build(H, W, 2 * m1, m2, rows.data(), rows.data(), 1.0f, 1.0f / ((float)H * (float)W), s);
  if (rc != DLWP_OK) { delete p; return rc; }
  p->describe(H, W, 2 * m1, m2, rows.data(), rows.data(), 1.0f, 1.0f / ((float)H * (float)W));
  std::vector<float> w((size_t)m2 * 2 * m1 * ci * co * 2, 0.f);
  pack_spectral(w, w1, ci, co, m1, m2, 2 * m1, 0);
  pack_spectral(w, w2, ci, co, m1, m2, 2 * m1, m1);
  std::vector<float> zb(kC, 0.f);
  hipError_t e = p->wt.upload(w.data(), w.size() * 4, s);
  if (e == hipSuccess) e = p->zero_bias.upload(zb.data(), zb.size() * 4, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { delete p; return fail(DLWP_ERR_HIP, "plan upload failed: %s", hipGetErrorString(e)); }
  *out = p;
  return DLWP_OK;
}

// General mode-truncated spectral convolution (explicit kept rows and transform scales) with weights set from the
// DEVICE: what a training step needs (weights change every step; the backward-data pass is the same operator with
// rows_in/rows_out swapped and conjugate-transposed weights).
extern "C" int32_t dlwp_spectral_conv2d_plan_create_ex(dlwp_spectral_plan** out, int32_t ci, int32_t co, int32_t H,
                                                       int32_t W, int32_t n_rows, int32_t n_cols, const int32_t* rows_in,
                                                       const int32_t* rows_out, float fwd_scale, float inv_scale,
                                                       void* stream) {
  DLWP_REQUIRE(out && rows_in && rows_out, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  if (!spectral_specialised(ci, co, H, W, n_cols))
    return spectral_generic_create(out, ci, co, H, W, n_rows, n_cols, rows_in, rows_out, fwd_scale, inv_scale, nullptr,
                                   nullptr, reinterpret_cast<hipStream_t>(stream));
  DLWP_REQUIRE(ci == kC && co == kC, DLWP_ERR_UNSUPPORTED, "SpectralConv2d kernels are specialised for %d channels", kC);
  DLWP_REQUIRE(W > 0 && W % 64 == 0 && H > 0, DLWP_ERR_UNSUPPORTED, "width %d must be a positive multiple of 64", W);
  DLWP_REQUIRE(n_rows >= 1 && n_rows <= H && n_cols >= 1 && n_cols <= W / 2 + 1, DLWP_ERR_INVALID_ARGUMENT, "bad mode counts");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  auto* p = new dlwp_spectral_plan();
  p->ci = ci; p->co = co;
  int32_t rc = p->sc.build(H, W, n_rows, n_cols, rows_in, rows_out, fwd_scale, inv_scale, s);
  if (rc != DLWP_OK) { delete p; return rc; }
  p->describe(H, W, n_rows, n_cols, rows_in, rows_out, fwd_scale, inv_scale);
  std::vector<float> zb(kC, 0.f);
  hipError_t e = p->wt.alloc((size_t)n_cols * n_rows * ci * co * 2 * sizeof(float));
  if (e == hipSuccess) e = hipMemsetAsync(p->wt.p, 0, p->wt.bytes, s);
  if (e == hipSuccess) e = p->zero_bias.upload(zb.data(), zb.size() * 4, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { delete p; return fail(DLWP_ERR_HIP, "plan allocation failed: %s", hipGetErrorString(e)); }
  *out = p;
  return DLWP_OK;
}

extern "C" int32_t dlwp_spectral_conv2d_set_weights_dev(dlwp_spectral_plan* plan, const float* weights_dev,
                                                        int32_t adjoint, void* stream) {
  DLWP_REQUIRE(plan && weights_dev, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  if (plan->gen)
    return sany::pack_dev(*plan->gen, weights_dev, adjoint, plan->wt.as<float2>(), reinterpret_cast<hipStream_t>(stream));
  const int R = plan->sc.M1, K = plan->sc.M2;
  const long long total = (long long)plan->ci * plan->co * R * K;
  long long blocks = (total + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  // weights_dev is [Ci][Co][R][K][2] of the FORWARD operator in both cases
  hipLaunchKernelGGL(pack_spectral_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const float2*>(weights_dev), plan->wt.as<float2>(), plan->ci, plan->co, R, K,
                     adjoint ? 1 : 0);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" int32_t dlwp_spectral_conv2d_plan_destroy(dlwp_spectral_plan* plan) {
  delete plan;
  return DLWP_OK;
}

extern "C" size_t dlwp_spectral_conv2d_workspace_bytes(const dlwp_spectral_plan* plan, int32_t batch) {
  if (!plan || batch <= 0) return 0;
  if (plan->gen) return sany::workspace_bytes(*plan->gen, batch);
  return 2 * align_up((size_t)batch * plan->sc.H * kC * plan->sc.KP * 4, 256);
}

extern "C" int32_t dlwp_spectral_conv2d_f32(const dlwp_spectral_plan* plan, const float* x, float* y, int32_t batch,
                                            void* workspace, size_t workspace_bytes, void* stream) {
  DLWP_REQUIRE(plan && x && y && workspace, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(batch > 0, DLWP_ERR_INVALID_ARGUMENT, "batch must be positive");
  const size_t need = dlwp_spectral_conv2d_workspace_bytes(plan, batch);
  DLWP_REQUIRE(workspace_bytes >= need, DLWP_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, need);
  DLWP_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(workspace) & 255) == 0,
               DLWP_ERR_INVALID_ARGUMENT, "pointers must be 16-byte (workspace 256-byte) aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (plan->gen) {
    const int32_t rc = sany::run_fwd_mix(*plan->gen, plan->wt.as<float2>(), x, batch, workspace, s);
    return rc != DLWP_OK ? rc : sany::run_inv(*plan->gen, y, batch, workspace, s);
  }
  const SpectralCore& sc = plan->sc;
  float* ybuf = reinterpret_cast<float*>(workspace);
  float* zbuf = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + need / 2);
  const int grid = grid_rows(batch * sc.H, 4);
  const size_t lds = (size_t)4 * kC * kTrStride * sizeof(float);
  if (sc.KP == 16) hipLaunchKernelGGL((fwd_dft_kernel<16>), dim3(grid), dim3(256), lds, s, x, ybuf, sc.tt.as<float>(), batch, sc.H, sc.W);
  else hipLaunchKernelGGL((fwd_dft_kernel<32>), dim3(grid), dim3(256), lds, s, x, ybuf, sc.tt.as<float>(), batch, sc.H, sc.W);
  DLWP_HIP_CHECK(hipGetLastError());
  int32_t rc = launch_modes(sc, ybuf, zbuf, plan->wt.as<float2>(), batch, s);
  if (rc != DLWP_OK) return rc;
  LayerParams lp;
  lp.x = x; lp.y = y; lp.wsp = nullptr; lp.wsb = nullptr; lp.bias = plan->zero_bias.as<float>(); lp.zbuf = zbuf;
  lp.t = sc.t.as<float>(); lp.tt = sc.tt.as<float>(); lp.ybuf = nullptr;
  lp.B = batch; lp.H = sc.H; lp.W = sc.W;
  lp.stagger = 0;
  return launch_layer<false, false, false>(sc, lp, s);
}

// Weight gradient (spectral_any.hip): the Geom it runs on, built on first use.  The build uploads tables and
// synchronises `s`, so the first call of a plan must not be inside a stream capture.
static int32_t spectral_wgrad_geom(const dlwp_spectral_plan* plan, hipStream_t s, sany::Geom** out) {
  sany::Geom* g = plan->gen.get();
  if (!g) {
    if (!plan->wgen) {
      std::unique_ptr<sany::Geom> w(new sany::Geom());
      const int32_t rc = sany::geom_build(*w, plan->ci, plan->co, plan->H, plan->W, (int)plan->rows_in.size(), plan->n_cols,
                                          plan->rows_in.data(), plan->rows_out.data(), plan->fwd_scale, plan->inv_scale, s);
      if (rc != DLWP_OK) return rc;
      plan->wgen = std::move(w);
    }
    g = plan->wgen.get();
  }
  const int32_t rc = sany::wgrad_prepare(*g, s);
  if (rc != DLWP_OK) return rc;
  *out = g;
  return DLWP_OK;
}

extern "C" size_t dlwp_spectral_conv2d_wgrad_workspace_bytes(const dlwp_spectral_plan* plan, int32_t batch) {
  if (!plan || batch <= 0) return 0;
  // shape arithmetic only: the same for gen and for the Geom a specialised plan would build
  const size_t nm = plan->gen ? (size_t)plan->gen->nr * plan->gen->nc : plan->rows_in.size() * (size_t)plan->n_cols;
  return align_up(nm * batch * plan->ci * sizeof(float2), 256) + align_up(nm * batch * plan->co * sizeof(float2), 256) +
         align_up(nm * plan->ci * plan->co * sizeof(float2), 256);
}

extern "C" int32_t dlwp_spectral_conv2d_wgrad_f32(const dlwp_spectral_plan* plan, const float* x, const float* grad_y,
                                                  float* grad_w, int32_t batch, void* workspace, size_t workspace_bytes,
                                                  void* stream) {
  DLWP_REQUIRE(plan && x && grad_y && grad_w && workspace, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(batch > 0, DLWP_ERR_INVALID_ARGUMENT, "batch must be positive");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  sany::Geom* g = nullptr;
  const int32_t rc = spectral_wgrad_geom(plan, s, &g);
  if (rc != DLWP_OK) return rc;
  const size_t need = sany::wgrad_workspace_bytes(*g, batch);
  DLWP_REQUIRE(workspace_bytes >= need, DLWP_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, need);
  DLWP_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(grad_y) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(grad_w) & 7) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 255) == 0,
               DLWP_ERR_INVALID_ARGUMENT, "x / grad_y must be 16-byte, grad_w 8-byte, workspace 256-byte aligned");
  return sany::run_wgrad(*g, x, grad_y, grad_w, batch, workspace, s);
}
