// Device-side types and helpers shared by the two FNO kernel files: fno_unfused.hpp (one kernel per stage) and
// fno_trunk.hpp (the fused step / rollout kernel).  Everything here is a struct, a constant or a __forceinline__ function;
// no kernel is defined or instantiated from this header.
#pragma once

#include "common.hpp"

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
    gelu_erf8(a1[0][0], a1[0][1]);
    __builtin_amdgcn_sched_barrier(0);
    unit_mfma(bgm, qm, I1{});
    gelu_erf8(a1[1][0], a1[1][1]);
    __builtin_amdgcn_sched_barrier(0);
    unit_mfma(bgm, qm, I2{});
    unit_split(bgv);
    __builtin_amdgcn_sched_barrier(0);
  };
  // prologue: unit 0 (tile pair 0, chains 0-1) on the fp32 lanes only
  unit_valu_fc1(0, I0{});
  gelu_erf8(a1[0][0], a1[0][1]);
  gelu_erf8(a1[1][0], a1[1][1]);
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

// Projection MLP of one 64-pixel row segment (see pw_proj_bf16x6_kernel): bx = the 32 input channels of the
// lane's 4 pixels as bf16x3 B operands (k order = whatever s_w1 was packed for), po[co][q] = this lane group's
// partial sum of output co at pixel 4 j + q (to be reduced over the 4 lane groups).
template <int CO, bool F16 = false>
__device__ __forceinline__ void proj_segment(const u32x4 (&bx)[4][3], const u32x4* s_w1, const float* s_b1,
                                             const float* s_w2, int ntile, int lane, float (&po)[CO][4], float f16_down = 1.f) {
  // F16: s_b1 holds b1 * 2^(11+s) and layer 1 comes out at that scale (common.hpp): one multiply per element in front of the GELU
  const int g = lane >> 4;
  // Every loop-carried value lives in ONE register set (a back-edge without copies, DESIGN.md section 4.6 "projection loop"):
  //   a[q]      layer-1 accumulators.  A half first forms x = a (x f16_down) of its two pixel chains, which leaves a dead, and the
  //             matrix instructions of the NEXT tile then write a in place, under the GELU of x
  //   ga, gb    GELU outputs of pixels 0-1 / 2-3.  ga is consumed by the layer-2 FMAs of half 1 of the same trip, gb by half 0 of
  //             the next trip, before half 1 rewrites it
  //   wa, bb    layer-1 operands, fetched from LDS right behind the last matrix instruction that reads them (they travel under
  //             the second GELU and the loop tail); w2v likewise behind the FMAs of half 0 (tile t - 1 -> t)
  u32x4 wa[3];
  f32x4 bb, w2v[CO];
  auto load_l1 = [&](int t) {
#pragma unroll
    for (int pp = 0; pp < 3; ++pp) wa[pp] = s_w1[(t * 3 + pp) * 64 + lane];
    bb = *reinterpret_cast<const f32x4*>(s_b1 + 16 * t + 4 * g);
  };
  auto load_l2 = [&](int t) {
#pragma unroll
    for (int co = 0; co < CO; ++co) w2v[co] = *reinterpret_cast<const f32x4*>(s_w2 + (t * CO + co) * 16 + 4 * g);
  };
  auto down = [&](const f32x4& a) -> f32x4 { return F16 ? a * f16_down : a; };
#pragma unroll
  for (int co = 0; co < CO; ++co)
#pragma unroll
    for (int q = 0; q < 4; ++q) po[co][q] = 0.f;
  // layer 2 of pixels q0, q0 + 1: the 16 hidden units of the tile w2v holds, on PLAIN v_fma_f32.  These FMAs sit between the
  // matrix instructions of the half, where a packed one costs far more than the two plain ones it replaces (MI355X: +22 cycles
  // beside an MFMA); hipcc SLP-packs the two pixels' chains whenever it can see both, so each chain runs between two empty asm
  // statements that make its accumulator opaque (no instruction, no constraint on order: the asm is not volatile)
  auto fma2 = [&](int q0, const f32x4(&gg)[2]) {
#pragma unroll
    for (int co = 0; co < CO; ++co)
#pragma unroll
      for (int qq = 0; qq < 2; ++qq) {
        float acc = po[co][q0 + qq];
        asm("" : "+v"(acc));
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = fmaf(w2v[co][r], gg[qq][r], acc);
        asm("" : "+v"(acc));
        po[co][q0 + qq] = acc;
      }
  };
  f32x4 a[4], ga[2], gb[2];
  // prologue: layer 1 of tiles 0 and 1, GELU of tile 0, layer 2 of its pixels 0-1
  load_l1(0);
#pragma unroll
  for (int q = 0; q < 4; ++q) a[q] = mfma_x<F16>(wa, bx[q], bb);
  load_l1(ntile > 1 ? 1 : 0);
  load_l2(0);
  ga[0] = down(a[0]); ga[1] = down(a[1]);
  gb[0] = down(a[2]); gb[1] = down(a[3]);
#pragma unroll
  for (int q = 0; q < 4; ++q) a[q] = mfma_x<F16>(wa, bx[q], bb);
  load_l1(ntile > 2 ? 2 : ntile - 1);
  gelu_erf8(ga[0], ga[1]);
  gelu_erf8(gb[0], gb[1]);
  fma2(0, ga);
  // trip t: matrix pipe = layer 1 of tile min(t + 1, ntile - 1); fp32 lanes = GELU of tile t, layer 2 of pixels 2-3 of tile t - 1
  // (half 0) and of pixels 0-1 of tile t (half 1).  sched_barrier keeps hipcc from moving a matrix instruction in front of the
  // multiply that frees its destination
  for (int t = 1; t < ntile; ++t) {
    ga[0] = down(a[0]); ga[1] = down(a[1]);
    __builtin_amdgcn_sched_barrier(0);
    a[0] = mfma_x<F16>(wa, bx[0], bb);
    a[1] = mfma_x<F16>(wa, bx[1], bb);
    gelu_erf8(ga[0], ga[1]);
    fma2(2, gb);
    load_l2(t);
    __builtin_amdgcn_sched_barrier(0);
    gb[0] = down(a[2]); gb[1] = down(a[3]);
    __builtin_amdgcn_sched_barrier(0);
    a[2] = mfma_x<F16>(wa, bx[2], bb);
    a[3] = mfma_x<F16>(wa, bx[3], bb);
    load_l1(t + 2 < ntile ? t + 2 : ntile - 1);
    gelu_erf8(gb[0], gb[1]);
    fma2(0, ga);
    __builtin_amdgcn_sched_barrier(0);
  }
  fma2(2, gb);   // pixels 2-3 of the last tile: w2v still holds it
}

// argument of fno_layer_kernel (fno_unfused.hpp); filled by the FNO step and by SpectralConv2d
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

__device__ __forceinline__ float2 cfma(float2 a, float2 b, float2 c) {
  return float2{fmaf(a.x, b.x, fmaf(-a.y, b.y, c.x)), fmaf(a.x, b.y, fmaf(a.y, b.x, c.y))};
}

// f16x3 products of the trunk's row phase (skip convolution + inverse W-DFT into ONE accumulator, forward W-DFT): the skip
// weights and the twiddles are packed with the SAME shift s = 3 (twiddles: max |t| = 1 -> [8, 16); skip weights must stay below 2,
// checked when the plan is made -- a plan with larger ones takes the bf16x6 form), so everything sits at 2^14 times the true scale
constexpr int kTrunkF16Shift = 3;
constexpr float kTrunkF16Up = 16384.0f, kTrunkF16Down = 1.0f / 16384.0f;

}  // namespace fno
}  // namespace dlwp
