// The U-Net / ConvLSTM / diffusion backbones' convolutions as implicit GEMMs on the bf16 matrix pipe (gfx950), one kernel for
//   * pad(1) + Conv2d(3x3) on cat([x0, x1], 1) under CylinderPad or HEALPixPadding                (dlwp_conv3x3_mfma_f32),
//   * the zero-padded k x k Conv2d, stride 1 or 2: 1x1 shortcuts and heads, the strided 3x3       (dlwp_conv2d_mfma_f32),
//   * ConvTranspose2d 4x4 s2 p1 and 2x2 s2                                                        (dlwp_conv_transpose2d_mfma_f32).
//
// The opt-in forms "bf16x6" and "bf16" of ops.conv3x3*, ops.conv2d and ops.conv_transpose2d; the kernels of conv.hip and
// conv2.hip stay the default.  Same semantics as those (reference utils/utils.py:11-26; utils/healpix.py:316-368;
// models/unet/unet.py:450-470, :512-533, :553, :583-584, :719, :879-886, :901; models/convlstm/convlstm.py:47-55, :94,
// :148-157): `pre_act` while staging, the layer's padding rule, bias + resid + act in the epilogue.
//
// D[cout][pixel] += W[cout][tap, cin] X[tap, cin][pixel], K walked as slabs of 32 input channels x the taps.  One workgroup
// (4 waves) = MFRAGS fragments of 16 GEMM pixels (a row of 16, or two rows of 8 on maps that waste less that way) of one sample
// x NF x 16 output channels:
//   * per slab the window of input cells the tile's taps reach is staged ONCE into LDS, channel-innermost, already converted
//     (bf16x6: the exact three-part split, one LDS image per part; bf16: the RNE value); where each cell comes from is the same
//     for every channel, so it is resolved once per workgroup into a source table.  The taps read shifted windows of the image
//     as MFMA B operands (lane = pixel, 8 consecutive channels = one ds_read_b128);
//   * the weights are packed once (dlwp_conv2d_mfma_pack_f32) in A-operand order, [image][tap][slab][16-channel fragment][lane]
//     [8 bf16], so a fragment is one coalesced 1 KiB global load; cin is zero-filled to the slab, cout to 16;
//   * A = weights, B = pixels: accumulator register r of lane l is channel 4 (l >> 4) + r of pixel l & 15, so a store
//     instruction writes runs of 16 (or 8) consecutive pixels of the NCHW output.
// No atomics, no split-K across workgroups: one writer per output, reruns are bit-identical.
//
// What the layers do not share is a geometry policy: where a staged cell comes from (locate, fetch), which window and pack
// index a tap has (kt, tap), and the store.
//   Padded3x3<TW>     compile-time tile (8 x 16 or 16 x 8 pixels) and 10 x 18 / 18 x 10 window, nine unrolled taps; a cell is the
//                     circular longitude or the HEALPix ring table's one or two cells (a synthesised corner is their mean) of
//                     either input segment.
//   ZeroPadWindow<MFRAGS>  runtime k and stride s; GEMM pixel = output pixel.  The window, ((TH-1) s + k) x ((TW-1) s + k) cells, is
//                     staged with its columns split by parity when s = 2 (row = [even columns | odd columns]): lane i's cell for tap
//                     kw is then (kw % s) * plane + i + kw / s -- unit stride over the lanes, the conflict-free read of the 3x3 tile,
//                     not the 4-way conflict of every second cell.  s = 1: MFRAGS = 8; s = 2: MFRAGS = 2 (2 x 16 outputs, a 5 x 33
//                     window for k = 3: 170 cells) so that three images fit several times into a CU's 160 KiB.
//   TransposedParity  stride 2 by output parity: output (2a + ph, 2b + pw) is a stride-1 convolution of the input around (a, b) with
//                     the (k/2)^2 taps kh = (ph + pad) % 2 + 2 jh, ih = a + (ph + pad) / 2 - jh.  GEMM pixel = input pixel (a, b);
//                     the tile with its +-1 halo (k = 4; none for k = 2) feeds BOTH column parities, whose accumulators a lane
//                     combines into one 8-byte store: 16 lanes write 32 consecutive floats of an output row.  The row parity
//                     rides on the grid (blockIdx.z), which keeps the accumulators at 2 per fragment.
//   DgradParity       the input gradient of the stride-2 Conv2d (dlwp_conv2d_dgrad_mfma_f32): TransposedParity's staging and taps
//                     on a GEMM pixel grid that comes from the map it writes, and a cropping store.  The stride-1 input gradient
//                     is ZeroPadWindow<8> itself on a pack with the channels exchanged and the taps reversed.
// The staging loop stands in the kernel body and indexes the LDS array itself (conv_wgrad.hip's note on staging functions).
#include "act_common.hpp"

namespace dlwp {
namespace convm {

using actc::apply_act;

constexpr int KSLAB = 32;    // input channels per K-slab: one v_mfma_f32_16x16x32_bf16 per tap and slab
// dwords per staged cell in LDS (16 hold the 32 channels).  24: the four 16-lane groups of a ds_read_b128 (lanes
// {0-3, 12-15, 20-27}, ...) then start at bank (6 i + g) * 4 mod 64 for cell i, channel group g -- even for one g, odd for
// the other, all distinct over a row of 16 cells: reads of 16 consecutive staged cells are conflict-free (16 would be 4-way,
// 20 2-way).  Where a fragment is two rows of 8 pixels, lanes 0-3 and 12-15 of a group can meet 2-way.  The staging stores are
// 16-byte stores of consecutive cells, the same address pattern as the reads.
constexpr int PS = 24;

// eight consecutive channels of one staged cell -> one 16-byte B-operand group per image (NIMG 3: the exact three-part
// split of form "bf16x6"; NIMG 1: the RNE value of form "bf16")
template <int NIMG>
__device__ __forceinline__ void convert_group(const float (&v)[8], u32x4 (&part)[3]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    unsigned h, m, l;
    if (NIMG == 3) split3_pair(v[2 * q], v[2 * q + 1], h, m, l);
    else { h = cvt_pk_bf16(v[2 * q], v[2 * q + 1]); m = 0u; l = 0u; }
    part[0][q] = h; part[1][q] = m; part[2][q] = l;
  }
}

struct Params {
  const float* x0; int c0;   // first input segment [B][c0][H][W]: the whole input except under Padded3x3
  const float* x1; int c1;   // Padded3x3: second segment or null
  const u32x4* wp;           // packed weights, see dlwp_conv2d_mfma_pack_f32
  const float* bias;         // [Cout] or null
  const float* resid;        // [B][Cout][OH][OW] or null (not transposed): added after bias, before `act`
  float* y;                  // [B][Cout][OH][OW]
  int B, H, W, Cout, OH, OW, k, pad, act, pre_act;
  const int2* hpx;           // Padded3x3: HEALPix ring table (null = cylinder), as conv::Params::hpx
  int kslabs, nfrags;        // ceil(cin / 32), ceil(Cout / 16)
  int GH, GW;                // the GEMM pixel grid: the output; transposed: the input
  int tw8;                   // fragment = 0: a row of 16 GEMM pixels, 1: two rows of 8
  int tiles_w;               // tiles across the GEMM pixel grid
  int ws;                    // stride of the staged window (Conv2d: its stride; otherwise 1)
  int wc, rowp, planew;      // window columns; cells per staged row (ws * planew); cells per column-parity plane
  int npix;                  // staged cells: window rows * rowp
  int wpad;                  // rows and columns the window begins before the tile's first input pixel (Conv2d: pad;
                             // transposed: 1 for k = 4, 0 for k = 2)
};

// One GEMM per workgroup and the plain NCHW store with the residual: everything but the transposed layer
struct PlainStore {
  static constexpr int NPW = 1;        // accumulators per fragment (output column parities)
  static constexpr int ROWPAR = 1;     // output row parities on blockIdx.z
  static __device__ __forceinline__ void store(const Params& p, float* yb, const float* rb, int co_off, int, int prow, int pcol,
                                               const float (&a)[1], float bv) {
    const int o = co_off + prow * p.OW + pcol;
    float v = a[0] + bv;
    if (rb) v += rb[o];
    yb[o] = apply_act(v, p.act);
  }
};

template <int TW_>
struct Padded3x3 : PlainStore {
  static constexpr int MFRAGS = 8, TW = TW_, TH = 128 / TW, HWD = TW + 2, NPIX = (TH + 2) * HWD;
  static_assert(NPIX == 180, "(8 + 2) * (16 + 2) = (16 + 2) * (8 + 2) cells");
  using Source = int4;                 // (sample a, pixel a, sample b, pixel b); sample < 0: none
  static __device__ __forceinline__ int npix(const Params&) { return NPIX; }
  static __device__ __forceinline__ bool tw8(const Params&) { return TW == 8; }
  static __device__ __forceinline__ int row_step(const Params&) { return HWD; }   // staged cells from a GEMM row to the next
  // the padding rules of conv3x3_cyl_kernel
  static __device__ __forceinline__ Source locate(const Params& p, int b, int h0, int w0, int i) {
    const int HW = p.H * p.W;
    const int r = i / HWD, cc = i % HWD;
    const int ih = h0 + r - 1;
    int iw = w0 + cc - 1;
    int4 e = {-1, 0, -1, 0};                                     // x < 0: zero
    if (p.hpx) {
      if (ih >= -1 && ih <= p.H && iw >= -1 && iw <= p.W) {
        if (ih >= 0 && ih < p.H && iw >= 0 && iw < p.W) {
          e.x = b; e.y = ih * p.W + iw;
        } else {
          const int face = b % 12, s0 = b - face;
          const int2 t = p.hpx[(long long)face * (p.H + 2) * (p.W + 2) + (ih + 1) * (p.W + 2) + (iw + 1)];
          const int fa = t.x / HW;
          e.x = s0 + fa; e.y = t.x - fa * HW;
          if (t.y >= 0) {
            const int fb = t.y / HW;
            e.z = s0 + fb; e.w = t.y - fb * HW;
          }
        }
      }
    } else if (ih >= 0 && ih < p.H && iw >= -1 && iw <= p.W) {
      iw = iw < 0 ? iw + p.W : (iw >= p.W ? iw - p.W : iw);      // circular longitude
      e.x = b; e.y = ih * p.W + iw;
    }
    return e;
  }
  // the padded, activated fp32 value of channel c; padding zeros stay zero (act(0) = 0)
  static __device__ __forceinline__ float fetch(const Params& p, int, const int4 e, int c, int HW) {
    if (e.x < 0 || c >= p.c0 + p.c1) return 0.f;
    const bool seg0 = c < p.c0;
    const float* base = seg0 ? p.x0 : p.x1;
    const int cs = seg0 ? p.c0 : p.c1, cl = seg0 ? c : c - p.c0;
    float v = apply_act(base[(long long)e.x * cs * HW + (cl * HW + e.y)], p.pre_act);
    // a synthesised corner is the mean of two cells of the ACTIVATED tensor (the reference pads after the activation)
    if (e.z >= 0) v = 0.5f * v + 0.5f * apply_act(base[(long long)e.z * cs * HW + (cl * HW + e.w)], p.pre_act);
    return v;
  }
  // taps per axis of one GEMM, and tap (th, tw) of output parity (ph, pw): the staged-cell offset of its window and its index
  // in the pack
  static constexpr int KT = 3;         // compile-time: the kernel unrolls the taps
  static __device__ __forceinline__ int kt(const Params&) { return KT; }
  static __device__ __forceinline__ void tap(const Params&, int, int, int th, int tw, int& shift, int& tap) {
    shift = th * HWD + tw; tap = th * 3 + tw;
  }
};

template <int MFRAGS_>
struct ZeroPadWindow : PlainStore {
  static constexpr int MFRAGS = MFRAGS_;
  using Source = int;                  // pixel of this sample; -1 = zero (padding, or a cell no tap reads)
  static __device__ __forceinline__ int npix(const Params& p) { return p.npix; }
  static __device__ __forceinline__ bool tw8(const Params& p) { return p.tw8; }
  static __device__ __forceinline__ int row_step(const Params& p) { return p.ws * p.rowp; }
  static __device__ __forceinline__ Source locate(const Params& p, int, int h0, int w0, int i) {
    const int r = i / p.rowp, rem = i - r * p.rowp;
    const int plane = rem / p.planew, q = rem - plane * p.planew;
    const int c = q * p.ws + plane;
    const int ih = h0 * p.ws - p.wpad + r, iw = w0 * p.ws - p.wpad + c;
    return (c < p.wc && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W) ? ih * p.W + iw : -1;
  }
  // padding zeros stay zero (act(0) = 0), channels past the layer too
  static __device__ __forceinline__ float fetch(const Params& p, int b, int src, int c, int HW) {
    return (src >= 0 && c < p.c0) ? apply_act((p.x0 + (long long)b * p.c0 * HW)[c * HW + src], p.pre_act) : 0.f;
  }
  static constexpr int KT = 0;         // runtime: the taps stay loops
  static __device__ __forceinline__ int kt(const Params& p) { return p.k; }
  static __device__ __forceinline__ void tap(const Params& p, int, int, int th, int tw, int& shift, int& tap) {
    shift = th * p.rowp + (tw % p.ws) * p.planew + tw / p.ws; tap = th * p.k + tw;
  }
};

struct TransposedParity : ZeroPadWindow<8> {
  static constexpr int NPW = 2, ROWPAR = 2;
  static __device__ __forceinline__ int kt(const Params& p) { return p.k / 2; }
  static __device__ __forceinline__ void tap(const Params& p, int ph, int pw, int th, int tw, int& shift, int& tap) {
    const int kh0 = (ph + p.pad) & 1, kw0 = (pw + p.pad) & 1;
    const int dh = (ph + p.pad - kh0) / 2 - th, dw = (pw + p.pad - kw0) / 2 - tw;
    shift = (dh + p.wpad) * p.rowp + (dw + p.wpad);
    tap = (kh0 + 2 * th) * p.k + (kw0 + 2 * tw);
  }
  // both column parities of input pixel (a, b): outputs (2a + ph, 2b) and (2a + ph, 2b + 1), one 8-byte store
  static __device__ __forceinline__ void store(const Params& p, float* yb, const float*, int co_off, int ph, int prow, int pcol,
                                               const float (&a)[2], float bv) {
    const int o = co_off + (2 * prow + ph) * p.OW + 2 * pcol;
    float2 v = {apply_act(a[0] + bv, p.act), apply_act(a[1] + bv, p.act)};
    *reinterpret_cast<float2*>(yb + o) = v;
  }
};

// The input gradient of Conv2d(k, stride 2, pad): the parity form again, driven by the map it WRITES.  dx (OH x OW here) row
// 2a + ph collects gz (H x W here) rows a + (ph + pad - kh0) / 2 - jh through taps kh = kh0 + 2 jh -- TransposedParity's
// arithmetic with the Conv2d weight [cout][cin][k][k] read as the ConvTranspose2d weight it is.  An odd k arrives zero-extended
// to k + 1 at the high tap index (the pack's k_packed), so p.k is even.  GEMM pixel (a, b), a < ceil(OH / 2), b < ceil(OW / 2):
// gz cells outside its map stage as zeros (ZeroPadWindow::locate), so rows and columns of dx that no output read come out as
// computed zeros; the store crops to OH x OW.  OW may be odd and dx may lie at any 4-byte offset: two scalar stores.
struct DgradParity : TransposedParity {
  static __device__ __forceinline__ void store(const Params& p, float* yb, const float*, int co_off, int ph, int prow, int pcol,
                                               const float (&a)[2], float) {
    const int row = 2 * prow + ph, col = 2 * pcol;
    if (row >= p.OH) return;
    float* d = yb + (co_off + row * p.OW + col);
    if (col < p.OW) d[0] = a[0];
    if (col + 1 < p.OW) d[1] = a[1];
  }
};

// G: the geometry policy; NF: 16-channel output fragments per workgroup; NIMG: 3 bf16x6, 1 bf16.
// Waves: WN along the output channels x WM along the pixels; each owns NFW x MF accumulator fragments per column parity.
template <class G, int NF, int NIMG>
__global__ __launch_bounds__(256) void conv_mfma_kernel(const Params p) {
  constexpr int MFRAGS = G::MFRAGS, NPW = G::NPW;
  constexpr int WN = (NF >= 2 || MFRAGS == 2) ? 2 : 1, WM = 4 / WN, MF = MFRAGS / WM, NFW = NF / WN;
  static_assert(MF >= 1 && NFW >= 1 && MF * WM == MFRAGS && NFW * WN == NF, "wave layout");
  using Source = typename G::Source;
  extern __shared__ __attribute__((aligned(16))) unsigned s_dyn[];     // [NIMG][npix * PS] images, then Source s_src[npix]
  const int npix = G::npix(p);
  Source* s_src = reinterpret_cast<Source*>(s_dyn + NIMG * npix * PS);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, g = lane >> 4;
  const int wm = wv / WN, wn = wv % WN;
  const bool tw8 = G::tw8(p);
  const int TWr = tw8 ? 8 : 16, THr = tw8 ? 2 * MFRAGS : MFRAGS;
  const int w0 = (blockIdx.x % p.tiles_w) * TWr, h0 = (blockIdx.x / p.tiles_w) * THr;
  const int b = blockIdx.y;
  const int ph = (int)(blockIdx.z % G::ROWPAR), chunk = (int)(blockIdx.z / G::ROWPAR);
  const int HW = p.H * p.W, OHW = p.OH * p.OW;

  // sources of the staged cells: the same for every channel, so resolved once
  for (int i = tid; i < npix; i += 256) s_src[i] = G::locate(p, b, h0, w0, i);

  int hp0[MF];         // staged cell of tap (0, 0) for this lane's pixel of every M fragment
  bool live[MF];       // wave-uniform: the fragment has a row inside the grid
#pragma unroll
  for (int m = 0; m < MF; ++m) {
    const int f = wm * MF + m;
    hp0[m] = (tw8 ? 2 * f + (li >> 3) : f) * G::row_step(p) + (tw8 ? (li & 7) : li);
    live[m] = h0 + (tw8 ? 2 * f : f) < p.GH;
  }
  const int nf0 = chunk * NF + wn * NFW;
  f32x4 acc[NFW][MF][NPW];
#pragma unroll
  for (int j = 0; j < NFW; ++j)
#pragma unroll
    for (int m = 0; m < MF; ++m)
#pragma unroll
      for (int w = 0; w < NPW; ++w) acc[j][m][w] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int UNROLL = G::KT ? G::KT : 1;     // compile-time taps are unrolled, runtime taps stay loops
  const int kt = G::kt(p);                      // taps per axis of one GEMM
  const size_t img_stride = (size_t)p.k * p.k * p.kslabs * p.nfrags * 64;

  for (int ks = 0; ks < p.kslabs; ++ks) {
    __syncthreads();
    // one K group (8 channels) of one staged cell per item, cells fastest: eight loads in flight per thread, each a run of an
    // NCHW plane across the lanes; one 16-byte LDS store per image, in the pattern the taps read
    for (int i = tid; i < 4 * npix; i += 256) {
      const int kg = i / npix, pix = i - kg * npix;
      const int c = ks * KSLAB + 8 * kg;
      const Source e = s_src[pix];
      float v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = G::fetch(p, b, e, c + q, HW);
      u32x4 part[3];
      convert_group<NIMG>(v, part);
#pragma unroll
      for (int q = 0; q < NIMG; ++q) *reinterpret_cast<u32x4*>(&s_dyn[q * npix * PS + pix * PS + kg * 4]) = part[q];
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < NPW; ++w) {
#pragma unroll UNROLL
      for (int th = 0; th < kt; ++th) {
#pragma unroll UNROLL
        for (int tw = 0; tw < kt; ++tw) {
          int shift, tap;      // staged-cell offset of this tap's window, and its index in the pack
          G::tap(p, ph, w, th, tw, shift, tap);
          u32x4 xf[MF][NIMG];
#pragma unroll
          for (int m = 0; m < MF; ++m)
#pragma unroll
            for (int q = 0; q < NIMG; ++q)
              xf[m][q] = *reinterpret_cast<const u32x4*>(&s_dyn[q * npix * PS + (hp0[m] + shift) * PS + g * 4]);
#pragma unroll
          for (int j = 0; j < NFW; ++j) {
            const int nf = nf0 + j;
            if (nf < p.nfrags) {
              u32x4 wf[NIMG];
              const size_t o = (((size_t)tap * p.kslabs + ks) * p.nfrags + nf) * 64 + lane;
#pragma unroll
              for (int q = 0; q < NIMG; ++q) wf[q] = p.wp[q * img_stride + o];
#pragma unroll
              for (int m = 0; m < MF; ++m) {
                if (live[m]) {
                  if constexpr (NIMG == 3) acc[j][m][w] = mfma_bf16x6(wf, xf[m], acc[j][m][w]);
                  else acc[j][m][w] = mfma16x16x32_bf16(wf[0], xf[m][0], acc[j][m][w]);
                }
              }
            }
          }
        }
      }
    }
  }

  float* yb = p.y + (long long)b * p.Cout * OHW;
  const float* rb = p.resid ? p.resid + (long long)b * p.Cout * OHW : nullptr;
#pragma unroll
  for (int m = 0; m < MF; ++m) {
    const int f = wm * MF + m;
    const int prow = h0 + (tw8 ? 2 * f + (li >> 3) : f), pcol = w0 + (tw8 ? (li & 7) : li);   // this lane's GEMM pixel
    if (prow >= p.GH || pcol >= p.GW) continue;
#pragma unroll
    for (int j = 0; j < NFW; ++j) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = (nf0 + j) * 16 + 4 * g + r;
        if (co < p.Cout) {
          float a[NPW];
#pragma unroll
          for (int w = 0; w < NPW; ++w) a[w] = acc[j][m][w][r];
          G::store(p, yb, rb, co * OHW, ph, prow, pcol, a, p.bias ? p.bias[co] : 0.f);
        }
      }
    }
  }
}

// weight [cout][cin][k][k] (transposed: [cin][cout][k][k]) -> three bf16 images [tap][slab][fragment][lane][8]: lane l of
// fragment nf holds output channel 16 nf + (l & 15), input channels 32 slab + 8 (l >> 4) + 0..7 (element 0 in the low half of
// dword 0); zero outside.  The pack has kp x kp taps, kp >= k: taps at index k and above are zero (the even window of
// DgradParity); flip: pack tap (th, tw) holds weight tap (k - 1 - th, k - 1 - tw) (the stride-1 adjoint)
__global__ __launch_bounds__(256) void conv_mfma_pack_kernel(const float* __restrict__ w, unsigned short* __restrict__ out,
                                                             int cout, int cin, int k, int kp, int transposed, int flip, int kslabs,
                                                             int nfrags, long long total) {
  const int kk = k * k;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int e = (int)(i & 7), lane = (int)((i >> 3) & 63);
    long long rest = i >> 9;
    const int nf = (int)(rest % nfrags); rest /= nfrags;
    const int ks = (int)(rest % kslabs);
    const int ptap = (int)(rest / kslabs);
    const int th = ptap / kp, tw = ptap - th * kp;
    const int tap = flip ? (k - 1 - th) * k + (k - 1 - tw) : th * k + tw;
    const int co = nf * 16 + (lane & 15), c = ks * KSLAB + 8 * (lane >> 4) + e;
    float v = 0.f;
    if (co < cout && c < cin && th < k && tw < k) v = transposed ? w[((long long)c * cout + co) * kk + tap] : w[((long long)co * cin + c) * kk + tap];
    unsigned h, m, l;
    split3_pair(v, 0.f, h, m, l);
    out[i] = (unsigned short)(h & 0xffffu);
    out[total + i] = (unsigned short)(m & 0xffffu);
    out[2 * total + i] = (unsigned short)(l & 0xffffu);
  }
}

}  // namespace convm
}  // namespace dlwp

using namespace dlwp;

namespace {

constexpr int kMaxLds = 64 * 1024;      // dynamic LDS a launch may ask for without a function attribute

enum Layer { PADDED3X3, CONV2D, TRANSPOSED, DGRAD_PARITY };

// the kernel instance and the staged window of a shape.  GH x GW: the GEMM pixel grid (the output; transposed: the input);
// ws: the window's stride (Conv2d: its stride; otherwise 1).  The padded 3x3 layer is (tr false, k 3, ws 1): a window of
// (TH + 2) x (TW + 2) = 180 cells
struct Variant {
  int tw, mfrags, nf, tiles, tiles_w, wc, rowp, planew, npix;
};

Variant choose_variant(bool tr, int B, int GH, int GW, int nfrags, int k, int ws) {
  Variant v;
  // Conv2d s = 2 stages (TH - 1) 2 + k rows of 2 TW + k - 1 columns: a 128-pixel tile would need 17 x 33 cells, 3 x 54 KiB
  v.mfrags = (!tr && ws == 2) ? 2 : 8;
  // tile: a 16-pixel MFMA fragment is one row of 16 or two rows of 8; fragments wholly below the grid are skipped, so the
  // cost of a shape is its count of live fragments -- take the smaller (8 x 8 maps: 4 against 8; 20 x 20: 30 against 40), on a
  // tie the rows of 16 (longer runs of consecutive pixels per load and store; every 16 | W map)
  const long long frags16 = (long long)((GW + 15) / 16) * GH, frags8 = (long long)((GW + 7) / 8) * ((GH + 1) / 2);
  const bool narrow = frags8 < frags16;
  v.tw = narrow ? 8 : 16;
  const int th = narrow ? 2 * v.mfrags : v.mfrags;
  v.tiles_w = (GW + v.tw - 1) / v.tw;
  v.tiles = v.tiles_w * ((GH + th - 1) / th);
  // output fragments per workgroup: 4 (64 channels: every staged window feeds the most MFMAs) while the layer still makes
  // >= 512 workgroups, 2 per CU (the transposed kernel makes two per tile and channel chunk, one per row parity); the 32-pixel
  // tile has two wave columns, so at least 2
  const int nfmin = v.mfrags == 2 ? 2 : 1;
  const long long wgs = (long long)v.tiles * B * (tr ? 2 : 1);      // per channel chunk
  int nf = 4;
  while (nf > nfmin && (nf / 2 >= nfrags || (wgs < 512 && wgs * ((nfrags + nf - 1) / nf) < 512))) nf /= 2;
  v.nf = nf;
  const int halo = tr ? (k == 4 ? 1 : 0) : 0;
  const int wr = tr ? th + 2 * halo : (th - 1) * ws + k;
  v.wc = tr ? v.tw + 2 * halo : (v.tw - 1) * ws + k;
  v.planew = (v.wc + ws - 1) / ws;
  v.rowp = ws * v.planew;
  v.npix = wr * v.rowp;
  return v;
}

size_t lds_bytes(const Variant& v, int nimg, Layer layer) {
  return (size_t)v.npix * (nimg * convm::PS * 4 + (layer == PADDED3X3 ? sizeof(int4) : sizeof(int)));
}

bool conv_geometry_ok(int k, int stride, int pad) { return k >= 1 && k <= 4 && (stride == 1 || stride == 2) && pad >= 0 && pad < k; }
bool transposed_geometry_ok(int k, int stride, int pad) { return stride == 2 && ((k == 4 && pad == 1) || (k == 2 && pad == 0)); }

template <class G, int NIMG>
void launch_nf(const convm::Params& p, int nf, dim3 grid, size_t lds, hipStream_t s) {
  if (nf == 4) hipLaunchKernelGGL((convm::conv_mfma_kernel<G, 4, NIMG>), grid, dim3(256), lds, s, p);
  else if (nf == 2) hipLaunchKernelGGL((convm::conv_mfma_kernel<G, 2, NIMG>), grid, dim3(256), lds, s, p);
  else if constexpr (G::MFRAGS != 2) hipLaunchKernelGGL((convm::conv_mfma_kernel<G, 1, NIMG>), grid, dim3(256), lds, s, p);
}

template <class G>
void launch_form(const convm::Params& p, int form, int nf, dim3 grid, size_t lds, hipStream_t s) {
  form == 0 ? launch_nf<G, 3>(p, nf, grid, lds, s) : launch_nf<G, 1>(p, nf, grid, lds, s);
}

// What the launch entries share.  `p` arrives with its tensors, H, W, OH, OW, k, pad and ws described; the checks of
// form, activations, the grid's y and z, the kernel's 32-bit offsets (inside one sample: channel plane + pixel; the tile
// count and the window sources too) and the pack's size, then the variant, the Params fields that follow from it, and the launch.
// `check` stops before the launch and leaves the variant in `v`: what the entries and the dgrad query both run.
// DGRAD_PARITY: p.H x p.W is the map read (gz), p.OH x p.OW the map written (dx), and the GEMM pixel grid is one pixel per 2 x 2
// block of the map written, ceil(OH / 2) x ceil(OW / 2).
int32_t check(convm::Params& p, Layer layer, int form, const char* name, Variant& v) {
  const bool tr = layer == TRANSPOSED || layer == DGRAD_PARITY;
  DLWP_REQUIRE(p.act >= 0 && p.act <= 4 && p.pre_act >= 0 && p.pre_act <= 4, DLWP_ERR_INVALID_ARGUMENT, "%s: unknown activation",
               name);
  DLWP_REQUIRE(form == 0 || form == 1, DLWP_ERR_INVALID_ARGUMENT, "%s: unknown form %d (0 bf16x6, 1 bf16)", name, form);
  DLWP_REQUIRE(p.B <= 65535, DLWP_ERR_UNSUPPORTED, "%s: batch %d exceeds the grid's y dimension", name, p.B);
  const long long HW = (long long)p.H * p.W, OHW = (long long)p.OH * p.OW;
  const long long cin = (long long)p.c0 + p.c1, cseg = p.c0 > p.c1 ? p.c0 : p.c1;
  DLWP_REQUIRE(((long long)p.H + 40) * ((long long)p.W + 40) < (1ll << 31) && ((long long)p.OH + 40) * ((long long)p.OW + 40) < (1ll << 31),
               DLWP_ERR_UNSUPPORTED, "%s: maps of %d x %d -> %d x %d exceed the kernel's 32-bit offsets", name, p.H, p.W, p.OH, p.OW);
  DLWP_REQUIRE(cin < (1ll << 31) - 64 && (cseg + 32) * HW < (1ll << 31) && (long long)p.Cout * OHW < (1ll << 31),
               DLWP_ERR_UNSUPPORTED, "%s: %lld -> %d channels of %d x %d -> %d x %d exceed the kernel's 32-bit offsets", name, cin,
               p.Cout, p.H, p.W, p.OH, p.OW);
  p.kslabs = (int)((cin + convm::KSLAB - 1) / convm::KSLAB); p.nfrags = (int)(((long long)p.Cout + 15) / 16);
  DLWP_REQUIRE(p.nfrags * 2 <= 65535, DLWP_ERR_UNSUPPORTED, "%s: %d output channels exceed the grid's z dimension", name, p.Cout);
  DLWP_REQUIRE(dlwp_conv2d_mfma_packed_bytes(p.Cout, (int32_t)cin, p.k) > 0, DLWP_ERR_UNSUPPORTED,
               "%s: unsupported shape cout=%d cin=%lld k=%d", name, p.Cout, cin, p.k);
  if (layer == DGRAD_PARITY) { p.GH = p.OH / 2 + (p.OH & 1); p.GW = p.OW / 2 + (p.OW & 1); }    // no OH + 1: OH may be INT_MAX
  else { p.GH = tr ? p.H : p.OH; p.GW = tr ? p.W : p.OW; }
  v = choose_variant(tr, p.B, p.GH, p.GW, p.nfrags, p.k, p.ws);
  DLWP_REQUIRE(lds_bytes(v, 3, layer) <= (size_t)kMaxLds, DLWP_ERR_UNSUPPORTED, "%s: window of %d cells exceeds the LDS budget", name, v.npix);
  p.tw8 = v.tw == 8; p.tiles_w = v.tiles_w; p.wc = v.wc; p.rowp = v.rowp; p.planew = v.planew; p.npix = v.npix;
  p.wpad = tr ? (p.k == 4 ? 1 : 0) : p.pad;
  return DLWP_OK;
}

int32_t launch_checked(const convm::Params& p, Layer layer, int form, const Variant& v, hipStream_t s) {
  const bool tr = layer == TRANSPOSED || layer == DGRAD_PARITY;
  const dim3 grid(v.tiles, p.B, (tr ? 2 : 1) * ((p.nfrags + v.nf - 1) / v.nf));    // transposed: z = channel chunk * 2 + output row parity
  const size_t lds = lds_bytes(v, form == 0 ? 3 : 1, layer);
  if (layer == PADDED3X3) {
    if (v.tw == 8) launch_form<convm::Padded3x3<8>>(p, form, v.nf, grid, lds, s);
    else launch_form<convm::Padded3x3<16>>(p, form, v.nf, grid, lds, s);
  } else if (layer == DGRAD_PARITY) {
    launch_nf<convm::DgradParity, 3>(p, v.nf, grid, lds, s);        // the gradient has the one fp32-grade form
  } else if (tr) {
    launch_form<convm::TransposedParity>(p, form, v.nf, grid, lds, s);
  } else if (v.mfrags == 8) {
    launch_form<convm::ZeroPadWindow<8>>(p, form, v.nf, grid, lds, s);
  } else {
    launch_form<convm::ZeroPadWindow<2>>(p, form, v.nf, grid, lds, s);
  }
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

int32_t check_and_launch(convm::Params& p, Layer layer, int form, const char* name, hipStream_t s) {
  Variant v;
  const int32_t status = check(p, layer, form, name, v);
  return status != DLWP_OK ? status : launch_checked(p, layer, form, v, s);
}

}  // namespace

extern "C" size_t dlwp_conv2d_mfma_packed_bytes(int32_t cout, int32_t cin, int32_t k) {
  if (cout <= 0 || cin <= 0 || k <= 0 || k > 4) return 0;
  const long long kslabs = ((long long)cin + convm::KSLAB - 1) / convm::KSLAB, nfrags = ((long long)cout + 15) / 16;
  if (kslabs * nfrags > (1ll << 21)) return 0;                         // 3 KiB per (slab, fragment) and tap: past 2 GiB already
  const long long bytes = 3ll * k * k * kslabs * nfrags * 1024;
  return bytes < (1ll << 31) ? (size_t)bytes : 0;
}

extern "C" size_t dlwp_conv3x3_mfma_packed_bytes(int32_t cout, int32_t cin) { return dlwp_conv2d_mfma_packed_bytes(cout, cin, 3); }

// 16 * fragment width (16: rows of 16 GEMM pixels, 8: two rows of 8) + output fragments per workgroup, the launchers' own rule
extern "C" int32_t dlwp_conv2d_mfma_variant(int32_t transposed, int32_t batch, int32_t H, int32_t W, int32_t cout, int32_t k,
                                            int32_t stride, int32_t pad) {
  if (batch <= 0 || H <= 0 || W <= 0 || cout <= 0) return 0;
  if (transposed ? !transposed_geometry_ok(k, stride, pad) : !conv_geometry_ok(k, stride, pad)) return 0;
  long long GH = H, GW = W;
  if (!transposed) {
    if ((long long)H + 2 * pad < k || (long long)W + 2 * pad < k) return 0;
    GH = ((long long)H + 2 * pad - k) / stride + 1; GW = ((long long)W + 2 * pad - k) / stride + 1;
  }
  if (GH <= 0 || GW <= 0 || (GH + 40) * (GW + 40) >= (1ll << 31)) return 0;
  const Variant v = choose_variant(transposed != 0, batch, (int)GH, (int)GW, (int)(((long long)cout + 15) / 16), k, transposed ? 1 : stride);
  return v.tw * 16 + v.nf;
}

extern "C" int32_t dlwp_conv3x3_mfma_variant(int32_t batch, int32_t H, int32_t W, int32_t cout) {
  return dlwp_conv2d_mfma_variant(0, batch, H, W, cout, 3, 1, 1);
}

static int32_t pack(const char* name, const float* weight_dev, int32_t cout, int32_t cin, int32_t k, int32_t k_packed,
                    int32_t transposed, int32_t flip, void* packed_dev, void* stream) {
  DLWP_REQUIRE(weight_dev && packed_dev, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(k >= 1 && k_packed >= k, DLWP_ERR_INVALID_ARGUMENT, "%s: k=%d does not fit a pack of %d x %d taps", name, k, k_packed, k_packed);
  const size_t bytes = dlwp_conv2d_mfma_packed_bytes(cout, cin, k_packed);
  DLWP_REQUIRE(bytes > 0, DLWP_ERR_UNSUPPORTED, "%s: unsupported shape cout=%d cin=%d k=%d", name, cout, cin, k_packed);
  const int kslabs = (cin + convm::KSLAB - 1) / convm::KSLAB, nfrags = (cout + 15) / 16;
  const long long total = (long long)(bytes / 6);               // bf16 elements per image
  long long blocks = (total + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(convm::conv_mfma_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     weight_dev, reinterpret_cast<unsigned short*>(packed_dev), cout, cin, k, k_packed, transposed != 0, flip != 0,
                     kslabs, nfrags, total);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" int32_t dlwp_conv2d_mfma_pack_f32(const float* weight_dev, int32_t cout, int32_t cin, int32_t k, int32_t transposed,
                                             void* packed_dev, void* stream) {
  return pack("conv2d_mfma", weight_dev, cout, cin, k, k, transposed, 0, packed_dev, stream);
}

extern "C" int32_t dlwp_conv3x3_mfma_pack_f32(const float* weight_dev, int32_t cout, int32_t cin, void* packed_dev,
                                              void* stream) {
  return pack("conv3x3_mfma", weight_dev, cout, cin, 3, 3, 0, 0, packed_dev, stream);
}

extern "C" int32_t dlwp_conv3x3_mfma_f32(const float* x0, int32_t c0, const float* x1, int32_t c1, const void* packed,
                                         const float* bias, const float* resid, float* y, int32_t batch, int32_t H, int32_t W,
                                         int32_t cout, int32_t pre_act, int32_t act, const int32_t* ring_table, int32_t form,
                                         void* stream) {
  DLWP_REQUIRE(x0 && packed && y, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(batch > 0 && H > 0 && W > 0 && c0 > 0 && cout > 0 && c1 >= 0, DLWP_ERR_INVALID_ARGUMENT, "bad shape");
  DLWP_REQUIRE(c1 == 0 || x1, DLWP_ERR_INVALID_ARGUMENT, "second segment pointer missing");
  if (ring_table) {
    DLWP_REQUIRE(batch % 12 == 0, DLWP_ERR_INVALID_ARGUMENT, "n_faces=%d is not a multiple of 12", batch);
    DLWP_REQUIRE((long long)12 * H * W < (1ll << 31), DLWP_ERR_INVALID_ARGUMENT, "face too large for the 32-bit table");
  } else {
    DLWP_REQUIRE(W > 1, DLWP_ERR_INVALID_ARGUMENT, "bad shape");
  }
  convm::Params p = {};
  p.x0 = x0; p.c0 = c0; p.x1 = x1; p.c1 = c1; p.wp = reinterpret_cast<const u32x4*>(packed); p.bias = bias; p.resid = resid;
  p.y = y; p.B = batch; p.H = H; p.W = W; p.Cout = cout; p.OH = H; p.OW = W; p.k = 3; p.pad = 1; p.act = act; p.pre_act = pre_act;
  p.hpx = reinterpret_cast<const int2*>(ring_table); p.ws = 1;
  return check_and_launch(p, PADDED3X3, form, "conv3x3_mfma", reinterpret_cast<hipStream_t>(stream));
}

extern "C" int32_t dlwp_conv2d_mfma_f32(const float* x, const void* packed, const float* bias, const float* resid, float* y,
                                        int32_t batch, int32_t cin, int32_t H, int32_t W, int32_t cout, int32_t k, int32_t stride,
                                        int32_t pad, int32_t pre_act, int32_t act, int32_t form, void* stream) {
  DLWP_REQUIRE(x && packed && y, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(batch > 0 && cin > 0 && cout > 0 && H > 0 && W > 0 && k > 0 && stride > 0 && pad >= 0, DLWP_ERR_INVALID_ARGUMENT, "bad shape");
  DLWP_REQUIRE(conv_geometry_ok(k, stride, pad), DLWP_ERR_UNSUPPORTED,
               "conv2d_mfma: k=%d stride=%d pad=%d has no matrix-pipe kernel (k <= 4, stride 1 or 2, pad < k)", k, stride, pad);
  const long long OH = ((long long)H + 2 * pad - k) / stride + 1, OW = ((long long)W + 2 * pad - k) / stride + 1;
  DLWP_REQUIRE(OH > 0 && OW > 0 && (long long)H + 2 * pad >= k && (long long)W + 2 * pad >= k, DLWP_ERR_INVALID_ARGUMENT, "empty output");
  DLWP_REQUIRE(OH < (1ll << 31) && OW < (1ll << 31), DLWP_ERR_UNSUPPORTED, "conv2d_mfma: output too large");
  convm::Params p = {};
  p.x0 = x; p.c0 = cin; p.wp = reinterpret_cast<const u32x4*>(packed); p.bias = bias; p.resid = resid; p.y = y;
  p.B = batch; p.H = H; p.W = W; p.Cout = cout; p.OH = (int)OH; p.OW = (int)OW; p.k = k; p.pad = pad;
  p.act = act; p.pre_act = pre_act; p.ws = stride;
  return check_and_launch(p, CONV2D, form, "conv2d_mfma", reinterpret_cast<hipStream_t>(stream));
}

extern "C" int32_t dlwp_conv_transpose2d_mfma_f32(const float* x, const void* packed, const float* bias, float* y, int32_t batch,
                                                  int32_t cin, int32_t H, int32_t W, int32_t cout, int32_t k, int32_t stride,
                                                  int32_t pad, int32_t act, int32_t form, void* stream) {
  DLWP_REQUIRE(x && packed && y, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(batch > 0 && cin > 0 && cout > 0 && H > 0 && W > 0 && k > 0 && stride > 0 && pad >= 0, DLWP_ERR_INVALID_ARGUMENT, "bad shape");
  DLWP_REQUIRE(transposed_geometry_ok(k, stride, pad), DLWP_ERR_UNSUPPORTED,
               "conv_transpose2d_mfma: k=%d stride=%d pad=%d has no matrix-pipe kernel (4x4 s2 p1 and 2x2 s2 p0 have)", k, stride, pad);
  DLWP_REQUIRE(H < (1 << 30) && W < (1 << 30), DLWP_ERR_UNSUPPORTED, "conv_transpose2d_mfma: output too large");
  DLWP_REQUIRE((reinterpret_cast<uintptr_t>(y) & 7) == 0, DLWP_ERR_INVALID_ARGUMENT, "conv_transpose2d_mfma: y must be 8-byte aligned");
  convm::Params p = {};
  p.x0 = x; p.c0 = cin; p.wp = reinterpret_cast<const u32x4*>(packed); p.bias = bias; p.y = y;
  p.B = batch; p.H = H; p.W = W; p.Cout = cout; p.OH = 2 * H; p.OW = 2 * W; p.k = k; p.pad = pad;   // both geometries double
  p.act = act; p.ws = 1;
  return check_and_launch(p, TRANSPOSED, form, "conv_transpose2d_mfma", reinterpret_cast<hipStream_t>(stream));
}

extern "C" int32_t dlwp_conv2d_mfma_pack_ex_f32(const float* weight_dev, int32_t cout, int32_t cin, int32_t k, int32_t k_packed,
                                                int32_t exchange, int32_t flip, void* packed_dev, void* stream) {
  return pack("conv2d_mfma_pack_ex", weight_dev, cout, cin, k, k_packed, exchange, flip, packed_dev, stream);
}

namespace {

// The input gradient of Conv2d(cin -> cout, k, stride, pad) on an H x W map, as the launcher runs it.  Stride 1: the Conv2d
// forward of gz with padding k - 1 - pad (pack: channels exchanged, taps reversed, k_packed = k).  Stride 2: DgradParity on
// the even window k_packed = k + k % 2 (pack: channels exchanged, taps as they lie, zero-extended); a 2 x 2 window has no halo,
// so it takes pad 0 alone, a 4 x 4 window reaches one cell either way, which covers pad 0, 1 and 2.
struct DgradPlan {
  Layer layer;
  int k_packed, flip;
  long long SH, SW;          // gz's map
};

bool dgrad_plan(int32_t H, int32_t W, int32_t k, int32_t stride, int32_t pad, DgradPlan& d) {
  if (!conv_geometry_ok(k, stride, pad)) return false;
  if ((long long)H + 2 * pad < k || (long long)W + 2 * pad < k) return false;
  d.SH = ((long long)H + 2 * pad - k) / stride + 1; d.SW = ((long long)W + 2 * pad - k) / stride + 1;
  if (stride == 1) { d.layer = CONV2D; d.k_packed = k; d.flip = 1; return true; }
  d.layer = DGRAD_PARITY; d.k_packed = k + (k & 1); d.flip = 0;
  return d.k_packed == 2 ? pad == 0 : pad <= 2;
}

// the Params of the launch (tensors aside) and every check of it short of the launch
int32_t dgrad_check(convm::Params& p, const DgradPlan& d, int32_t batch, int32_t cin, int32_t cout, int32_t H, int32_t W, int32_t k,
                    int32_t pad, Variant& v) {
  p.c0 = cout; p.B = batch; p.H = (int)d.SH; p.W = (int)d.SW; p.Cout = cin; p.OH = H; p.OW = W; p.k = d.k_packed;
  p.pad = d.layer == CONV2D ? k - 1 - pad : pad; p.ws = 1;
  return check(p, d.layer, 0, "conv2d_dgrad_mfma", v);
}

}  // namespace

// 4096 * k_packed + 1024 * policy (0: ZeroPadWindow<8> on the reversed pack, stride 1; 1: DgradParity, stride 2) + 16 * fragment
// width + output fragments per workgroup; 0 for what dlwp_conv2d_dgrad_mfma_f32 refuses
extern "C" int32_t dlwp_conv2d_dgrad_mfma_variant(int32_t batch, int32_t cin, int32_t cout, int32_t H, int32_t W, int32_t k,
                                                  int32_t stride, int32_t pad) {
  if (batch <= 0 || cin <= 0 || cout <= 0 || H <= 0 || W <= 0 || k <= 0 || stride <= 0 || pad < 0) return 0;
  DgradPlan d;
  if (!dgrad_plan(H, W, k, stride, pad, d) || d.SH <= 0 || d.SW <= 0 || d.SH >= (1ll << 31) || d.SW >= (1ll << 31)) return 0;
  convm::Params p = {};
  Variant v;
  if (dgrad_check(p, d, batch, cin, cout, H, W, k, pad, v) != DLWP_OK) return 0;
  return 4096 * d.k_packed + 1024 * (d.layer == DGRAD_PARITY) + 16 * v.tw + v.nf;
}

extern "C" int32_t dlwp_conv2d_dgrad_mfma_f32(const float* gz, const void* packed, float* dx, int32_t batch, int32_t cin, int32_t H,
                                              int32_t W, int32_t cout, int32_t k, int32_t stride, int32_t pad, void* stream) {
  DLWP_REQUIRE(gz && packed && dx, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(batch > 0 && cin > 0 && cout > 0 && H > 0 && W > 0 && k > 0 && stride > 0 && pad >= 0, DLWP_ERR_INVALID_ARGUMENT, "bad shape");
  DgradPlan d;
  DLWP_REQUIRE(dgrad_plan(H, W, k, stride, pad, d), DLWP_ERR_UNSUPPORTED,
               "conv2d_dgrad_mfma: k=%d stride=%d pad=%d on %d x %d has no matrix-pipe kernel (stride 1: k <= 4, pad < k; stride 2: "
               "k 1 or 2 with pad 0, k 3 or 4 with pad <= 2; an output map of at least one pixel)", k, stride, pad, H, W);
  DLWP_REQUIRE(d.SH > 0 && d.SW > 0, DLWP_ERR_INVALID_ARGUMENT, "empty output");
  DLWP_REQUIRE(d.SH < (1ll << 31) && d.SW < (1ll << 31), DLWP_ERR_UNSUPPORTED, "conv2d_dgrad_mfma: output too large");
  convm::Params p = {};
  p.x0 = gz; p.wp = reinterpret_cast<const u32x4*>(packed); p.y = dx;
  Variant v;
  const int32_t status = dgrad_check(p, d, batch, cin, cout, H, W, k, pad, v);
  if (status != DLWP_OK) return status;
  return launch_checked(p, d.layer, 0, v, reinterpret_cast<hipStream_t>(stream));
}
