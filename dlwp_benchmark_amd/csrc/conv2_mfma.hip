// The U-Net family's other convolutions -- zero-padded Conv2d (1x1 shortcuts and heads, the strided 3x3 down-sampling) and
// ConvTranspose2d (4x4 s2 p1, 2x2 s2 up-sampling) -- as implicit GEMMs on the bf16 matrix pipe (gfx950).
//
// The opt-in forms "bf16x6" and "bf16" of ops.conv2d / ops.conv_transpose2d; the one-thread-per-output kernels of conv2.hip
// stay the default.  Same semantics as conv2d_kernel / conv_transpose2d_kernel there (reference models/unet/unet.py:583-584,
// :879-881, :450, :533 and :719, :523): `pre_act` while staging, bias + resid + act in the epilogue, padding cells zero.
//
// Conventions of conv_mfma.hip: D[cout][pixel] += W[cout][tap, cin] X[tap, cin][pixel]; A = weights (packed once, one
// coalesced 1 KiB load per fragment), B = pixels (lane = pixel, 8 consecutive channels = one ds_read_b128 of an LDS image
// staged once per K-slab of 32 input channels, already converted: three images for the exact split of "bf16x6", one RNE
// image for "bf16"); fp32 accumulation; one writer per output, no atomics, no split-K: reruns are bit-identical.
//
// One workgroup (4 waves) = MFRAGS fragments of 16 GEMM pixels (a row of 16, or two rows of 8 on maps that waste less that
// way: a runtime choice here, the lane -> pixel map is only used outside the K loop) x NF x 16 output channels.
//   Conv2d, stride s: GEMM pixel = output pixel.  The input window of the tile, ((TH-1) s + k) x ((TW-1) s + k) pixels, is staged
//     with its columns split by parity when s = 2 (row = [even columns | odd columns]): lane i's pixel for tap kw is then cell
//     (kw % s) * plane + i + kw / s -- unit stride over the lanes, the conflict-free read of the 3x3 kernel, not the 4-way
//     conflict of reading every second pixel.  s = 1: MFRAGS = 8 (128 pixels); s = 2: MFRAGS = 2 (2 x 16 outputs, a 5 x 33 window for
//     k = 3: 170 cells) so that three images fit several times into a CU's 160 KiB.
//   ConvTranspose2d, stride 2, by output parity: output (2a + ph, 2b + pw) is a stride-1 convolution of the input around (a, b)
//     with the (k/2)^2 taps kh = (ph + pad) % 2 + 2 jh, ih = a + (ph + pad) / 2 - jh.  GEMM pixel = input pixel (a, b), MFRAGS = 8;
//     the tile with its +-1 halo (k = 4; none for k = 2) is staged once per slab and feeds BOTH column parities, whose
//     accumulators a lane combines into one 8-byte store: 16 lanes write 32 consecutive floats of an output row.  The row
//     parity rides on the grid (blockIdx.z), which keeps the accumulators at 2 per fragment.
#include "conv_mfma_common.hpp"

namespace dlwp {
namespace conv2m {

using convm::KSLAB;
using convm::PS;
using convm::apply_act;

struct Params {
  const float* x;            // [B][Cin][H][W]
  const u32x4* wp;           // packed weights, see dlwp_conv2d_mfma_pack_f32
  const float* bias;         // [Cout] or null
  const float* resid;        // [B][Cout][OH][OW] or null (Conv2d only): added after bias, before `act`
  float* y;                  // [B][Cout][OH][OW]
  int B, Cin, H, W, Cout, OH, OW, k, pad, act, pre_act;
  int kslabs, nfrags;        // ceil(Cin / 32), ceil(Cout / 16)
  int tw8;                   // fragment = 0: a row of 16 GEMM pixels, 1: two rows of 8
  int tiles_w;               // tiles across the GEMM pixel grid
  int ws;                    // stride of the staged window (Conv2d: its stride; transposed: 1)
  int wc, rowp, planew;      // window columns; cells per staged row (ws * planew); cells per column-parity plane
  int npix;                  // staged cells: window rows * rowp
  int halo;                  // transposed: 1 for k = 4, 0 for k = 2
};

// TR: ConvTranspose2d (two column parities per workgroup); MFRAGS: 16-pixel fragments per workgroup; NF: 16-channel output
// fragments per workgroup; NIMG: 3 bf16x6, 1 bf16.  Waves: WN along the output channels x WM along the pixels.
template <bool TR, int MFRAGS, int NF, int NIMG>
__global__ __launch_bounds__(256) void conv2_mfma_kernel(const Params p) {
  constexpr int WN = (NF >= 2 || MFRAGS == 2) ? 2 : 1, WM = 4 / WN, MF = MFRAGS / WM, NFW = NF / WN, NPW = TR ? 2 : 1;
  static_assert(MF >= 1 && NFW >= 1 && MF * WM == MFRAGS && NFW * WN == NF, "wave layout");
  extern __shared__ __attribute__((aligned(16))) unsigned s_dyn[];     // [NIMG][npix * PS] images, then int s_src[npix]
  int* s_src = reinterpret_cast<int*>(s_dyn + NIMG * p.npix * PS);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, g = lane >> 4;
  const int wm = wv / WN, wn = wv % WN;
  const int TWr = p.tw8 ? 8 : 16, THr = p.tw8 ? 2 * MFRAGS : MFRAGS;
  const int GH = TR ? p.H : p.OH, GW = TR ? p.W : p.OW;              // the GEMM pixel grid
  const int w0 = (blockIdx.x % p.tiles_w) * TWr, h0 = (blockIdx.x / p.tiles_w) * THr;
  const int b = blockIdx.y;
  const int ph = TR ? (int)(blockIdx.z & 1) : 0, chunk = TR ? (int)(blockIdx.z >> 1) : (int)blockIdx.z;
  const int HW = p.H * p.W, OHW = p.OH * p.OW;

  // sources of the staged cells: the same for every channel, resolved once; -1 = zero (padding, or a cell no tap reads)
  {
    const int ih0 = TR ? h0 - p.halo : h0 * p.ws - p.pad, iw0 = TR ? w0 - p.halo : w0 * p.ws - p.pad;
    for (int i = tid; i < p.npix; i += 256) {
      const int r = i / p.rowp, rem = i - r * p.rowp;
      const int plane = rem / p.planew, q = rem - plane * p.planew;
      const int c = q * p.ws + plane;
      const int ih = ih0 + r, iw = iw0 + c;
      s_src[i] = (c < p.wc && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W) ? ih * p.W + iw : -1;
    }
  }

  int hp0[MF];         // staged cell of tap (0, 0) for this lane's pixel of every M fragment
  bool live[MF];       // wave-uniform: the fragment has a row inside the grid
  int prow[MF], pcol; // this lane's GEMM pixel
  pcol = w0 + (p.tw8 ? (li & 7) : li);
#pragma unroll
  for (int m = 0; m < MF; ++m) {
    const int f = wm * MF + m;
    const int tr = p.tw8 ? 2 * f + (li >> 3) : f, tc = p.tw8 ? (li & 7) : li;
    hp0[m] = tr * p.ws * p.rowp + tc;
    live[m] = h0 + (p.tw8 ? 2 * f : f) < GH;
    prow[m] = h0 + tr;
  }
  const int nf0 = chunk * NF + wn * NFW;
  f32x4 acc[NFW][MF][NPW];
#pragma unroll
  for (int j = 0; j < NFW; ++j)
#pragma unroll
    for (int m = 0; m < MF; ++m)
#pragma unroll
      for (int w = 0; w < NPW; ++w) acc[j][m][w] = f32x4{0.f, 0.f, 0.f, 0.f};
  const size_t img_stride = (size_t)p.k * p.k * p.kslabs * p.nfrags * 64;
  const int kt = TR ? p.k / 2 : p.k;            // taps per axis of one GEMM
  const float* xb = p.x + (long long)b * p.Cin * HW;

  for (int ks = 0; ks < p.kslabs; ++ks) {
    __syncthreads();
    // one K group (8 channels) of one staged cell per item, cells fastest: eight loads in flight per thread, each a run of an
    // NCHW plane across the lanes; one 16-byte LDS store per image, in the pattern the taps read
    for (int i = tid; i < 4 * p.npix; i += 256) {
      const int kg = i / p.npix, pix = i - kg * p.npix;
      const int c = ks * KSLAB + 8 * kg;
      const int src = s_src[pix];
      float v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q)    // padding zeros stay zero (act(0) = 0), channels past Cin too
        v[q] = (src >= 0 && c + q < p.Cin) ? apply_act(xb[(c + q) * HW + src], p.pre_act) : 0.f;
      u32x4 part[3];
      convm::convert_group<NIMG>(v, part);
#pragma unroll
      for (int q = 0; q < NIMG; ++q) *reinterpret_cast<u32x4*>(&s_dyn[q * p.npix * PS + pix * PS + kg * 4]) = part[q];
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < NPW; ++w) {
      for (int th = 0; th < kt; ++th) {
        for (int tw = 0; tw < kt; ++tw) {
          int shift, tap;      // staged-cell offset of this tap's window, and its index in the pack
          if constexpr (TR) {
            const int kh0 = (ph + p.pad) & 1, kw0 = (w + p.pad) & 1;
            const int dh = (ph + p.pad - kh0) / 2 - th, dw = (w + p.pad - kw0) / 2 - tw;
            shift = (dh + p.halo) * p.rowp + (dw + p.halo);
            tap = (kh0 + 2 * th) * p.k + (kw0 + 2 * tw);
          } else {
            shift = th * p.rowp + (tw % p.ws) * p.planew + tw / p.ws;
            tap = th * p.k + tw;
          }
          u32x4 xf[MF][NIMG];
#pragma unroll
          for (int m = 0; m < MF; ++m)
#pragma unroll
            for (int q = 0; q < NIMG; ++q)
              xf[m][q] = *reinterpret_cast<const u32x4*>(&s_dyn[q * p.npix * PS + (hp0[m] + shift) * PS + g * 4]);
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
    if (prow[m] >= GH || pcol >= GW) continue;
#pragma unroll
    for (int j = 0; j < NFW; ++j) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = (nf0 + j) * 16 + 4 * g + r;
        if (co < p.Cout) {
          const float bv = p.bias ? p.bias[co] : 0.f;
          if constexpr (TR) {
            // both column parities of input pixel (a, b): outputs (2a + ph, 2b) and (2a + ph, 2b + 1), one 8-byte store
            const int o = co * OHW + (2 * prow[m] + ph) * p.OW + 2 * pcol;
            float2 v = {apply_act(acc[j][m][0][r] + bv, p.act), apply_act(acc[j][m][NPW - 1][r] + bv, p.act)};
            *reinterpret_cast<float2*>(yb + o) = v;
          } else {
            const int o = co * OHW + prow[m] * p.OW + pcol;
            float v = acc[j][m][0][r] + bv;
            if (rb) v += rb[o];
            yb[o] = apply_act(v, p.act);
          }
        }
      }
    }
  }
}

// weight [cout][cin][k][k] (transposed: [cin][cout][k][k]) -> three bf16 images [tap][slab][fragment][lane][8]: lane l of
// fragment nf holds output channel 16 nf + (l & 15), input channels 32 slab + 8 (l >> 4) + 0..7; zero outside
__global__ __launch_bounds__(256) void conv2_mfma_pack_kernel(const float* __restrict__ w, unsigned short* __restrict__ out,
                                                              int cout, int cin, int kk, int transposed, int kslabs,
                                                              int nfrags, long long total) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int e = (int)(i & 7), lane = (int)((i >> 3) & 63);
    long long rest = i >> 9;
    const int nf = (int)(rest % nfrags); rest /= nfrags;
    const int ks = (int)(rest % kslabs);
    const int tap = (int)(rest / kslabs);
    const int co = nf * 16 + (lane & 15), c = ks * KSLAB + 8 * (lane >> 4) + e;
    float v = 0.f;
    if (co < cout && c < cin) v = transposed ? w[((long long)c * cout + co) * kk + tap] : w[((long long)co * cin + c) * kk + tap];
    convm::pack_store(v, out, i, total);
  }
}

}  // namespace conv2m
}  // namespace dlwp

using namespace dlwp;

namespace {

constexpr int kMaxLds = 64 * 1024;      // dynamic LDS a launch may ask for without a function attribute

// the kernel instance and the staged window of a shape.  GH x GW: the GEMM pixel grid (Conv2d: the output; transposed: the
// input); ws: the window's stride (Conv2d: its stride; transposed: 1)
struct Variant {
  int tw, mfrags, nf, tiles, tiles_w, wc, rowp, planew, npix;
};

Variant choose_variant(bool tr, int B, int GH, int GW, int nfrags, int k, int ws) {
  Variant v;
  // Conv2d s = 2 stages (TH - 1) 2 + k rows of 2 TW + k - 1 columns: a 128-pixel tile would need 17 x 33 cells, 3 x 54 KiB
  v.mfrags = (!tr && ws == 2) ? 2 : 8;
  // tile: as conv_mfma.hip's choose_variant -- the fewer live 16-pixel fragments, on a tie rows of 16
  const long long frags16 = (long long)((GW + 15) / 16) * GH, frags8 = (long long)((GW + 7) / 8) * ((GH + 1) / 2);
  const bool narrow = frags8 < frags16;
  v.tw = narrow ? 8 : 16;
  const int th = narrow ? 2 * v.mfrags : v.mfrags;
  v.tiles_w = (GW + v.tw - 1) / v.tw;
  v.tiles = v.tiles_w * ((GH + th - 1) / th);
  // output fragments per workgroup: 4 while the layer still makes >= 512 workgroups (the transposed kernel makes two per
  // tile and channel chunk, one per row parity); the 32-pixel tile has two wave columns, so at least 2
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

size_t lds_bytes(const Variant& v, int nimg) { return (size_t)v.npix * (nimg * conv2m::PS * 4 + 4); }

bool conv_geometry_ok(int k, int stride, int pad) { return k >= 1 && k <= 4 && (stride == 1 || stride == 2) && pad >= 0 && pad < k; }
bool transposed_geometry_ok(int k, int stride, int pad) { return stride == 2 && ((k == 4 && pad == 1) || (k == 2 && pad == 0)); }

template <bool TR, int MFRAGS, int NIMG>
void launch_nf(const conv2m::Params& p, int nf, dim3 grid, size_t lds, hipStream_t s) {
  if (nf == 4) hipLaunchKernelGGL((conv2m::conv2_mfma_kernel<TR, MFRAGS, 4, NIMG>), grid, dim3(256), lds, s, p);
  else if (nf == 2) hipLaunchKernelGGL((conv2m::conv2_mfma_kernel<TR, MFRAGS, 2, NIMG>), grid, dim3(256), lds, s, p);
  else if constexpr (MFRAGS != 2) hipLaunchKernelGGL((conv2m::conv2_mfma_kernel<TR, MFRAGS, 1, NIMG>), grid, dim3(256), lds, s, p);
}

// shape checks both launch entries share; fills the Params fields that follow from the variant
int32_t check_and_fill(conv2m::Params& p, bool tr, int form, Variant& v, const char* name) {
  DLWP_REQUIRE(form == 0 || form == 1, DLWP_ERR_INVALID_ARGUMENT, "%s: unknown form %d (0 bf16x6, 1 bf16)", name, form);
  DLWP_REQUIRE(p.B <= 65535, DLWP_ERR_UNSUPPORTED, "%s: batch %d exceeds the grid's y dimension", name, p.B);
  // offsets inside one sample (channel plane + pixel) are 32-bit in the kernel; the tile count and the window sources too
  const long long HW = (long long)p.H * p.W, OHW = (long long)p.OH * p.OW;
  DLWP_REQUIRE(((long long)p.H + 40) * ((long long)p.W + 40) < (1ll << 31) && ((long long)p.OH + 40) * ((long long)p.OW + 40) < (1ll << 31),
               DLWP_ERR_UNSUPPORTED, "%s: maps of %d x %d -> %d x %d exceed the kernel's 32-bit offsets", name, p.H, p.W, p.OH, p.OW);
  DLWP_REQUIRE((long long)p.Cin < (1ll << 31) - 64 && ((long long)p.Cin + 32) * HW < (1ll << 31) && (long long)p.Cout * OHW < (1ll << 31),
               DLWP_ERR_UNSUPPORTED, "%s: %d -> %d channels of %d x %d -> %d x %d exceed the kernel's 32-bit offsets", name, p.Cin,
               p.Cout, p.H, p.W, p.OH, p.OW);
  p.kslabs = (p.Cin + conv2m::KSLAB - 1) / conv2m::KSLAB; p.nfrags = (p.Cout + 15) / 16;
  DLWP_REQUIRE(p.nfrags * 2 <= 65535, DLWP_ERR_UNSUPPORTED, "%s: %d output channels exceed the grid's z dimension", name, p.Cout);
  const int ws = tr ? 1 : (p.ws);
  v = choose_variant(tr, p.B, tr ? p.H : p.OH, tr ? p.W : p.OW, p.nfrags, p.k, ws);
  DLWP_REQUIRE(lds_bytes(v, 3) <= (size_t)kMaxLds, DLWP_ERR_UNSUPPORTED, "%s: window of %d cells exceeds the LDS budget", name, v.npix);
  p.tw8 = v.tw == 8; p.tiles_w = v.tiles_w; p.ws = ws; p.wc = v.wc; p.rowp = v.rowp; p.planew = v.planew; p.npix = v.npix;
  p.halo = tr ? (p.k == 4 ? 1 : 0) : 0;
  return DLWP_OK;
}

}  // namespace

extern "C" size_t dlwp_conv2d_mfma_packed_bytes(int32_t cout, int32_t cin, int32_t k) {
  if (cout <= 0 || cin <= 0 || k <= 0 || k > 4) return 0;
  const long long kslabs = ((long long)cin + conv2m::KSLAB - 1) / conv2m::KSLAB, nfrags = ((long long)cout + 15) / 16;
  if (kslabs * nfrags > (1ll << 21)) return 0;                         // 3 KiB per (slab, fragment) and tap: past 2 GiB already
  const long long bytes = 3ll * k * k * kslabs * nfrags * 1024;
  return bytes < (1ll << 31) ? (size_t)bytes : 0;
}

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

extern "C" int32_t dlwp_conv2d_mfma_pack_f32(const float* weight_dev, int32_t cout, int32_t cin, int32_t k, int32_t transposed,
                                             void* packed_dev, void* stream) {
  DLWP_REQUIRE(weight_dev && packed_dev, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  const size_t bytes = dlwp_conv2d_mfma_packed_bytes(cout, cin, k);
  DLWP_REQUIRE(bytes > 0, DLWP_ERR_UNSUPPORTED, "conv2d_mfma: unsupported shape cout=%d cin=%d k=%d", cout, cin, k);
  const int kslabs = (cin + conv2m::KSLAB - 1) / conv2m::KSLAB, nfrags = (cout + 15) / 16;
  const long long total = (long long)(bytes / 6);               // bf16 elements per image
  long long blocks = (total + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(conv2m::conv2_mfma_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     weight_dev, reinterpret_cast<unsigned short*>(packed_dev), cout, cin, k * k, transposed != 0, kslabs, nfrags,
                     total);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" int32_t dlwp_conv2d_mfma_f32(const float* x, const void* packed, const float* bias, const float* resid, float* y,
                                        int32_t batch, int32_t cin, int32_t H, int32_t W, int32_t cout, int32_t k, int32_t stride,
                                        int32_t pad, int32_t pre_act, int32_t act, int32_t form, void* stream) {
  DLWP_REQUIRE(x && packed && y, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(batch > 0 && cin > 0 && cout > 0 && H > 0 && W > 0 && k > 0 && stride > 0 && pad >= 0, DLWP_ERR_INVALID_ARGUMENT, "bad shape");
  DLWP_REQUIRE(act >= 0 && act <= 4 && pre_act >= 0 && pre_act <= 4, DLWP_ERR_INVALID_ARGUMENT, "unknown activation");
  DLWP_REQUIRE(conv_geometry_ok(k, stride, pad), DLWP_ERR_UNSUPPORTED,
               "conv2d_mfma: k=%d stride=%d pad=%d has no matrix-pipe kernel (k <= 4, stride 1 or 2, pad < k)", k, stride, pad);
  DLWP_REQUIRE(dlwp_conv2d_mfma_packed_bytes(cout, cin, k) > 0, DLWP_ERR_UNSUPPORTED,
               "conv2d_mfma: unsupported shape cout=%d cin=%d k=%d", cout, cin, k);
  const long long OH = ((long long)H + 2 * pad - k) / stride + 1, OW = ((long long)W + 2 * pad - k) / stride + 1;
  DLWP_REQUIRE(OH > 0 && OW > 0 && (long long)H + 2 * pad >= k && (long long)W + 2 * pad >= k, DLWP_ERR_INVALID_ARGUMENT, "empty output");
  DLWP_REQUIRE(OH < (1ll << 31) && OW < (1ll << 31), DLWP_ERR_UNSUPPORTED, "conv2d_mfma: output too large");
  conv2m::Params p;
  p.x = x; p.wp = reinterpret_cast<const u32x4*>(packed); p.bias = bias; p.resid = resid; p.y = y;
  p.B = batch; p.Cin = cin; p.H = H; p.W = W; p.Cout = cout; p.OH = (int)OH; p.OW = (int)OW; p.k = k; p.pad = pad;
  p.act = act; p.pre_act = pre_act; p.ws = stride;
  Variant v;
  const int32_t rc = check_and_fill(p, false, form, v, "conv2d_mfma");
  if (rc != DLWP_OK) return rc;
  const int nimg = form == 0 ? 3 : 1;
  const dim3 grid(v.tiles, batch, (p.nfrags + v.nf - 1) / v.nf);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (v.mfrags == 8) form == 0 ? launch_nf<false, 8, 3>(p, v.nf, grid, lds_bytes(v, nimg), s) : launch_nf<false, 8, 1>(p, v.nf, grid, lds_bytes(v, nimg), s);
  else form == 0 ? launch_nf<false, 2, 3>(p, v.nf, grid, lds_bytes(v, nimg), s) : launch_nf<false, 2, 1>(p, v.nf, grid, lds_bytes(v, nimg), s);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" int32_t dlwp_conv_transpose2d_mfma_f32(const float* x, const void* packed, const float* bias, float* y, int32_t batch,
                                                  int32_t cin, int32_t H, int32_t W, int32_t cout, int32_t k, int32_t stride,
                                                  int32_t pad, int32_t act, int32_t form, void* stream) {
  DLWP_REQUIRE(x && packed && y, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(batch > 0 && cin > 0 && cout > 0 && H > 0 && W > 0 && k > 0 && stride > 0 && pad >= 0, DLWP_ERR_INVALID_ARGUMENT, "bad shape");
  DLWP_REQUIRE(act >= 0 && act <= 4, DLWP_ERR_INVALID_ARGUMENT, "unknown activation %d", act);
  DLWP_REQUIRE(transposed_geometry_ok(k, stride, pad), DLWP_ERR_UNSUPPORTED,
               "conv_transpose2d_mfma: k=%d stride=%d pad=%d has no matrix-pipe kernel (4x4 s2 p1 and 2x2 s2 p0 have)", k, stride, pad);
  DLWP_REQUIRE(dlwp_conv2d_mfma_packed_bytes(cout, cin, k) > 0, DLWP_ERR_UNSUPPORTED,
               "conv_transpose2d_mfma: unsupported shape cout=%d cin=%d k=%d", cout, cin, k);
  DLWP_REQUIRE(H < (1 << 30) && W < (1 << 30), DLWP_ERR_UNSUPPORTED, "conv_transpose2d_mfma: output too large");
  DLWP_REQUIRE((reinterpret_cast<uintptr_t>(y) & 7) == 0, DLWP_ERR_INVALID_ARGUMENT, "conv_transpose2d_mfma: y must be 8-byte aligned");
  conv2m::Params p;
  p.x = x; p.wp = reinterpret_cast<const u32x4*>(packed); p.bias = bias; p.resid = nullptr; p.y = y;
  p.B = batch; p.Cin = cin; p.H = H; p.W = W; p.Cout = cout; p.OH = 2 * H; p.OW = 2 * W; p.k = k; p.pad = pad;   // both geometries double
  p.act = act; p.pre_act = 0; p.ws = 1;
  Variant v;
  const int32_t rc = check_and_fill(p, true, form, v, "conv_transpose2d_mfma");
  if (rc != DLWP_OK) return rc;
  const int nimg = form == 0 ? 3 : 1;
  const dim3 grid(v.tiles, batch, 2 * ((p.nfrags + v.nf - 1) / v.nf));       // z = channel chunk * 2 + output row parity
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  form == 0 ? launch_nf<true, 8, 3>(p, v.nf, grid, lds_bytes(v, nimg), s) : launch_nf<true, 8, 1>(p, v.nf, grid, lds_bytes(v, nimg), s);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}
