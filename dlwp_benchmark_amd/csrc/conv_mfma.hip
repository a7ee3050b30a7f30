// pad(1) + Conv2d(3x3) of the U-Net / ConvLSTM / diffusion backbones as an implicit GEMM on the bf16 matrix pipe (gfx950).
//
// The opt-in forms "bf16x6" and "bf16" of ops.conv3x3*; the scalar-FMA direct kernel of conv.hip stays the default.  Same
// semantics as conv3x3_cyl_kernel (reference utils/utils.py:11-26; models/unet/unet.py:456-470, :512-525, :553, :886, :901;
// models/convlstm/convlstm.py:47-55, :94, :148-157; utils/healpix.py:316-368): two input segments (the folded torch.cat),
// `pre_act` while staging, either padding rule, bias + resid + act in the epilogue.
//
// One workgroup (4 waves) = one tile of 128 output pixels (8 x 16, or 16 x 8 on maps that waste less that way) of one
// sample and NF x 16 output channels.  GEMM per workgroup: D[cout][pixel] += W[cout][tap, cin] X[tap, cin][pixel], K walked
// as slabs of 32 input channels x 9 taps:
//   * per slab the (TH+2) x (TW+2) halo tile is staged ONCE into LDS, channel-innermost, already converted (bf16x6: the exact
//     three-part split, one LDS image per part; bf16: the RNE value) -- the nine taps read shifted windows of that image as
//     MFMA B operands (lane = pixel, 8 consecutive channels = one ds_read_b128);
//   * the weights are packed once (dlwp_conv3x3_mfma_pack_f32) in A-operand order, [image][tap][slab][16-channel fragment]
//     [lane][8 bf16], so a fragment is one coalesced 1 KiB global load; cin is zero-filled to the slab, cout to 16;
//   * A = weights, B = pixels: accumulator register r of lane l is channel 4 (l >> 4) + r of pixel l & 15, so a store
//     instruction writes runs of 16 (or 8) consecutive pixels of the NCHW output.
// No atomics, no split-K across workgroups: one writer per output, reruns are bit-identical.
#include "conv_mfma_common.hpp"

namespace dlwp {
namespace convm {

constexpr int HALO = 180;    // (8 + 2) * (16 + 2) = (16 + 2) * (8 + 2) halo pixels; PS dwords each (conv_mfma_common.hpp)

struct Params {
  const float* x0; int c0;   // first input segment [B][c0][H][W]
  const float* x1; int c1;   // second segment or null
  const u32x4* wp;           // packed weights, see dlwp_conv3x3_mfma_pack_f32
  const float* bias;         // [Cout] or null
  const float* resid;        // [B][Cout][H][W] or null: added after bias, before `act`
  float* y;                  // [B][Cout][H][W]
  int B, H, W, Cout, act, pre_act;
  const int2* hpx;           // HEALPix ring table (null = cylinder), as conv::Params::hpx
  int kslabs, nfrags;        // ceil(cin / 32), ceil(Cout / 16)
};

// the padded, activated fp32 value of channel c at a halo pixel whose sources are e = (sample a, pixel a, sample b, pixel b)
__device__ __forceinline__ float fetch(const Params& p, const int4 e, int c, int HW) {
  if (c >= p.c0 + p.c1) return 0.f;
  const bool seg0 = c < p.c0;
  const float* base = seg0 ? p.x0 : p.x1;
  const int cs = seg0 ? p.c0 : p.c1, cl = seg0 ? c : c - p.c0;
  float v = apply_act(base[(long long)e.x * cs * HW + (cl * HW + e.y)], p.pre_act);
  // a synthesised corner is the mean of two cells of the ACTIVATED tensor (the reference pads after the activation)
  if (e.z >= 0) v = 0.5f * v + 0.5f * apply_act(base[(long long)e.z * cs * HW + (cl * HW + e.w)], p.pre_act);
  return v;
}

// TW: tile width (16 -> 8 x 16 pixels, 8 -> 16 x 8); NF: 16-channel output fragments per workgroup; NIMG: 3 bf16x6, 1 bf16.
// Waves: WN along the output channels x WM along the pixels; each owns NFW x MF accumulator fragments.
template <int TW, int NF, int NIMG>
__global__ __launch_bounds__(256) void conv3x3_mfma_kernel(const Params p) {
  constexpr int TH = 128 / TW, HWD = TW + 2;
  constexpr int WN = NF >= 2 ? 2 : 1, WM = 4 / WN, MF = 8 / WM, NFW = NF / WN;
  static_assert((TH + 2) * HWD == HALO, "halo size");
  __shared__ __attribute__((aligned(16))) unsigned s_x[NIMG][HALO * PS];
  __shared__ int4 s_src[HALO];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, g = lane >> 4;
  const int wm = wv / WN, wn = wv % WN;
  const int tiles_w = (p.W + TW - 1) / TW;
  const int w0 = (blockIdx.x % tiles_w) * TW, h0 = (blockIdx.x / tiles_w) * TH;
  const int b = blockIdx.y;
  const int HW = p.H * p.W;

  // sources of the halo pixels: the same for every channel, so resolved once (padding rules of conv3x3_cyl_kernel)
  for (int i = tid; i < HALO; i += 256) {
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
    s_src[i] = e;
  }

  int hp0[MF];         // halo pixel of tap (0, 0) for this lane's pixel of every M fragment
  bool live[MF];       // wave-uniform: the fragment has a row inside the map
#pragma unroll
  for (int m = 0; m < MF; ++m) {
    const int f = wm * MF + m;
    if (TW == 16) { hp0[m] = f * HWD + li; live[m] = h0 + f < p.H; }
    else { hp0[m] = (2 * f + (li >> 3)) * HWD + (li & 7); live[m] = h0 + 2 * f < p.H; }
  }
  const int nf0 = blockIdx.z * NF + wn * NFW;
  f32x4 acc[NFW][MF];
#pragma unroll
  for (int j = 0; j < NFW; ++j)
#pragma unroll
    for (int m = 0; m < MF; ++m) acc[j][m] = f32x4{0.f, 0.f, 0.f, 0.f};
  const size_t img_stride = (size_t)9 * p.kslabs * p.nfrags * 64;

  for (int ks = 0; ks < p.kslabs; ++ks) {
    __syncthreads();
    // one K group (8 channels) of one halo pixel per item, pixels fastest: eight loads in flight per thread, each a coalesced
    // row of an NCHW plane across the lanes; one 16-byte LDS store per image, in the pattern the taps read
    for (int i = tid; i < 4 * HALO; i += 256) {
      const int kg = i / HALO, pix = i - kg * HALO;
      const int c = ks * KSLAB + 8 * kg;
      const int4 e = s_src[pix];
      float v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = e.x >= 0 ? fetch(p, e, c + q, HW) : 0.f;   // padding zeros stay zero (act(0) = 0)
      u32x4 part[3];
      convert_group<NIMG>(v, part);
#pragma unroll
      for (int q = 0; q < NIMG; ++q) *reinterpret_cast<u32x4*>(&s_x[q][pix * PS + kg * 4]) = part[q];
    }
    __syncthreads();
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int shift = (tap / 3) * HWD + (tap % 3);
      u32x4 xf[MF][NIMG];
#pragma unroll
      for (int m = 0; m < MF; ++m)
#pragma unroll
        for (int q = 0; q < NIMG; ++q) xf[m][q] = *reinterpret_cast<const u32x4*>(&s_x[q][(hp0[m] + shift) * PS + g * 4]);
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
              if constexpr (NIMG == 3) acc[j][m] = mfma_bf16x6(wf, xf[m], acc[j][m]);
              else acc[j][m] = mfma16x16x32_bf16(wf[0], xf[m][0], acc[j][m]);
            }
          }
        }
      }
    }
  }

#pragma unroll
  for (int m = 0; m < MF; ++m) {
    const int f = wm * MF + m;
    const int oh = TW == 16 ? h0 + f : h0 + 2 * f + (li >> 3);
    const int ow = TW == 16 ? w0 + li : w0 + (li & 7);
    if (oh >= p.H || ow >= p.W) continue;
#pragma unroll
    for (int j = 0; j < NFW; ++j) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = (nf0 + j) * 16 + 4 * g + r;
        if (co < p.Cout) {
          float v = acc[j][m][r] + (p.bias ? p.bias[co] : 0.f);
          const long long o = (long long)b * p.Cout * HW + (co * HW + oh * p.W + ow);
          if (p.resid) v += p.resid[o];
          p.y[o] = apply_act(v, p.act);
        }
      }
    }
  }
}

// weight [cout][cin][3][3] -> three bf16 images [tap][slab][fragment][lane][8]: lane l of fragment nf holds output channel
// 16 nf + (l & 15), input channels 32 slab + 8 (l >> 4) + 0..7 (element 0 in the low half of dword 0); zero outside
__global__ __launch_bounds__(256) void conv3x3_mfma_pack_kernel(const float* __restrict__ w, unsigned short* __restrict__ out,
                                                                int cout, int cin, int kslabs, int nfrags, long long total) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int e = (int)(i & 7), lane = (int)((i >> 3) & 63);
    long long rest = i >> 9;
    const int nf = (int)(rest % nfrags); rest /= nfrags;
    const int ks = (int)(rest % kslabs);
    const int tap = (int)(rest / kslabs);
    const int co = nf * 16 + (lane & 15), c = ks * KSLAB + 8 * (lane >> 4) + e;
    const float v = (co < cout && c < cin) ? w[((long long)co * cin + c) * 9 + tap] : 0.f;
    pack_store(v, out, i, total);
  }
}

}  // namespace convm
}  // namespace dlwp

using namespace dlwp;

template <int TW, int NIMG>
static void launch_nf(const convm::Params& p, int nf, int tiles, hipStream_t s) {
  const dim3 grid(tiles, p.B, (p.nfrags + nf - 1) / nf);
  if (nf == 4) hipLaunchKernelGGL((convm::conv3x3_mfma_kernel<TW, 4, NIMG>), grid, dim3(256), 0, s, p);
  else if (nf == 2) hipLaunchKernelGGL((convm::conv3x3_mfma_kernel<TW, 2, NIMG>), grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL((convm::conv3x3_mfma_kernel<TW, 1, NIMG>), grid, dim3(256), 0, s, p);
}

// the kernel instance of a shape: tile width (16 -> 8 x 16, 8 -> 16 x 8), output fragments per workgroup, tile count
static void choose_variant(int B, int H, int W, int nfrags, int& tw, int& nf_out, int& tiles_out) {
  const struct { int B, H, W, nfrags; } p{B, H, W, nfrags};
  // tile: a 16-pixel MFMA fragment is one row of 16 (8 x 16 tile) or two rows of 8 (16 x 8 tile); fragments wholly below the
  // map are skipped, so the cost of a shape is its count of live fragments -- take the smaller (8 x 8 maps: 4 against 8; 20 x 20:
  // 30 against 40), on a tie the 8 x 16 tile (longer runs of consecutive pixels per load and store; every 16 | W map)
  const long long frags16 = (long long)((p.W + 15) / 16) * p.H, frags8 = (long long)((p.W + 7) / 8) * ((p.H + 1) / 2);
  const bool narrow = frags8 < frags16;
  const int tiles = narrow ? ((p.W + 7) / 8) * ((p.H + 15) / 16) : ((p.W + 15) / 16) * ((p.H + 7) / 8);
  // output fragments per workgroup: 4 (64 channels: every staged halo tile feeds the most MFMAs) while the layer still makes
  // >= 512 workgroups (2 per CU); fewer channels per workgroup, i.e. more workgroups, on the small maps
  int nf = 4;
  while (nf > 1 && (nf / 2 >= p.nfrags || (long long)tiles * p.B * ((p.nfrags + nf - 1) / nf) < 512)) nf /= 2;
  tw = narrow ? 8 : 16; nf_out = nf; tiles_out = tiles;
}

static void launch_conv3x3_mfma(const convm::Params& p, int form, hipStream_t s) {
  int tw, nf, tiles;
  choose_variant(p.B, p.H, p.W, p.nfrags, tw, nf, tiles);
  const bool narrow = tw == 8;
  if (form == 0) narrow ? launch_nf<8, 3>(p, nf, tiles, s) : launch_nf<16, 3>(p, nf, tiles, s);
  else narrow ? launch_nf<8, 1>(p, nf, tiles, s) : launch_nf<16, 1>(p, nf, tiles, s);
}

extern "C" int32_t dlwp_conv3x3_mfma_variant(int32_t batch, int32_t H, int32_t W, int32_t cout) {
  if (batch <= 0 || H <= 0 || W <= 0 || cout <= 0) return 0;
  int tw, nf, tiles;
  choose_variant(batch, H, W, (cout + 15) / 16, tw, nf, tiles);
  return tw * 16 + nf;
}

extern "C" size_t dlwp_conv3x3_mfma_packed_bytes(int32_t cout, int32_t cin) {
  if (cout <= 0 || cin <= 0) return 0;
  const long long kslabs = (cin + convm::KSLAB - 1) / convm::KSLAB, nfrags = (cout + 15) / 16;
  const long long bytes = 3ll * 9 * kslabs * nfrags * 1024;
  return bytes < (1ll << 31) ? (size_t)bytes : 0;
}

extern "C" int32_t dlwp_conv3x3_mfma_pack_f32(const float* weight_dev, int32_t cout, int32_t cin, void* packed_dev,
                                              void* stream) {
  DLWP_REQUIRE(weight_dev && packed_dev, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  const size_t bytes = dlwp_conv3x3_mfma_packed_bytes(cout, cin);
  DLWP_REQUIRE(bytes > 0, DLWP_ERR_UNSUPPORTED, "conv3x3_mfma: unsupported shape cout=%d cin=%d", cout, cin);
  const int kslabs = (cin + convm::KSLAB - 1) / convm::KSLAB, nfrags = (cout + 15) / 16;
  const long long total = (long long)(bytes / 6);               // bf16 elements per image
  long long blocks = (total + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(convm::conv3x3_mfma_pack_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), weight_dev, reinterpret_cast<unsigned short*>(packed_dev), cout,
                     cin, kslabs, nfrags, total);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" int32_t dlwp_conv3x3_mfma_f32(const float* x0, int32_t c0, const float* x1, int32_t c1, const void* packed,
                                         const float* bias, const float* resid, float* y, int32_t batch, int32_t H, int32_t W,
                                         int32_t cout, int32_t pre_act, int32_t act, const int32_t* ring_table, int32_t form,
                                         void* stream) {
  DLWP_REQUIRE(x0 && packed && y, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(batch > 0 && H > 0 && W > 0 && c0 > 0 && cout > 0 && c1 >= 0, DLWP_ERR_INVALID_ARGUMENT, "bad shape");
  DLWP_REQUIRE(c1 == 0 || x1, DLWP_ERR_INVALID_ARGUMENT, "second segment pointer missing");
  DLWP_REQUIRE(act >= 0 && act <= 4 && pre_act >= 0 && pre_act <= 4, DLWP_ERR_INVALID_ARGUMENT, "unknown activation");
  DLWP_REQUIRE(form == 0 || form == 1, DLWP_ERR_INVALID_ARGUMENT, "unknown form %d (0 bf16x6, 1 bf16)", form);
  DLWP_REQUIRE(batch <= 65535, DLWP_ERR_UNSUPPORTED, "batch %d exceeds the grid's y dimension", batch);
  if (ring_table) {
    DLWP_REQUIRE(batch % 12 == 0, DLWP_ERR_INVALID_ARGUMENT, "n_faces=%d is not a multiple of 12", batch);
    DLWP_REQUIRE((long long)12 * H * W < (1ll << 31), DLWP_ERR_INVALID_ARGUMENT, "face too large for the 32-bit table");
  } else {
    DLWP_REQUIRE(W > 1, DLWP_ERR_INVALID_ARGUMENT, "bad shape");
  }
  // offsets inside one sample (channel plane + pixel) are 32-bit in the kernel; the halo table index and the tile count too
  const long long HW = (long long)H * W;
  const long long cmax = c0 > c1 ? (c0 > cout ? c0 : cout) : (c1 > cout ? c1 : cout);
  DLWP_REQUIRE((long long)c0 + c1 < (1ll << 31) - 64, DLWP_ERR_UNSUPPORTED, "conv3x3_mfma: too many input channels");
  DLWP_REQUIRE(cmax * HW < (1ll << 31) && ((long long)H + 17) * ((long long)W + 17) < (1ll << 31), DLWP_ERR_UNSUPPORTED,
               "conv3x3_mfma: %lld channels of %d x %d exceed the kernel's 32-bit offsets", cmax, H, W);
  DLWP_REQUIRE(dlwp_conv3x3_mfma_packed_bytes(cout, c0 + c1) > 0, DLWP_ERR_UNSUPPORTED,
               "conv3x3_mfma: unsupported shape cout=%d cin=%d", cout, c0 + c1);
  convm::Params p;
  p.x0 = x0; p.c0 = c0; p.x1 = x1; p.c1 = c1; p.wp = reinterpret_cast<const u32x4*>(packed); p.bias = bias; p.resid = resid;
  p.y = y; p.B = batch; p.H = H; p.W = W; p.Cout = cout; p.act = act; p.pre_act = pre_act;
  p.hpx = reinterpret_cast<const int2*>(ring_table);
  p.kslabs = (c0 + c1 + convm::KSLAB - 1) / convm::KSLAB; p.nfrags = (cout + 15) / 16;
  launch_conv3x3_mfma(p, form, reinterpret_cast<hipStream_t>(stream));
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}
