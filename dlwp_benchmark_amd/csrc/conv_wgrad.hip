// Weight and bias gradient of the U-Net / ConvLSTM family's convolutions (gfx950), one kernel for
//   * pad(1) + Conv2d(3x3) on cat([x0, x1], 1) under CylinderPad or HEALPixPadding      (dlwp_conv3x3_wgrad_f32),
//   * the zero-padded k x k Conv2d, stride 1 or 2, and ConvTranspose2d: the 1x1 shortcuts, first layers and heads, the 3x3
//     stride-2 downsampling, ConvTranspose2d 2x2 s2 and 4x4 s2 p1                       (dlwp_conv2d_wgrad_f32).
//
// Replaces, per layer and backward, torch.cat + the pre-activated copy + the padded copy + the library's weight gradient +
// gz.sum (reference backward: scripts/train.py:271 through models/unet/unet.py:450-470, :512-525, :583-584, :719, :879, :886,
// models/convlstm/convlstm.py:94, :148-157, utils/healpix.py:69-114).  One formula serves every layer.  With a "small" map
// S [B][CS][SH][SW] and a "large" map L [B][CL][H][W] related by stride s, padding p and a k x k kernel,
//
//   G[a][b][ky][kx] = sum_{n,i,j} S[n][a][i][j] * P(act_pre(L))[n][b][i s - p + ky][j s - p + kx]
//
// is dW of Conv2d with S = dz, L = x (G = [cout][cin][k][k]) and dW of ConvTranspose2d with S = x, L = dz (G = [cin][cout][k][k]:
// the transposed layer scatters x[i][j] to z[i s - p + ky][j s - p + kx], the same index pair with the roles exchanged).
// db[c] = sum dz[n][c][.][.] is the sum of the S map (Conv2d) or of the L map (ConvTranspose2d).  P, the padding rule, is the
// one thing the two families do not share; it is a loader policy:
//   PaddedLoad   L = cat([x0, x1], 1) behind the forward's own padding, read through conv3x3_load.hpp (k 3, s 1, p 1): no
//                concatenated, activated or padded copy exists;
//   ZeroPadLoad  one segment, zero outside the map.
//
// As a GEMM: M = CS, N = CL * k^2, K = B * SH * SW, on the exact-fp32 matrix instruction v_mfma_f32_32x32x2_f32 (an fmaf chain
// per element, bitwise).  A workgroup (4 waves) owns a 64 x 64 (S x L channel) block of G for one tap group and one K-slice, a
// run of consecutive pixel tiles of S in (sample, tile row, tile column) order.  Per tile it stages the S tile and the L halo
// the tile's taps reach in LDS, pixel-major with the channel fastest (stride 65: staging writes consecutive pixels, operand
// reads consecutive channels), both read where they lie.  While staging a wave owns every fourth channel (wave-uniform, so the
// channel's base address is scalar work) and its lanes the positions: the padding rule is resolved once per position and the
// loads of 16 channels are in flight together (one load at a time, each waiting on memory, was 4 x slower); act_pre is applied
// on the way into LDS.  Each wave owns a 32 x 32 quarter: per pair of S pixels it reads the S operand once and issues one MFMA
// per tap into one accumulator per tap, the L operand read at halo offset (i s + ky, j s + kx).  Pixels outside the map carry
// S = 0, channels outside the layer are zero-filled, and a wave whose quarter lies wholly outside skips its MFMAs.
//
// Tile and tap split (compile-time per (k, s), Geo below):
//   * stride 1: 8 x 8 S pixels; stride 2: 4 x 8, whose L halo at k = 4 is 10 x 18 positions = 46.8 KB beside the 8.3 KB S
//     tile: two workgroups per CU fit the 160 KB (an 8 x 8 tile's 18 x 18 halo is 84 KB: one workgroup).
//   * k <= 3: all k^2 taps in one workgroup (9 accumulators of 16 registers).  k = 4: sixteen accumulators are the whole
//     256-register accumulator file, so the taps split into two groups of two kernel rows (8 accumulators); N = CL * k^2 makes
//     the group one more block index (blockIdx.y = L block * groups + group).  Both groups stage the whole halo: two rows of
//     ten more than they read, for one staging routine and one bias rule.
//
// Bias: summed from the staged dz by thread c < 64 of the workgroups that see every dz value once: the S tile in the first L
// block (Conv2d); for ConvTranspose2d the L positions a tile owns -- the s TH x s TW positions from its halo's corner, which
// tile the map without overlap, and for the last tile row / column the rest of the halo (k > s + p leaves rows beyond) -- in
// the first S block.  The halo is max(k, s) wide per step so that it always holds the owned positions (k = 1, s = 2).
//
// Partial G / db of every slice go to the workspace; a second kernel (wgrad_reduce.hpp) adds the slices in index order.  One
// writer per element, no atomics, and a slice count that depends on the shape arguments only: reruns are bit-identical.
//
// The staging loops stand in the kernel body, which indexes the __shared__ arrays itself, and only the per-position and
// per-channel reads go through the loader.  Staging in a function that receives the LDS arrays as float* (member or free)
// compiles the 3x3 padded instance to 432 VGPRs with 1152 v_mov_b64 copies of the accumulators, against 212.
#include "act_common.hpp"
#include "conv3x3_load.hpp"
#include "wgrad_reduce.hpp"

namespace dlwp {
namespace wgrad {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int CT = 64;            // channels per workgroup on both axes (2 x 2 waves of 32 x 32)
constexpr int LDP = CT + 1;       // LDS floats per pixel
constexpr int NT = 256;
constexpr int MAX_CH = 1024;      // envelope: both channel counts (the 3x3 layer's: c0 + c1)
constexpr int MAX_K = 4;
constexpr int TARGET_WGS = 512;   // workgroups a launch aims at (2 per CU on 256 CUs)
constexpr int MIN_SLICE_PIX = 256;   // S pixels per slice from which the accumulator write-out stops mattering: 4 tiles of 8 x 8

constexpr int tile_h(int stride) { return stride == 1 ? 8 : 4; }
constexpr int tile_w(int) { return 8; }
constexpr int tap_groups(int k) { return k == 4 ? 2 : 1; }

template <int K, int STR>
struct Geo {
  static constexpr int TH = tile_h(STR), TW = tile_w(STR), PIX = TH * TW;
  static constexpr int GROUPS = tap_groups(K), ROWS = K / GROUPS, TAPS = ROWS * K;   // kernel rows and taps per group
  static constexpr int EXT = K > STR ? K : STR;
  static constexpr int HR = (TH - 1) * STR + EXT, HC = (TW - 1) * STR + EXT, HALO = HR * HC;
  static constexpr int SUB = 64 / PIX;       // lanes per S pixel while staging (stride 2: the two take alternate channels)
};

// The small map is S [B][CS][SH][SW].  The large map [B][c0 + c1][H][W] goes by the field names of conv3x3_load.hpp's Src (x0,
// c0, x1, c1, H, W, pre_act, hpx), so that its three steps take this block.  The order is the k x k kernel's, what only
// PaddedLoad reads last: with the 3x3 kernel's order the arguments load in other pieces and the transposed layers measured
// 1-2 % slower.
struct Params {
  const float* S;
  const float* x0;                  // first segment (ZeroPadLoad: the whole map)
  float* part_w;                    // [slices][CS][CL][k][k] or null
  float* part_b;                    // [slices][CB] or null
  int CS, SH, SW, c0, H, W, pad, pre_act;   // pad: ZeroPadLoad's (PaddedLoad pads 1)
  int bias_from_l, CB;              // dz is the L map (ConvTranspose2d); its channels
  int tiles_w, tiles_hw;            // tiles per row, per sample
  int tiles, tiles_per_slice;
  const float* x1; int c1;          // PaddedLoad alone: second segment or null
  const int2* hpx;                  // ... ring table, null = cylinder
};

// The loaders: which cells a halo position reads (locate, once per position), the raw values of one channel there (fetch: 0
// where there is none or the channel is past the layer) and the value that goes into LDS (finish); and what the kernel asks
// about the large map: its padding, its channel count, whether it is dz.
struct PaddedLoad {
  using Where = conv::PadSource;
  static __device__ __forceinline__ Where nowhere() { return {0, 0, 0, 0, 0}; }
  static __device__ __forceinline__ int pad(const Params&) { return 1; }
  static __device__ __forceinline__ int channels(const Params& p) { return p.c0 + p.c1; }
  static __device__ __forceinline__ bool bias_from_l(const Params&) { return false; }
  static __device__ __forceinline__ Where locate(const Params& p, int b, int y, int x) { return conv::locate_padded(p, b, y, x); }
  static __device__ __forceinline__ void fetch(const Params& p, const Where& at, int c, float& v, float& v2) {
    conv::fetch_padded(p, at, c, v, v2);
  }
  static __device__ __forceinline__ float finish(const Params& p, const Where& at, int, float v, float v2) {
    return conv::finish_padded_act(p, at, v, v2);
  }
};

struct ZeroPadLoad {
  struct Where { bool inside; int b, pos; };
  static __device__ __forceinline__ Where nowhere() { return {false, 0, 0}; }
  static __device__ __forceinline__ int pad(const Params& p) { return p.pad; }
  static __device__ __forceinline__ int channels(const Params& p) { return p.c0; }
  static __device__ __forceinline__ bool bias_from_l(const Params& p) { return p.bias_from_l; }
  static __device__ __forceinline__ Where locate(const Params& p, int b, int y, int x) {
    const bool inside = y >= 0 && y < p.H && x >= 0 && x < p.W;
    return {inside, b, inside ? y * p.W + x : 0};
  }
  static __device__ __forceinline__ void fetch(const Params& p, const Where& at, int c, float& v, float&) {
    const long long HW = (long long)p.H * p.W;
    v = 0.f;
    if (at.inside && c < p.c0) v = (p.x0 + (long long)at.b * p.c0 * HW)[c * HW + at.pos];   // scalar bases, 32-bit lane part
  }
  static __device__ __forceinline__ float finish(const Params& p, const Where& at, int c, float v, float) {
    return at.inside && c < p.c0 ? actc::apply_act(v, p.pre_act) : 0.f;
  }
};

template <int K, int STR, class Load>
__global__ __launch_bounds__(NT) void wgrad_kernel(const Params p) {
  using G = Geo<K, STR>;
  __shared__ float s_l[G::HALO * LDP];
  __shared__ float s_s[G::PIX * LDP];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l31 = lane & 31;
  const int CL = Load::channels(p);
  const int slice = blockIdx.x, cs0 = blockIdx.z * CT;
  const int group = blockIdx.y % G::GROUPS, cl0 = (blockIdx.y / G::GROUPS) * CT, ky0 = group * G::ROWS;
  const int wcs = (wave >> 1) * 32, wcl = (wave & 1) * 32;
  const bool active = p.part_w && cs0 + wcs < p.CS && cl0 + wcl < CL;        // wave-uniform
  // thread tid sums channel cb0 + tid of dz in the workgroups that see every value of it once (tap group 0 of one block row)
  const bool from_l = Load::bias_from_l(p);
  const bool bias_owner = p.part_b && tid < CT && (from_l ? blockIdx.z == 0 && group == 0 : blockIdx.y == 0);
  const int cb0 = from_l ? cl0 : cs0;
  const long long SHW = (long long)p.SH * p.SW;

  f32x16 acc[G::TAPS];
#pragma unroll
  for (int t = 0; t < G::TAPS; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float bsum = 0.f;

  const int t_begin = slice * p.tiles_per_slice;
  const int t_end = min(p.tiles, t_begin + p.tiles_per_slice);
  for (int tile = t_begin; tile < t_end; ++tile) {
    const int b = tile / p.tiles_hw, rem = tile - b * p.tiles_hw;
    const int i0 = (rem / p.tiles_w) * G::TH, j0 = (rem % p.tiles_w) * G::TW;
    __syncthreads();
    // staging: a wave takes the channels wave, wave + 4, ... of the block and its lanes the positions; the loads of all 16
    // channels at a position are issued before the first is used
    {
      const int y0 = i0 * STR - Load::pad(p), x0 = j0 * STR - Load::pad(p);
#pragma unroll
      for (int part = 0; part < (G::HALO + 63) / 64; ++part) {
        const int hp = lane + 64 * part;                               // halo position
        const bool on = hp < G::HALO;
        const int r = hp / G::HC;
        typename Load::Where at = Load::nowhere();
        if (on) at = Load::locate(p, b, y0 + r, x0 + hp - r * G::HC);
        float v[CT / 4], v2[CT / 4];
#pragma unroll
        for (int k = 0; k < CT / 4; ++k) Load::fetch(p, at, cl0 + wave + 4 * k, v[k], v2[k]);
        if (on) {
#pragma unroll
          for (int k = 0; k < CT / 4; ++k) s_l[hp * LDP + wave + 4 * k] = Load::finish(p, at, cl0 + wave + 4 * k, v[k], v2[k]);
        }
      }
    }
    {
      const float* sb = p.S + (long long)b * p.CS * SHW;
      const int px = lane % G::PIX, sub = lane / G::PIX;               // this lane's pixel of the tile
      const int i = i0 + px / G::TW, j = j0 + px % G::TW;
      const bool inside = i < p.SH && j < p.SW;
      const int pos = inside ? i * p.SW + j : 0;
      float d[CT / 4 / G::SUB];
#pragma unroll
      for (int k = 0; k < CT / 4 / G::SUB; ++k) {
        const int c = cs0 + wave + 4 * (k * G::SUB + sub);
        d[k] = 0.f;
        if (inside && c < p.CS) d[k] = sb[c * SHW + pos];
      }
#pragma unroll
      for (int k = 0; k < CT / 4 / G::SUB; ++k) s_s[px * LDP + wave + 4 * (k * G::SUB + sub)] = d[k];
    }
    __syncthreads();
    if (bias_owner) {
      if (!from_l) {
        for (int px = 0; px < G::PIX; ++px) bsum += s_s[px * LDP + tid];
      } else {
        const int rows = i0 + G::TH >= p.SH ? G::HR : G::TH * STR;     // the last tile row / column owns the rest of the halo
        const int cols = j0 + G::TW >= p.SW ? G::HC : G::TW * STR;
        for (int r = 0; r < rows; ++r)
          for (int c = 0; c < cols; ++c) bsum += s_l[(r * G::HC + c) * LDP + tid];
      }
    }
    if (active) {
#pragma unroll 2
      for (int s = 0; s < G::PIX / 2; ++s) {
        const int px = 2 * s + half;                                   // this lane's pixel of the pair (the MFMA's k index)
        const float a = s_s[px * LDP + wcs + l31];                     // A[i = S channel][k]
        const float* bp = &s_l[(((px / G::TW) * STR + ky0) * G::HC + (px % G::TW) * STR) * LDP + wcl + l31];   // B[k][j = L channel], first tap
#pragma unroll
        for (int t = 0; t < G::TAPS; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[((t / K) * G::HC + t % K) * LDP], acc[t], 0, 0, 0);
      }
    }
  }

  // D register r of lane l is D[row = (r & 3) + 8 (r >> 2) + 4 (l >> 5)][col = l & 31]: row = S channel, col = L channel
  if (active) {
    const int cl = cl0 + wcl + l31;
    float* out = p.part_w + (long long)slice * p.CS * CL * (K * K) + ky0 * K;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int cs = cs0 + wcs + (r & 3) + 8 * (r >> 2) + 4 * half;
      if (cs < p.CS && cl < CL) {
        float* o = out + ((long long)cs * CL + cl) * (K * K);
#pragma unroll
        for (int t = 0; t < G::TAPS; ++t) o[t] = acc[t][r];
      }
    }
  }
  if (bias_owner && cb0 + tid < p.CB) p.part_b[(long long)slice * p.CB + cb0 + tid] = bsum;
}

// K-slices of a shape: the S tiles split into runs of one length (the last may be shorter), so that the blocks times the slices
// reach TARGET_WGS workgroups while a slice keeps at least MIN_SLICE_PIX pixels.  A function of the shape alone.  False for a
// shape outside the envelope.  The 3x3 padded layer is k = 3, stride = 1, pad = 1, not transposed.
struct Plan {
  int k, stride, transposed, cin, cout;
  int CS, SH, SW, CL, LH, LW;
  int tiles_w, tiles_hw, tiles, tiles_per_slice, slices, cs_blocks, cl_blocks, groups;
};

static bool make_plan(int B, int cin, int H, int W, int cout, int k, int stride, int pad, bool transposed, Plan& pl) {
  if (B <= 0 || H <= 0 || W <= 0 || cin <= 0 || cout <= 0 || cin > MAX_CH || cout > MAX_CH) return false;
  if (k < 1 || k > MAX_K || stride < 1 || stride > 2 || pad < 0 || pad >= k) return false;
  long long OH, OW;
  if (transposed) {
    OH = ((long long)H - 1) * stride - 2 * pad + k;
    OW = ((long long)W - 1) * stride - 2 * pad + k;
  } else {
    OH = ((long long)H + 2 * pad - k) / stride + 1;
    OW = ((long long)W + 2 * pad - k) / stride + 1;
    if ((long long)H + 2 * pad < k || (long long)W + 2 * pad < k) return false;
  }
  if (OH < 1 || OW < 1) return false;
  if ((long long)H * W * cin >= (1ll << 31) || OH * OW * cout >= (1ll << 31)) return false;   // per-sample offsets within 32 bits
  pl.k = k; pl.stride = stride; pl.transposed = transposed; pl.cin = cin; pl.cout = cout;
  if (transposed) { pl.CS = cin; pl.SH = H; pl.SW = W; pl.CL = cout; pl.LH = (int)OH; pl.LW = (int)OW; }
  else            { pl.CS = cout; pl.SH = (int)OH; pl.SW = (int)OW; pl.CL = cin; pl.LH = H; pl.LW = W; }
  const int TH = tile_h(stride), TW = tile_w(stride);
  const long long th = (pl.SH + TH - 1) / TH, tw = (pl.SW + TW - 1) / TW;
  const long long tiles = th * tw * B;
  if (tiles >= (1ll << 31)) return false;
  pl.tiles_w = (int)tw; pl.tiles_hw = (int)(th * tw); pl.tiles = (int)tiles;
  pl.cs_blocks = (pl.CS + CT - 1) / CT; pl.cl_blocks = (pl.CL + CT - 1) / CT; pl.groups = tap_groups(k);
  const long long blocks = (long long)pl.cs_blocks * pl.cl_blocks * pl.groups;
  const long long want = TARGET_WGS / blocks > 0 ? TARGET_WGS / blocks : 1;    // rounded down: one more workgroup than fit is a second round
  const long long min_tiles = MIN_SLICE_PIX / (TH * TW);
  long long tps = (tiles + want - 1) / want;
  if (tps < min_tiles) tps = min_tiles;
  pl.tiles_per_slice = (int)tps;
  pl.slices = (int)((tiles + tps - 1) / tps);
  return true;
}

static long long weight_count(const Plan& pl) { return (long long)pl.cout * pl.cin * pl.k * pl.k; }

static size_t workspace_bytes(const Plan& pl) { return (size_t)pl.slices * ((size_t)weight_count(pl) + pl.cout) * sizeof(float); }

// The two launches.  `p` arrives with its two maps described; the small map's shape, the workspace split and the tiles come
// from the plan.  Without dW only the workgroups that sum the bias run: the first L block (Conv2d), the first S block
// (ConvTranspose2d).
static int32_t launch(const Plan& pl, Params p, bool padded, float* workspace, float* dw, float* db, hipStream_t s) {
  const long long n_w = weight_count(pl);
  p.CS = pl.CS; p.SH = pl.SH; p.SW = pl.SW;
  p.part_w = dw ? workspace : nullptr;
  p.part_b = db ? workspace + (size_t)pl.slices * n_w : nullptr;
  p.bias_from_l = pl.transposed; p.CB = pl.cout;
  p.tiles_w = pl.tiles_w; p.tiles_hw = pl.tiles_hw; p.tiles = pl.tiles; p.tiles_per_slice = pl.tiles_per_slice;
  dim3 grid(pl.slices, pl.cl_blocks * pl.groups, pl.cs_blocks);
  if (!dw && pl.transposed) grid.z = 1;
  if (!dw && !pl.transposed) grid.y = 1;
  switch (padded ? 0 : pl.k * 10 + pl.stride) {
#define DLWP_CASE(KEY, K, S, LOAD) case KEY: hipLaunchKernelGGL((wgrad_kernel<K, S, LOAD>), grid, dim3(NT), 0, s, p); break;
    DLWP_CASE(0, 3, 1, PaddedLoad)
    DLWP_CASE(11, 1, 1, ZeroPadLoad) DLWP_CASE(12, 1, 2, ZeroPadLoad) DLWP_CASE(21, 2, 1, ZeroPadLoad)
    DLWP_CASE(22, 2, 2, ZeroPadLoad) DLWP_CASE(31, 3, 1, ZeroPadLoad) DLWP_CASE(32, 3, 2, ZeroPadLoad)
    DLWP_CASE(41, 4, 1, ZeroPadLoad) DLWP_CASE(42, 4, 2, ZeroPadLoad)
#undef DLWP_CASE
    default: DLWP_REQUIRE(false, DLWP_ERR_UNSUPPORTED, "no kernel for k=%d stride=%d", pl.k, pl.stride);
  }
  DLWP_HIP_CHECK(hipGetLastError());
  const long long n = (dw ? n_w : 0) + (db ? pl.cout : 0);
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p.part_w, p.part_b, dw, db,
                     dw ? n_w : 0, db ? pl.cout : 0, pl.slices);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

}  // namespace wgrad
}  // namespace dlwp

using namespace dlwp;

extern "C" size_t dlwp_conv2d_wgrad_workspace_bytes(int32_t batch, int32_t cin, int32_t H, int32_t W, int32_t cout, int32_t k,
                                                    int32_t stride, int32_t pad, int32_t transposed) {
  wgrad::Plan pl;
  return wgrad::make_plan(batch, cin, H, W, cout, k, stride, pad, transposed != 0, pl) ? wgrad::workspace_bytes(pl) : 0;
}

extern "C" int32_t dlwp_conv2d_wgrad_slices(int32_t batch, int32_t cin, int32_t H, int32_t W, int32_t cout, int32_t k,
                                            int32_t stride, int32_t pad, int32_t transposed) {
  wgrad::Plan pl;
  return wgrad::make_plan(batch, cin, H, W, cout, k, stride, pad, transposed != 0, pl) ? pl.slices : 0;
}

extern "C" size_t dlwp_conv3x3_wgrad_workspace_bytes(int32_t batch, int32_t H, int32_t W, int32_t cin, int32_t cout) {
  return dlwp_conv2d_wgrad_workspace_bytes(batch, cin, H, W, cout, 3, 1, 1, 0);
}

extern "C" int32_t dlwp_conv3x3_wgrad_slices(int32_t batch, int32_t H, int32_t W, int32_t cin, int32_t cout) {
  return dlwp_conv2d_wgrad_slices(batch, cin, H, W, cout, 3, 1, 1, 0);
}

extern "C" int32_t dlwp_conv3x3_wgrad_f32(const float* x0, int32_t c0, const float* x1, int32_t c1, const float* dz, float* dw,
                                          float* db, int32_t batch, int32_t H, int32_t W, int32_t cout, int32_t pre_act,
                                          const int32_t* ring_table, void* workspace, size_t workspace_bytes, void* stream) {
  DLWP_REQUIRE(x0 && dz && dw, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(batch > 0 && H > 0 && W > 0 && c0 > 0 && cout > 0 && c1 >= 0, DLWP_ERR_INVALID_ARGUMENT, "bad shape");
  DLWP_REQUIRE(c1 == 0 || x1, DLWP_ERR_INVALID_ARGUMENT, "second segment pointer missing");
  DLWP_REQUIRE(pre_act >= 0 && pre_act <= 4, DLWP_ERR_INVALID_ARGUMENT, "unknown activation %d", pre_act);
  DLWP_REQUIRE(c1 <= wgrad::MAX_CH && c0 <= wgrad::MAX_CH, DLWP_ERR_UNSUPPORTED, "more than %d input channels", wgrad::MAX_CH);
  wgrad::Plan pl;
  DLWP_REQUIRE(wgrad::make_plan(batch, c0 + c1, H, W, cout, 3, 1, 1, false, pl), DLWP_ERR_UNSUPPORTED,
               "shape outside the envelope (channels up to %d, per-sample offsets within 32 bits)", wgrad::MAX_CH);
  if (ring_table) {
    DLWP_REQUIRE(batch % 12 == 0, DLWP_ERR_UNSUPPORTED, "n_faces=%d is not a multiple of 12", batch);
    DLWP_REQUIRE((long long)12 * H * W < (1ll << 31), DLWP_ERR_UNSUPPORTED, "face too large for the 32-bit table");
  }
  const size_t need = wgrad::workspace_bytes(pl);
  DLWP_REQUIRE(workspace && workspace_bytes >= need, DLWP_ERR_WORKSPACE, "workspace of %zu bytes, %zu needed", workspace_bytes,
               need);
  wgrad::Params p = {};
  p.S = dz;
  p.x0 = x0; p.c0 = c0; p.x1 = x1; p.c1 = c1; p.H = H; p.W = W; p.pre_act = pre_act;
  p.hpx = reinterpret_cast<const int2*>(ring_table); p.pad = 1;
  return wgrad::launch(pl, p, true, reinterpret_cast<float*>(workspace), dw, db, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int32_t dlwp_conv2d_wgrad_f32(const float* x, const float* dz, float* dw, float* db, int32_t batch, int32_t cin,
                                         int32_t H, int32_t W, int32_t cout, int32_t k, int32_t stride, int32_t pad,
                                         int32_t pre_act, int32_t transposed, void* workspace, size_t workspace_bytes,
                                         void* stream) {
  DLWP_REQUIRE(x && dz, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(batch > 0 && H > 0 && W > 0 && cin > 0 && cout > 0 && k > 0 && stride > 0 && pad >= 0, DLWP_ERR_INVALID_ARGUMENT,
               "bad shape");
  DLWP_REQUIRE(pre_act >= 0 && pre_act <= 4, DLWP_ERR_INVALID_ARGUMENT, "unknown activation %d", pre_act);
  DLWP_REQUIRE(!transposed || pre_act == 0, DLWP_ERR_INVALID_ARGUMENT, "the transposed layer has no pre-activation");
  wgrad::Plan pl;
  DLWP_REQUIRE(wgrad::make_plan(batch, cin, H, W, cout, k, stride, pad, transposed != 0, pl), DLWP_ERR_UNSUPPORTED,
               "shape outside the envelope (k up to %d, stride 1 or 2, padding < k, channels up to %d, per-sample offsets "
               "within 32 bits)", wgrad::MAX_K, wgrad::MAX_CH);
  if (!dw && !db) return DLWP_OK;
  const size_t need = wgrad::workspace_bytes(pl);
  DLWP_REQUIRE(workspace && workspace_bytes >= need, DLWP_ERR_WORKSPACE, "workspace of %zu bytes, %zu needed", workspace_bytes,
               need);
  wgrad::Params p = {};
  p.S = transposed ? x : dz;
  p.x0 = transposed ? dz : x; p.c0 = pl.CL; p.H = pl.LH; p.W = pl.LW; p.pre_act = pre_act; p.pad = pad;
  return wgrad::launch(pl, p, false, reinterpret_cast<float*>(workspace), dw, db, reinterpret_cast<hipStream_t>(stream));
}
