// Weight and bias gradient of pad(1) + Conv2d(3x3) on cat([x0, x1], 1) for the U-Net / ConvLSTM backbones (gfx950).
//
// Replaces, per layer and backward, the composition torch.cat + pre-activation + padding copy +
// torch.nn.grad.conv2d_weight + gz.sum (reference backward: scripts/train.py:271 through models/unet/unet.py:456-470,
// :512-525, :886, models/convlstm/convlstm.py:94, :148-157, utils/healpix.py:69-114):
//
//   dW[co][ci][ky][kx] = sum_{b,y,x} dz[b][co][y][x] * P(act_pre(xcat))[b][ci][y+ky][x+kx]
//   db[co]             = sum_{b,y,x} dz[b][co][y][x]
//
// with P the forward's padding rule, read through the forward's own load (conv3x3_load.hpp): no concatenated, activated or
// padded copy exists.  As a GEMM: M = Cout, N = Cin * 9, K = B * H * W, on the exact-fp32 matrix instruction
// v_mfma_f32_32x32x2_f32 (an fmaf chain per element, bitwise).
//
// A workgroup (4 waves) owns a 64 x 64 (cout x cin) block of dW and one K-slice: a run of consecutive 8 x 8 pixel tiles in
// (sample, tile row, tile column) order.  Per tile it stages the 10 x 10 input halo and the 8 x 8 dz tile in LDS, pixel-major
// with the channel fastest (stride 65: staging writes consecutive pixels, operand reads consecutive channels).  While staging
// a wave owns every fourth channel and its lanes the positions: the padding rule is resolved once per position and the loads
// of 16 channels are in flight together (one load at a time, each waiting on memory, was 4 x slower).  Each wave owns
// a 32 x 32 quarter: per pair of pixels it reads the dz operand once and issues nine MFMAs into nine accumulators (one per
// tap), each reading the input operand at the tap's halo offset.  Pixels outside the map carry dz = 0; channels outside the
// layer are zero-filled, and a wave whose quarter lies wholly outside skips its MFMAs.  The bias gradient is summed from the
// staged dz tile by the workgroups of the first cin block.  Partial dW / db of every slice go to the workspace; a second
// kernel (wgrad_reduce.hpp) adds the slices in index order.  One writer per element, no atomics, and the slice count depends
// on the shape arguments only: reruns are bit-identical.
#include "act_common.hpp"
#include "conv3x3_load.hpp"
#include "wgrad_reduce.hpp"

namespace dlwp {
namespace wgrad {

constexpr int CT = 64;            // channels per workgroup on both axes (2 x 2 waves of 32 x 32)
constexpr int LDP = CT + 1;       // LDS floats per pixel
constexpr int TH = 8, TW = 8;     // output pixels per tile
constexpr int PIX = TH * TW, HALO = (TH + 2) * (TW + 2);
constexpr int NT = 256;
constexpr int MAX_CH = 1024;      // envelope: c0 + c1 and cout
constexpr int TARGET_WGS = 512;   // workgroups a launch aims at (2 per CU on 256 CUs)
constexpr int MIN_SLICE_TILES = 4;   // tiles per slice from which the accumulator write-out stops mattering

struct Params {
  const float* x0; int c0;   // first input segment [B][c0][H][W]
  const float* x1; int c1;   // second segment or null
  const float* dz;           // [B][Cout][H][W]
  float* part_w;             // [slices][Cout][c0+c1][9]
  float* part_b;             // [slices][Cout] or null
  int B, H, W, Cout, pre_act;
  const int2* hpx;           // ring table of conv::Params, null = cylinder
  int tiles_w, tiles_hw;     // tiles per row, per sample
  int tiles, tiles_per_slice;
};

// K-slices of a shape: the pixel tiles split into runs of one length (the last may be shorter), so that the (cout, cin) blocks
// times the slices reach TARGET_WGS workgroups while a slice keeps at least MIN_SLICE_TILES tiles.  A function of the shape
// alone.  Returns 0 for a shape outside the envelope.
struct Plan { int tiles_w, tiles_hw, tiles, tiles_per_slice, slices, co_blocks, ci_blocks; };

static bool make_plan(int B, int H, int W, int cin, int cout, Plan& pl) {
  if (B <= 0 || H <= 0 || W <= 0 || cin <= 0 || cout <= 0 || cin > MAX_CH || cout > MAX_CH) return false;
  const long long HW = (long long)H * W;
  if (HW * cin >= (1ll << 31) || HW * cout >= (1ll << 31)) return false;           // per-sample offsets within 32 bits
  const long long th = (H + TH - 1) / TH, tw = (W + TW - 1) / TW;
  const long long tiles = th * tw * B;
  if (tiles >= (1ll << 31)) return false;
  pl.tiles_w = (int)tw; pl.tiles_hw = (int)(th * tw); pl.tiles = (int)tiles;
  pl.co_blocks = (cout + CT - 1) / CT; pl.ci_blocks = (cin + CT - 1) / CT;
  const long long blocks = (long long)pl.co_blocks * pl.ci_blocks;
  const long long want = TARGET_WGS / blocks > 0 ? TARGET_WGS / blocks : 1;    // rounded down: one more workgroup than fit is a second round
  long long tps = (tiles + want - 1) / want;
  if (tps < MIN_SLICE_TILES) tps = MIN_SLICE_TILES;
  pl.tiles_per_slice = (int)tps;
  pl.slices = (int)((tiles + tps - 1) / tps);
  return true;
}

__global__ __launch_bounds__(NT) void wgrad_kernel(const Params p) {
  __shared__ float s_in[HALO * LDP];
  __shared__ float s_dz[PIX * LDP];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l31 = lane & 31;
  const int cin = p.c0 + p.c1;
  const int slice = blockIdx.x, ci0 = blockIdx.y * CT, co0 = blockIdx.z * CT;
  const int wco = (wave >> 1) * 32, wci = (wave & 1) * 32;
  const bool active = co0 + wco < p.Cout && ci0 + wci < cin;        // wave-uniform
  const bool bias_owner = p.part_b && blockIdx.y == 0 && tid < CT;   // thread tid sums channel co0 + tid
  const long long HW = (long long)p.H * p.W;

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float bsum = 0.f;

  const int t_begin = slice * p.tiles_per_slice;
  const int t_end = min(p.tiles, t_begin + p.tiles_per_slice);
  for (int tile = t_begin; tile < t_end; ++tile) {
    const int b = tile / p.tiles_hw, rem = tile - b * p.tiles_hw;
    const int h0 = (rem / p.tiles_w) * TH, w0 = (rem % p.tiles_w) * TW;
    __syncthreads();
    // staging: a wave takes the channels wave, wave + 4, ... of the block (wave-uniform, so the channel's base address is
    // scalar work) and its lanes the positions; the loads of all 16 channels at a position are issued before the first is used
#pragma unroll
    for (int part = 0; part < 2; ++part) {
      const int hp = lane + 64 * part;                               // halo position: 100 of the 128 are real
      const bool on = hp < HALO;
      const int r = hp / (TW + 2), cc = hp - r * (TW + 2);
      conv::PadSource src = {0, 0, 0, 0, 0};
      if (on) src = conv::locate_padded(p, b, h0 + r - 1, w0 + cc - 1);
      float v[CT / 4], v2[CT / 4];
#pragma unroll
      for (int k = 0; k < CT / 4; ++k) conv::fetch_padded(p, src, ci0 + wave + 4 * k, v[k], v2[k]);
      if (on) {
#pragma unroll
        for (int k = 0; k < CT / 4; ++k) s_in[hp * LDP + wave + 4 * k] = conv::finish_padded_act(p, src, v[k], v2[k]);
      }
    }
    {
      const int oh = h0 + lane / TW, ow = w0 + lane % TW;            // this lane's pixel of the tile
      const bool inside = oh < p.H && ow < p.W;
      const long long pix = (long long)oh * p.W + ow;
      float d[CT / 4];
#pragma unroll
      for (int k = 0; k < CT / 4; ++k) {
        const int co = co0 + wave + 4 * k;
        d[k] = 0.f;
        if (co < p.Cout && inside) d[k] = p.dz[((long long)b * p.Cout + co) * HW + pix];
      }
#pragma unroll
      for (int k = 0; k < CT / 4; ++k) s_dz[lane * LDP + wave + 4 * k] = d[k];
    }
    __syncthreads();
    if (bias_owner) {
      for (int px = 0; px < PIX; ++px) bsum += s_dz[px * LDP + tid];
    }
    if (active) {
#pragma unroll 2
      for (int s = 0; s < PIX / 2; ++s) {
        const int px = 2 * s + half;                                 // this lane's pixel of the pair (the MFMA's k index)
        const float a = s_dz[px * LDP + wco + l31];                  // A[i = co][k]
        const float* bp = &s_in[((px / TW) * (TW + 2) + px % TW) * LDP + wci + l31];   // B[k][j = ci] at tap (0, 0)
#pragma unroll
        for (int t = 0; t < 9; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[((t / 3) * (TW + 2) + t % 3) * LDP], acc[t], 0, 0, 0);
      }
    }
  }

  // D register r of lane l is D[row = (r & 3) + 8 (r >> 2) + 4 (l >> 5)][col = l & 31]: row = cout, col = cin
  if (active) {
    const int ci = ci0 + wci + l31;
    float* out = p.part_w + (long long)slice * p.Cout * cin * 9;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + wco + (r & 3) + 8 * (r >> 2) + 4 * half;
      if (co < p.Cout && ci < cin) {
        float* o = out + ((long long)co * cin + ci) * 9;
#pragma unroll
        for (int t = 0; t < 9; ++t) o[t] = acc[t][r];
      }
    }
  }
  if (bias_owner && co0 + tid < p.Cout) p.part_b[(long long)slice * p.Cout + co0 + tid] = bsum;
}

static size_t workspace_bytes(const Plan& pl, int cin, int cout) {
  return (size_t)pl.slices * ((size_t)cout * cin * 9 + cout) * sizeof(float);
}

}  // namespace wgrad
}  // namespace dlwp

using namespace dlwp;

extern "C" size_t dlwp_conv3x3_wgrad_workspace_bytes(int32_t batch, int32_t H, int32_t W, int32_t cin, int32_t cout) {
  wgrad::Plan pl;
  if (!wgrad::make_plan(batch, H, W, cin, cout, pl)) return 0;
  return wgrad::workspace_bytes(pl, cin, cout);
}

extern "C" int32_t dlwp_conv3x3_wgrad_slices(int32_t batch, int32_t H, int32_t W, int32_t cin, int32_t cout) {
  wgrad::Plan pl;
  if (!wgrad::make_plan(batch, H, W, cin, cout, pl)) return 0;
  return pl.slices;
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
  DLWP_REQUIRE(wgrad::make_plan(batch, H, W, c0 + c1, cout, pl), DLWP_ERR_UNSUPPORTED,
               "shape outside the envelope (channels up to %d, per-sample offsets within 32 bits)", wgrad::MAX_CH);
  if (ring_table) {
    DLWP_REQUIRE(batch % 12 == 0, DLWP_ERR_UNSUPPORTED, "n_faces=%d is not a multiple of 12", batch);
    DLWP_REQUIRE((long long)12 * H * W < (1ll << 31), DLWP_ERR_UNSUPPORTED, "face too large for the 32-bit table");
  }
  const int cin = c0 + c1;
  const size_t need = wgrad::workspace_bytes(pl, cin, cout);
  DLWP_REQUIRE(workspace && workspace_bytes >= need, DLWP_ERR_WORKSPACE, "workspace of %zu bytes, %zu needed", workspace_bytes,
               need);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const long long n_w = (long long)cout * cin * 9;
  wgrad::Params p;
  p.x0 = x0; p.c0 = c0; p.x1 = x1; p.c1 = c1; p.dz = dz;
  p.part_w = reinterpret_cast<float*>(workspace);
  p.part_b = db ? p.part_w + (size_t)pl.slices * n_w : nullptr;
  p.B = batch; p.H = H; p.W = W; p.Cout = cout; p.pre_act = pre_act;
  p.hpx = reinterpret_cast<const int2*>(ring_table);
  p.tiles_w = pl.tiles_w; p.tiles_hw = pl.tiles_hw; p.tiles = pl.tiles; p.tiles_per_slice = pl.tiles_per_slice;
  hipLaunchKernelGGL(wgrad::wgrad_kernel, dim3(pl.slices, pl.ci_blocks, pl.co_blocks), dim3(wgrad::NT), 0, s, p);
  DLWP_HIP_CHECK(hipGetLastError());
  const long long n = n_w + (db ? cout : 0);
  hipLaunchKernelGGL(wgrad::wgrad_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p.part_w, p.part_b, dw,
                     db, n_w, db ? cout : 0, pl.slices);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}
