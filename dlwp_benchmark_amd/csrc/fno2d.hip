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
//
// Files:
//   fno_device.hpp      device-side types and inline helpers both kernel files use
//   fno_kernels.hip     the translation unit of all kernels: it includes the two kernel files (and says why they share a module)
//   fno_unfused.hpp     the kernels above, one launch per stage, and the host functions that launch them
//   fno_trunk.hpp       the fused kernel (all layers / a whole step / a whole rollout range in one launch) and its launch
//   fno_lift_table.hip  host-only fp64 builder of the one-input-channel lifting table
//   fno_plan.hpp        the plan, the workspace layout and the launch functions the two kernel files export
//   fno2d.hip (this)    plan create / destroy, workspace, forward, rollout, status and counters behind the dlwp_fno2d_* C ABI,
//                       and the dlwp_spectral_conv2d_* C ABI; no kernel is defined or launched here
#include <memory>

#include "fno_plan.hpp"

using namespace dlwp;
using namespace dlwp::fno;

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
int32_t SpectralCore::build(int H_, int W_, int M1_, int M2_, const int32_t* rows_in, const int32_t* rows_out, float fwd,
                            float inv, hipStream_t s) {
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

static int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

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
      int32_t accepted = 0;
      const int32_t trc = dlwp_fno2d_lift_table_build(d->lift_w1, d->lift_b1, d->lift_w2, d->lift_b2, p->hid_l, kLiftTabRange,
                                                      kLiftTabLog2, tab.data(), tab.size(), &p->lift_tab_err, &accepted);
      if (trc != DLWP_OK) { delete p; return trc; }
      p->lift_tab_state = accepted ? 1 : 2;
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
    const int32_t rc = fno_lift(p, xt, B, ws, s, timer);
    if (rc != DLWP_OK) return rc;
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
    rc = launch_layer(p->sc, lp, last ? LayerForm::kFnoLast : LayerForm::kFnoHidden, s, !p->k.fp32_mfma);
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
  // weights_dev is [Ci][Co][R][K][2] of the FORWARD operator in both cases
  return launch_pack_spectral(reinterpret_cast<const float2*>(weights_dev), plan->wt.as<float2>(), plan->ci, plan->co,
                              plan->sc.M1, plan->sc.M2, adjoint != 0, reinterpret_cast<hipStream_t>(stream));
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
  int32_t rc = launch_fwd_dft(sc, x, ybuf, batch, s);
  if (rc != DLWP_OK) return rc;
  rc = launch_modes(sc, ybuf, zbuf, plan->wt.as<float2>(), batch, s);
  if (rc != DLWP_OK) return rc;
  LayerParams lp;
  lp.x = x; lp.y = y; lp.wsp = nullptr; lp.wsb = nullptr; lp.bias = plan->zero_bias.as<float>(); lp.zbuf = zbuf;
  lp.t = sc.t.as<float>(); lp.tt = sc.tt.as<float>(); lp.ybuf = nullptr;
  lp.B = batch; lp.H = sc.H; lp.W = sc.W;
  lp.stagger = 0;
  return launch_layer(sc, lp, LayerForm::kSpectralConv, s);
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
