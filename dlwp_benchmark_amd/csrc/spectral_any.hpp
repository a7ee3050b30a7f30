// Width-generic spectral path (spectral_any.hip): the SpectralConv2d and FNO2d plans for every shape the 32-channel
// kernels of fno_unfused.hpp / fno_trunk.hpp do not take.  fno2d.hip keeps the C ABI and routes a plan here when its shape is outside the
// specialised domain; nothing here is reached by a plan the specialised kernels accept.
#pragma once

#include "common.hpp"

namespace dlwp {
namespace sany {

constexpr int kMaxChannels = 512;             // Ci, Co, hidden, lifting, projection, in / out channels
constexpr size_t kMaxLdsBytes = 128 * 1024;   // per-plane LDS image of the transform kernels (H x 2 n_cols)

// Geometry of one mode-truncated spectral convolution: twiddle tables and shape.
struct Geom {
  int ci = 0, co = 0, H = 0, W = 0, nr = 0, nc = 0;
  int Hp = 0, Wp = 0, KPp = 0;   // H and W rounded up to 16; 2 * n_cols rounded up to 16
  float fwd = 1.f;
  DevBuf tf;   // [Wp][KPp]  forward W-DFT: tf[w][2k] = cos(2 pi k w / W), tf[w][2k+1] = -sin (zero padded)
  DevBuf ti;   // [KPp][Wp]  the same values transposed: inverse W-DFT of the half spectrum (C2R)
  DevBuf ef;   // [nr][H] float2: e^{-2 pi i rows_in[r] h / H}
  DevBuf ei;   // [nr][H] float2: e^{+2 pi i rows_out[r] h / H}
  DevBuf ck;   // [nc]: inv_scale x (1 for the DC and Nyquist columns, 2 otherwise)
  DevBuf efo;  // [nr][H] float2: e^{-2 pi i rows_out[r] h / H}, the weight gradient's transform of grad_y; built by
               // wgrad_prepare on first use, so inference plans pay nothing
  std::vector<int32_t> rows_o;   // host copy of rows_out (what efo is built from)
  size_t fwd_lds() const { return (size_t)Hp * (KPp + 1) * sizeof(float); }
  size_t inv_lds() const { return (size_t)Hp * (KPp + 4) * sizeof(float) + (size_t)nr * nc * sizeof(float2); }
};

// Validates the generic domain (DLWP_ERR_UNSUPPORTED naming the limit) and uploads the tables.
int32_t geom_build(Geom& g, int ci, int co, int H, int W, int nr, int nc, const int32_t* rows_in,
                   const int32_t* rows_out, float fwd_scale, float inv_scale, hipStream_t s);
// weights [Ci][Co][nr_blk][nc][2] (host, PyTorch layout) -> rows [row_off, row_off + nr_blk) of the packed
// [nr * nc][Ci][Co] complex image (mode m = ky * nr + r)
void pack_host(std::vector<float>& dst, const Geom& g, const float* w, int nr_blk, int row_off);
// device weights of the forward operator [Ci_f][Co_f][nr][nc][2] -> packed image; adjoint != 0 packs the conjugate
// transpose (then the plan's ci = Co_f and co = Ci_f)
int32_t pack_dev(const Geom& g, const float* w_dev, int adjoint, float2* wt, hipStream_t s);
// bytes of workspace for `batch` samples: the kept spectrum of the input and of the output
size_t workspace_bytes(const Geom& g, int batch);
// y = S(x), x [B, ci, H, W], y [B, co, H, W]; in two halves (forward transform + mode mix, inverse transform)
int32_t run_fwd_mix(const Geom& g, const float2* wt, const float* x, int batch, void* ws, hipStream_t s);
int32_t run_inv(const Geom& g, float* y, int batch, void* ws, hipStream_t s);
// Weight gradient of y = S_W(x): grad_w [Ci][Co][nr][nc][2] (PyTorch layout, overwritten)
//   = ck[k] * sum_b conj(fwd X[b, i, rows_in[r], k]) DY[b, o, rows_out[r], k]
// wgrad_prepare uploads efo once (it synchronises `s`: call it outside a stream capture, which the first
// first weight-gradient call of a plan does); run_wgrad is fwd_kernel on x, fwd_kernel on grad_y, wgrad_kernel into the
// packed [mode][Ci][Co] image in the workspace, unpack_kernel.
int32_t wgrad_prepare(Geom& g, hipStream_t s);
size_t wgrad_workspace_bytes(const Geom& g, int batch);
int32_t run_wgrad(const Geom& g, const float* x, const float* grad_y, float* grad_w, int batch, void* ws, hipStream_t s);

// Generic FNO2d plan (fno2d.hip's dlwp_fno2d_plan owns one when the shape is outside the specialised domain).
struct Fno;
int32_t fno_create(Fno** out, const dlwp_fno2d_desc* d, hipStream_t s);
void fno_destroy(Fno* p);
size_t fno_workspace_bytes(const Fno* p, int batch);
int32_t fno_forward(const Fno* p, const float* x, float* y, int batch, void* ws, size_t ws_bytes, hipStream_t s);
// rollout steps [step_begin, step_end) (step_end < 0: to the end); class_ms / class_launches non-null: every launch
// bracketed by events (dlwp_fno2d_rollout_profiled_f32 classes), the stream synchronised at the end
int32_t fno_rollout(const Fno* p, const float* constants, int32_t n_const, const float* prescribed, int32_t n_presc,
                    const float* prognostic, int32_t n_prog, int32_t batch, int32_t n_time, int32_t context, float* out,
                    void* ws, size_t ws_bytes, hipStream_t s, int32_t step_begin, int32_t step_end, double* class_ms,
                    int32_t* class_launches);

}  // namespace sany
}  // namespace dlwp
