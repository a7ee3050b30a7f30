/*
 * dlwp_hip.h -- C ABI of libdlwp_hip.so, the MI355X (gfx950) kernel library behind the
 * dlwpbench backbone rollout hot path.
 *
 * The reference (AnneLouisedb/dlwp-benchmark) is pure Python/PyTorch and has no FFI of its own;
 * every entry point below replaces a stretch of ATen calls inside a reference nn.Module.forward
 * (cited per function as file:line under src/dlwpbench/).  INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - plain C: raw device pointers, explicit sizes, no torch / C++ types.
 *   - every function returns 0 on success, a negative dlwp_status otherwise; the message for the
 *     calling thread is available from dlwp_last_error().  No C++ exception crosses the ABI.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  All work is
 *     enqueued asynchronously on it; nothing synchronises the device.
 *   - the caller owns every input / output / workspace buffer; the library owns plan handles.
 *     Plans are immutable after creation and may be shared between threads.
 *   - "dev" pointers are device memory, "host" pointers are host memory.
 */
#ifndef DLWP_HIP_H
#define DLWP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum dlwp_status {
  DLWP_OK = 0,
  DLWP_ERR_INVALID_ARGUMENT = -1,
  DLWP_ERR_UNSUPPORTED = -2,
  DLWP_ERR_HIP = -3,
  DLWP_ERR_WORKSPACE = -4,
  DLWP_ERR_TIMEOUT = -5,     /* a fused kernel's inter-workgroup hand-off exceeded its spin bound (output poisoned) */
  DLWP_ERR_RANGE = -6        /* dlwp_fno2d_status only: an unchecked f16x3 launch produced a non-finite output */
} dlwp_status;

/* library version, major*10000 + minor*100 + patch */
int32_t dlwp_version(void);
/* message of the last failing call on this thread ("" if none) */
const char* dlwp_last_error(void);
/* number of visible HIP devices (<0 on error); does not create a context */
int32_t dlwp_device_count(void);

/* ------------------------------------------------------------------------------------------
 * FNO2d rollout  (reference models/fno/fno.py:12-106 `FNO2DModule`; the arithmetic it delegates
 * to neuralop.models.FNO -- fno.py:38-47 -- is restated in DESIGN.md / oracle/restate/fno.py)
 * ------------------------------------------------------------------------------------------ */
typedef struct dlwp_fno2d_plan dlwp_fno2d_plan;

/* Two kernel sets behind one plan type, chosen at creation from the shape alone:
 *   specialised (csrc/fno_kernels.hip): hidden == 32, lifting and projection multiples of 16, in_channels <= 32,
 *     out_channels <= 16, n_cols <= 16 -- fused persistent kernels, the execution-form fields below apply;
 *   width-generic (csrc/spectral_any.hip): every other shape with every channel count in [1, 512] -- one fp32
 *     arithmetic (MFMA / FMA chains) and a fixed launch sequence per step (lifting 1x1 GELU 1x1, per layer the spectral
 *     convolution in three launches + the skip 1x1 with bias, GELU and the spectral output fused, projection 1x1 GELU
 *     1x1 + residual).  precision_form / launch_form / on_timeout / unchecked / debug_spin_limit are validated and
 *     otherwise ignored; it has no hand-offs and no f16 range: dlwp_fno2d_status returns DLWP_OK, the statistics 0.
 * Either way the width must be a multiple of 64; other shapes return DLWP_ERR_UNSUPPORTED naming the limit. */
typedef struct dlwp_fno2d_desc {
  int32_t in_channels;         /* constant + (prescribed + prognostic) * context  (1..512)  */
  int32_t hidden_channels;     /* fno.py:24  (1..512; 32 runs the specialised kernels)      */
  int32_t lifting_channels;    /* fno.py:25  (1..512)                                       */
  int32_t projection_channels; /* fno.py:26  (1..512)                                       */
  int32_t out_channels;        /* = prognostic_channels, fno.py:45 (1..512)                 */
  int32_t n_layers;            /* fno.py:27                                                 */
  int32_t height, width;       /* grid; width must be a multiple of 64                      */
  int32_t n_rows;              /* kept spectral rows   (neuralop: min(H, n_modes[0]))       */
  int32_t n_cols;              /* kept rfft columns    (neuralop: n_modes[1]/2+1)           */
  const int32_t* rows_in;      /* host [n_rows]: un-shifted rfft row read by weight row r   */
  const int32_t* rows_out;     /* host [n_rows]: un-shifted row of out_fft it lands in      */
  float fwd_scale;             /* rfftn normalisation  (norm="forward": 1/(H*W))            */
  float inv_scale;             /* irfftn normalisation (norm="forward": 1)                  */
  /* weights, HOST pointers, reference (PyTorch) layouts, fp32 */
  const float* lift_w1;        /* [lifting, in]                                             */
  const float* lift_b1;        /* [lifting]                                                 */
  const float* lift_w2;        /* [hidden, lifting]                                         */
  const float* lift_b2;        /* [hidden]                                                  */
  const float* const* spec_w;  /* n_layers x [hidden(in), hidden(out), n_rows, n_cols, 2]   */
  const float* spec_b;         /* [n_layers, hidden]                                        */
  const float* const* skip_w;  /* n_layers x [hidden(out), hidden(in)]                      */
  const float* proj_w1;        /* [projection, hidden]                                      */
  const float* proj_b1;        /* [projection]                                              */
  const float* proj_w2;        /* [out, projection]                                         */
  const float* proj_b2;        /* [out]                                                     */
  /* ---- execution form, fixed for the life of the plan (no process-wide switches exist) ---- */
  int32_t precision_form;      /* 0 (default): the fp32 channel GEMMs run as "bf16x6" -- each fp32 operand split exactly
                                  into three bf16 parts, the six significant cross products accumulated in fp32 on the
                                  bf16 matrix pipe (fp32-GEMM accuracy) -- and the fused kernels;
                                  1: plain fp32-MFMA kernels and the unfused spectral path (independent cross-check);
                                  2: "f16x3" in the fused step kernel -- operands split into two f16 parts (22 significant
                                  bits, the weight residual stored scaled), three products on the f16 matrix instructions:
                                  fp32-GEMM accuracy for |activation| < 65504 at half the matrix instructions and split
                                  work.  A range whose output is not finite is repeated on the
                                  bf16x6 kernels (checked calls) or reported by dlwp_fno2d_status as DLWP_ERR_RANGE
                                  (unchecked = 1).  Kernels other than the fused step keep bf16x6. */
  int32_t launch_form;         /* 0 (default): fewest launches the shapes allow (whole rollout range in one persistent
                                  launch); 1: one launch per step; 2: three launches per step; 3: unfused kernels */
  int32_t on_timeout;          /* a fused launch whose hand-off spin ran out: 0 (default) re-run the range on the unfused
                                  kernels (no hand-offs) and return DLWP_OK; 1 return DLWP_ERR_TIMEOUT */
  int32_t unchecked;           /* 0 (default): every call that used fused kernels synchronises `stream` once and reads
                                  their fail word; 1: fully asynchronous calls, the caller polls dlwp_fno2d_status */
  int32_t debug_spin_limit;    /* 0: default bound (~0.1 s); > 0: spin bound of the hand-offs (test hook) */
  int32_t lift_table;          /* in_channels == 1 on the fused step kernel: 0 (default) the lifting MLP -- a function of one
                                  scalar per grid point -- is read from a table built when the plan is created (quintic
                                  Hermite, h = 1/16 over [-32, 32); kept only if a guard finds it within 2^-22 of the fp64
                                  function for these weights; a row with a value outside the domain is evaluated as before);
                                  1: off, the MLP is always evaluated.  See dlwp_fno2d_lift_table_state. */
} dlwp_fno2d_desc;

int32_t dlwp_fno2d_plan_create(dlwp_fno2d_plan** plan, const dlwp_fno2d_desc* desc, void* stream);
int32_t dlwp_fno2d_plan_destroy(dlwp_fno2d_plan* plan);
/* bytes of device workspace one call needs for `batch` samples */
size_t dlwp_fno2d_workspace_bytes(const dlwp_fno2d_plan* plan, int32_t batch);
/* Deferred check for plans created with unchecked = 1 (fully asynchronous calls): synchronises `stream` and returns
 * DLWP_ERR_TIMEOUT if any fused launch of this plan timed out since the previous status call (a plan-owned device counter
 * the kernels add to; reset here).  The outputs of such launches are poisoned with NaN.  DLWP_ERR_RANGE: an f16x3 launch
 * (precision_form 2) wrote a non-finite output since the previous status call. */
int32_t dlwp_fno2d_status(const dlwp_fno2d_plan* plan, void* stream);
/* statistics: fused launches of this plan that timed out so far (re-run or reported) */
uint32_t dlwp_fno2d_timeouts(const dlwp_fno2d_plan* plan);
/* statistics: f16x3 step ranges of this plan (precision_form 2) repeated on the bf16x6 kernels after a non-finite output */
uint32_t dlwp_fno2d_range_reruns(const dlwp_fno2d_plan* plan);

/* The one-input-channel lifting table of a plan: 0 not applicable (another shape or launch form, more input channels),
 * 1 in use, 2 rejected by the guard for these weights (the MLP is evaluated), 3 switched off (desc.lift_table = 1 or
 * DLWP_FNO_LIFT_TABLE=0 in the environment when the plan was created). */
int32_t dlwp_fno2d_lift_table_state(const dlwp_fno2d_plan* plan);
/* Host only, no device needed: the builder the plans use.  Fills table [2 * range * 2^log2_inv_h][6][32] (fp32) for
 * lift(x)[o] = b2[o] + sum_c W2[o][c] gelu(w1[c] x + b1[c]) (weights in the descriptor's layouts, one input channel, 32 outputs)
 * over [-range, range) with knots at multiples of 2^-log2_inv_h.  *guard_err (may be NULL): the largest relative vector error
 * the guard found (NaN if anything was not finite); *accepted (may be NULL): 1 if it is <= 2^-22, else 0. */
int32_t dlwp_fno2d_lift_table_build(const float* lift_w1, const float* lift_b1, const float* lift_w2,
                                    const float* lift_b2, int32_t lifting, int32_t range, int32_t log2_inv_h,
                                    float* table, size_t table_floats, double* guard_err, int32_t* accepted);
/* Host only: evaluates such a table at x[0..n) with the arithmetic of the device (interval and coordinate exact in fp32,
 * fp32 fmaf Horner).  out [n][32]; v_out [n] (may be NULL) the coordinate in [0, 1) from the interval's end nearer zero;
 * interval_out [n] (may be NULL) the interval index.  An x outside the domain (|x| >= range, NaN) gives NaN and -1. */
int32_t dlwp_fno2d_lift_table_eval_host(const float* table, int32_t range, int32_t log2_inv_h, const float* x,
                                        int64_t n, float* out, float* v_out, int32_t* interval_out);

/* One backbone step WITHOUT the residual: y = fno(x).  Replaces `self.fno(x_t)` at fno.py:103.
 * x_dev [B, in, H, W], y_dev [B, out, H, W], both contiguous fp32. */
int32_t dlwp_fno2d_forward_f32(const dlwp_fno2d_plan* plan, const float* x_dev, float* y_dev,
                               int32_t batch, void* workspace_dev, size_t workspace_bytes,
                               void* stream);

/* Whole autoregressive rollout, device resident.  Replaces FNO2DModule.forward, fno.py:64-106
 * (loop + _prepare_inputs + residual + stack).  Tensors are contiguous fp32:
 *   constants_dev  [B, 1, Cc, H, W] or NULL (Cc = 0)
 *   prescribed_dev [B, T, Cp, H, W] or NULL (Cp = 0)
 *   prognostic_dev [B, T, Cg, H, W]
 *   out_dev        [B, T - context, Cg, H, W]
 * with Cc + (Cp + Cg) * context == plan in_channels and Cg == plan out_channels. */
int32_t dlwp_fno2d_rollout_f32(const dlwp_fno2d_plan* plan, const float* constants_dev,
                               int32_t n_const, const float* prescribed_dev, int32_t n_presc,
                               const float* prognostic_dev, int32_t n_prog, int32_t batch,
                               int32_t n_time, int32_t context, float* out_dev,
                               void* workspace_dev, size_t workspace_bytes, void* stream);

/* Rollout steps [step_begin, step_end) only (0 <= begin <= end <= T - context); steps before
 * step_begin must already be present in out_dev.  Lets the host overlap the all-gather of finished
 * time chunks with the remaining steps (dlwp_benchmark_amd/sharding.py). */
int32_t dlwp_fno2d_rollout_range_f32(const dlwp_fno2d_plan* plan, const float* constants_dev,
                                     int32_t n_const, const float* prescribed_dev, int32_t n_presc,
                                     const float* prognostic_dev, int32_t n_prog, int32_t batch,
                                     int32_t n_time, int32_t context, float* out_dev,
                                     void* workspace_dev, size_t workspace_bytes, void* stream,
                                     int32_t step_begin, int32_t step_end);

/* Same rollout with every kernel launch bracketed by a pair of HIP events on `stream`
 * (measurement aid for bench.py's roofline leg; synchronises the stream before returning).
 * Kernel classes: 0 lifting MLP, 1 fno_modes_kernel, 2 fno_layer_kernel, 3 projection MLP,
 * 4 an EMPTY bracket per step (what the event pair itself adds; subtract its average from the others).
 * class_ms[5]: summed event-to-event milliseconds, class_launches[5]: brackets per class. */
int32_t dlwp_fno2d_rollout_profiled_f32(const dlwp_fno2d_plan* plan, const float* constants_dev,
                                        int32_t n_const, const float* prescribed_dev,
                                        int32_t n_presc, const float* prognostic_dev,
                                        int32_t n_prog, int32_t batch, int32_t n_time,
                                        int32_t context, float* out_dev, void* workspace_dev,
                                        size_t workspace_bytes, void* stream, double* class_ms,
                                        int32_t* class_launches);

/* ------------------------------------------------------------------------------------------
 * SpectralConv2d  (reference models/unet/unet.py:19-69 + batchmul2d :15-17; PDE-Arena style:
 * un-normalised rfft2, rows [:m1] with weights1 and rows [-m1:] with weights2, cols [:m2],
 * irfft2).  x_dev [B, Ci, H, W] -> y_dev [B, Co, H, W], contiguous fp32.
 * Ci == Co == 32 on a width that is a multiple of 64 with at most 16 kept columns runs the specialised kernels
 * (csrc/fno_unfused.hpp); every other shape with Ci, Co in [1, 512], any H, a width that is a multiple of 4 and
 * H x 2 n_cols within the transform kernels' LDS image (128 KB) runs the width-generic ones (csrc/spectral_any.hip,
 * fp32 throughout).  Shapes outside both return DLWP_ERR_UNSUPPORTED naming the limit.
 * ------------------------------------------------------------------------------------------ */
typedef struct dlwp_spectral_plan dlwp_spectral_plan;

int32_t dlwp_spectral_conv2d_plan_create(dlwp_spectral_plan** plan, int32_t in_channels,
                                         int32_t out_channels, int32_t height, int32_t width,
                                         int32_t modes1, int32_t modes2,
                                         const float* weights1_host, /* [Ci,Co,m1,m2,2] */
                                         const float* weights2_host, /* [Ci,Co,m1,m2,2] */
                                         void* stream);
/* The same operator with explicit kept rows and transform scales (SpectralCore of the FNO layers: row r of the
 * weights reads un-shifted rfft row rows_in[r] and writes row rows_out[r]; x_hat is scaled by fwd_scale, the inverse
 * by inv_scale) and weights that live on the DEVICE -- what a training step needs (reference
 * scripts/train.py:263-271 `loss.backward()` through models/unet/unet.py:46-69 / neuralop SpectralConv).
 * dlwp_spectral_conv2d_set_weights_dev packs weights_dev [Ci, Co, n_rows, n_cols, 2] (PyTorch layout, forward
 * operator) into the plan on `stream`; with adjoint != 0 it packs the conjugate transpose, which makes
 * dlwp_spectral_conv2d_f32 the BACKWARD-DATA pass (create that plan with rows_in and rows_out swapped). */
int32_t dlwp_spectral_conv2d_plan_create_ex(dlwp_spectral_plan** plan, int32_t in_channels, int32_t out_channels,
                                            int32_t height, int32_t width, int32_t n_rows, int32_t n_cols,
                                            const int32_t* rows_in, const int32_t* rows_out, float fwd_scale,
                                            float inv_scale, void* stream);
int32_t dlwp_spectral_conv2d_set_weights_dev(dlwp_spectral_plan* plan, const float* weights_dev, int32_t adjoint,
                                             void* stream);
int32_t dlwp_spectral_conv2d_plan_destroy(dlwp_spectral_plan* plan);
size_t dlwp_spectral_conv2d_workspace_bytes(const dlwp_spectral_plan* plan, int32_t batch);
int32_t dlwp_spectral_conv2d_f32(const dlwp_spectral_plan* plan, const float* x_dev, float* y_dev,
                                 int32_t batch, void* workspace_dev, size_t workspace_bytes,
                                 void* stream);
/* Weight gradient of the FORWARD plan `plan` (reference scripts/train.py:263-271 `loss.backward()` through
 * models/unet/unet.py:46-69: what autograd derives from rfft2 :56, the two einsums of batchmul2d :15-17 / :60-65 and
 * irfft2 :68; the same for neuralop's SpectralConv inside FNO2DModule, fno.py:38-47):
 *   grad_w[i, o, r, k] = sum_b conj(fwd_scale X[b, i, rows_in[r], k]) * inv_scale c_k * DY[b, o, rows_out[r], k]
 * with X = rfft2(x), DY = rfft2(grad_y) un-normalised and c_k = 1 for k = 0 and the Nyquist column, 2 otherwise.
 * x_dev [B, Ci, H, W], grad_y_dev [B, Co, H, W]; grad_w_dev [Ci, Co, n_rows, n_cols, 2] fp32 (PyTorch layout) is
 * OVERWRITTEN.  Four launches on `stream`, no host synchronisation: the pruned forward transform of x and of grad_y
 * at the kept modes, one fp32 FMA contraction whose sum over b runs in index order in one thread (no atomics:
 * bitwise repeatable) into a packed [mode][Ci][Co] image in the workspace, and its transpose into PyTorch layout.  The width-generic kernels (csrc/spectral_any.hip) are the only form: Ci, Co in [1, 512],
 * width a multiple of 4, one plane's LDS image within 128 KB; a plan of the specialised 32-channel kernels builds the
 * generic tables from its own description on its first call here.  Outside that domain: DLWP_ERR_UNSUPPORTED naming
 * the limit.  The first dlwp_spectral_conv2d_wgrad_f32 of a plan uploads tables and synchronises `stream`: make it
 * before a stream capture.  A plan is used from one thread at a time. */
size_t dlwp_spectral_conv2d_wgrad_workspace_bytes(const dlwp_spectral_plan* plan, int32_t batch);
int32_t dlwp_spectral_conv2d_wgrad_f32(const dlwp_spectral_plan* plan, const float* x_dev, const float* grad_y_dev,
                                       float* grad_w_dev, int32_t batch, void* workspace_dev, size_t workspace_bytes,
                                       void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused (shifted-)window attention, fp32.  Replaces everything between the qkv Linear and the proj
 * Linear of a transformer block:
 *   Swin : models/swintransformer/swin_transformer.py:217-251 (pad, roll, window_partition,
 *          WindowAttention.forward :122-154 without its two Linears, window_reverse, roll, crop) and
 *          the per-call shift-mask build :383-401
 *   Pangu: models/panguweather/panguweather.py:285-316 + EarthAttention3D.forward :176-211 without
 *          its two Linears, utils/shift_window_mask.py, utils/earth_position_index.py, utils/pad.py,
 *          utils/crop.py
 * qkv_dev  [B, L, 3, heads, head_dim]  output of the qkv Linear on the un-padded token sequence,
 *          L = grid[0]*grid[1]*grid[2] (a 2-D model uses grid[0] = window[0] = 1)
 * qkv_bias_dev [3*heads*head_dim] or NULL: value of q,k,v at zero-padded tokens (the reference
 *          pads before the Linear); required when padded != grid
 * table_dev  bias_mode 0: relative_position_bias_table [(2Wh-1)(2Ww-1), heads]
 *            bias_mode 1: earth_position_bias_table [wpl^2*wlat^2*(2wlon-1), types, heads],
 *                         types = (padded[0]/window[0]) * (padded[1]/window[1])
 * out_dev  [B, L, heads*head_dim] in the input token order (window reverse / roll back / crop done)
 * ------------------------------------------------------------------------------------------ */
typedef struct dlwp_wattn_desc {
  int32_t grid[3];        /* un-padded (pl, lat, lon)                                          */
  int32_t padded[3];      /* padded grid, multiple of window                                   */
  int32_t pad_lead[3];    /* zeros added in front / top / left                                 */
  int32_t window[3];
  int32_t shift_fwd[3];   /* torch.roll(x, shifts=-shift_fwd) before partitioning              */
  int32_t shift_back[3];  /* torch.roll(y, shifts=+shift_back) after window_reverse            */
  int32_t use_mask;       /* add the 0/-100 region mask                                        */
  int32_t mask_b1[3];     /* region id along a dim = (p >= mask_b1) + (p >= mask_b2), p being  */
  int32_t mask_b2[3];     /*   the coordinate in the shifted, padded frame                     */
  int32_t bias_mode;      /* 0 Swin relative position, 1 Pangu earth-specific                  */
  int32_t heads, head_dim;
  float scale;            /* qk scale (head_dim ** -0.5 unless overridden)                     */
  int32_t form;           /* dlwp_window_attn_f32 only: -1 by window size (default), 0 fp32 MFMA, 1 bf16x6 */
} dlwp_wattn_desc;

/* fp32-accurate window attention (the parity path), in one of two independent forms of the two contractions:
 * fp32 operands on v_mfma_f32_16x16x4_f32, or exact three-way bf16 splits of Q, K, V and P with six cross products each
 * on the bf16 matrix pipe ("bf16x6").  desc->form selects: 0 fp32 MFMA, 1 bf16x6, -1 by window size as measured
 * (>= 512 tokens per window: fp32 MFMA; smaller: bf16x6).  No process-wide switch exists.
 * tokens * 3 * heads * head_dim must stay below 2^31. */
/* bytes of device workspace the FAST path of the call below needs for this descriptor (bf16 != 0: for
 * dlwp_window_attn_bf16); 0 when the descriptor runs on the generic kernel, which needs none.  The fast path covers
 * 2-D windows (bias_mode 0, grid[0] = 1, no zero padding, window longitude extent a multiple of 16, head_dim a multiple
 * of 8 but not of 32, region boundaries along longitude on multiples of 16): every Swin block of the reference.  Its
 * workspace holds the window-ordered bf16 operand images a prep kernel writes per call.  Masked
 * (shifted-window) tiles are skipped there: exact unless a masked logit exceeds its row's unmasked maximum by > 83. */
size_t dlwp_window_attn_workspace_bytes(const dlwp_wattn_desc* desc, int32_t batch, int32_t bf16);
/* Diagnostics (synchronises `stream`): workgroups of the LAST fast-path call on this workspace whose scores left the
 * 2^+-100 exponent slack around their reference offset and were recomputed with the exact row maximum. */
int32_t dlwp_window_attn_fallbacks(const dlwp_wattn_desc* desc, int32_t batch, int32_t bf16, const void* workspace_dev,
                                   void* stream, int32_t* count);
/* workspace_dev may be NULL (or smaller than the bytes above): the generic kernel runs instead. */
int32_t dlwp_window_attn_f32(const dlwp_wattn_desc* desc, const float* qkv_dev,
                             const float* qkv_bias_dev, const float* table_dev, float* out_dev,
                             int32_t batch, void* workspace_dev, size_t workspace_bytes, void* stream);
/* Same interface (fp32 tensors in and out); Q, K, V and the softmax probabilities are rounded to bf16
 * and both products run on v_mfma_f32_16x16x32_bf16 with fp32 accumulation and fp32 softmax statistics
 * (the precision BASELINE.json names for the Swin / Pangu configs). */
int32_t dlwp_window_attn_bf16(const dlwp_wattn_desc* desc, const float* qkv_dev,
                              const float* qkv_bias_dev, const float* table_dev, float* out_dev,
                              int32_t batch, void* workspace_dev, size_t workspace_bytes, void* stream);

/* dlwp_window_attn_bf16 with bfloat16 TENSORS: qkv_dev [B, L, 3 C], qkv_bias_dev [3 C] and out_dev [B, L, C] are bf16 -- the
 * hand-over of a block in the bf16 form (the qkv Linear writes bf16, proj reads bf16: dlwp_linear_bf16_io).  Same arithmetic as
 * dlwp_window_attn_bf16 on bf16-rounded inputs.  Covered: the descriptors of the two fast paths (workspace as for
 * dlwp_window_attn_bf16); anything else returns DLWP_ERR_UNSUPPORTED (convert and call dlwp_window_attn_bf16).
 * 2-D (Swin) descriptors run WITHOUT the prep kernel: the attention kernel gathers Q, K, V from qkv_dev itself (window order and
 * roll through an LDS token map), so the images part of the workspace stays unused; shifted blocks launch one small key-norm
 * kernel in front.  dlwp_window_attn_fallbacks is maintained for shifted blocks only on this entry point. */
int32_t dlwp_window_attn_bf16_io(const dlwp_wattn_desc* desc, const void* qkv_dev, const void* qkv_bias_dev,
                                 const float* table_dev, void* out_dev, int32_t batch, void* workspace_dev,
                                 size_t workspace_bytes, void* stream);

/* Backward of dlwp_window_attn_f32 (csrc/window_attn_bwd.hip): what loss.backward() of reference scripts/train.py:263-271
 * runs through WindowAttention.forward (swin_transformer.py:122-154, :217-251) / EarthAttention3D.forward
 * (panguweather.py:176-211, :285-316), without their Linears.  Flash-style: scores are recomputed per 32 x 32 tile from
 * qkv and per-row statistics; no N x N tensor exists.  fp32 arithmetic.
 *   grad_out_dev      [B, L, C]      gradient of the attention output (same token order as out_dev)
 *   grad_qkv_dev      [B, L, 3 C]    written (zeroed inside; dq arrives through float atomics)
 *   grad_qkv_bias_dev [3 C] or NULL  gradient that reaches the qkv bias through ZERO-PADDED tokens (they carry q = k = v =
 *                                    bias); required when the descriptor pads, written (zeroed inside)
 *   grad_table_dev    like table_dev written (zeroed inside)
 *   workspace_dev     dlwp_window_attn_bwd_workspace_bytes(desc, batch) bytes: {row max, row sum, delta} per window row */
size_t dlwp_window_attn_bwd_workspace_bytes(const dlwp_wattn_desc* desc, int32_t batch);
int32_t dlwp_window_attn_bwd_f32(const dlwp_wattn_desc* desc, const float* qkv_dev, const float* qkv_bias_dev,
                                 const float* table_dev, const float* grad_out_dev, float* grad_qkv_dev,
                                 float* grad_qkv_bias_dev, float* grad_table_dev, int32_t batch, void* workspace_dev,
                                 size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * AFNO2D frequency-domain mixing (reference models/fourcastnet/fourcastnet.py:87-121): complex
 * block-diagonal 2-layer MLP with ReLU, mode truncation and softshrink over the rfft2 spectrum.
 * xf_dev / yf_dev: interleaved complex64, CHANNELS-FIRST [B, C, H, Wf, 2] (Wf = W/2+1) -- the physical
 * layout torch.fft.rfft2(x_nhwc, dim=(1,2)) produces and irfft2 consumes without a copy; weights in the
 * reference layouts w1,w2 [2, nb, bs, bs], b1,b2 [2, nb, bs] (device pointers), bs in {4,8,16,32}.
 * yf is fully written (zeros outside the kept modes).
 * hard_thresholding_fraction is a DOUBLE in the three entry points below: kept = int((H/2+1) * fraction) must be the product of
 * doubles the reference forms (:93-94); as a float, 0.7 and 0.9 keep one mode fewer wherever that product is an integer (H = 18).
 * ------------------------------------------------------------------------------------------ */
int32_t dlwp_afno2d_mix_f32(const float* xf_dev, float* yf_dev, const float* w1_dev, const float* b1_dev,
                            const float* w2_dev, const float* b2_dev, int32_t batch, int32_t height,
                            int32_t wf, int32_t channels, int32_t num_blocks, float sparsity_threshold,
                            double hard_thresholding_fraction, void* stream);
/* Backward of the mixing between UNNORMALISED transforms (training; fourcastnet.py:96-121 under loss.backward()):
 * xf = R2C(x), gf = R2C(grad_y), both [B, C, H, Wf, 2] as above (Wf = the columns the transforms carry; `width` = W of the
 * real field, for the Hermitian weight of the Nyquist column).  Writes gxf (its C2R is grad_x) and the per-point factors of the
 * weight gradients -- xin, o1 (post-ReLU), d1, d2 (masked upstream gradients), same layout, zeros outside the kept modes:
 * dW1 = sum_p conj(xin) (x) d1, db1 = sum_p d1, dW2 = sum_p conj(o1) (x) d2, db2 = sum_p d2 per block (csrc/afno.hip). */
int32_t dlwp_afno2d_mix_bwd_f32(const float* xf_dev, const float* gf_dev, float* gxf_dev, float* xin_dev, float* o1_dev,
                                float* d1_dev, float* d2_dev, const float* w1_dev, const float* b1_dev, const float* w2_dev,
                                const float* b2_dev, int32_t batch, int32_t height, int32_t wf, int32_t channels,
                                int32_t num_blocks, int32_t width, float sparsity_threshold, double hard_thresholding_fraction,
                                float in_scale, float out_scale, void* stream);
/* Same with yf = out_scale * mix(in_scale * xf): lets the caller use UNNORMALISED transforms (below) and still get
 * the reference's norm="ortho" arithmetic (:87, :122; in_scale = out_scale = 1/sqrt(H*W)) without two elementwise
 * passes over the spectrum.  yf_dev may be xf_dev (in place): a point's channels are read before they are written and
 * no other point is read by the thread that writes it. */
int32_t dlwp_afno2d_mix_scaled_f32(const float* xf_dev, float* yf_dev, const float* w1_dev, const float* b1_dev,
                                   const float* w2_dev, const float* b2_dev, int32_t batch, int32_t height,
                                   int32_t wf, int32_t channels, int32_t num_blocks, float sparsity_threshold,
                                   double hard_thresholding_fraction, float in_scale, float out_scale, void* stream);

/* Batched unnormalised 2-D real FFTs of `batch` contiguous [H, W] planes (reference fourcastnet.py:87
 * `torch.fft.rfft2(x, dim=(1, 2))` and :122-123 `irfft2`, applied channels-first so that batch = B * C) through
 * hipFFT, without the clone, layout copies and scaling pass torch.fft adds per call.
 *   dlwp_rfft2_f32:  x_dev [batch][H][W] -> xf_dev [batch][H][W/2+1][2]
 *   dlwp_irfft2_f32: yf_dev [batch][H][W/2+1][2] -> y_dev [batch][H][W]; yf_dev is DESTROYED (C2R scratch). */
typedef struct dlwp_fft2_plan dlwp_fft2_plan;
int32_t dlwp_fft2_plan_create(dlwp_fft2_plan** out, int32_t batch, int32_t height, int32_t width);
int32_t dlwp_fft2_plan_destroy(dlwp_fft2_plan* plan);
int32_t dlwp_rfft2_f32(const dlwp_fft2_plan* plan, const float* x_dev, float* xf_dev, void* stream);
int32_t dlwp_irfft2_f32(const dlwp_fft2_plan* plan, float* yf_dev, float* y_dev, void* stream);

/* Hand-written 2-D real FFTs restricted to the columns the AFNO filter keeps (fourcastnet.py:85, :93-94, :124;
 * csrc/afno_fft.hip): one workgroup per [H][W] plane, rows as packed-real FFTs, columns on the LDS-resident image,
 * every complex FFT as two register passes (radix 4 / 8 / 16).  Unnormalised, like the hipFFT entry points above.
 *   dlwp_afno_rfft2_kept_f32:  x_dev [planes][H][W] -> spec_dev [planes][H][kept_cols][2]
 *   dlwp_afno_irfft2_kept_f32: spec_dev [planes][H][kept_cols][2] (columns >= kept_cols are zero; the imaginary part
 *                              of column 0 is ignored, c2r semantics) -> y_dev [planes][H][W]; spec_dev is preserved.
 * kept_cols = min(int((H/2+1) * hard_thresholding_fraction), W/2+1).  Instantiated grids: dlwp_afno_fft_supported. */
typedef struct dlwp_afno_fft_plan dlwp_afno_fft_plan;
int32_t dlwp_afno_fft_supported(int32_t height, int32_t width, int32_t kept_cols);
int32_t dlwp_afno_fft_plan_create(dlwp_afno_fft_plan** out, int32_t height, int32_t width, int32_t kept_cols, void* stream);
int32_t dlwp_afno_fft_plan_destroy(dlwp_afno_fft_plan* plan);
int32_t dlwp_afno_rfft2_kept_f32(const dlwp_afno_fft_plan* plan, const float* x_dev, float* spec_dev, int32_t planes,
                                 void* stream);
int32_t dlwp_afno_irfft2_kept_f32(const dlwp_afno_fft_plan* plan, const float* spec_dev, float* y_dev, int32_t planes,
                                  void* stream);

/* ------------------------------------------------------------------------------------------
 * CylinderPad(1) + Conv2d(3x3, padding 0) + bias + activation, input optionally given as two
 * channel segments (folds the preceding torch.cat).  Reference: utils/utils.py:11-26;
 * models/unet/unet.py:456-470, :512-525, :553; models/convlstm/convlstm.py:47-55, :94, :148-157.
 * x0_dev [B, c0, H, W], x1_dev [B, c1, H, W] or NULL (c1 = 0), weight_dev [cout, c0+c1, 3, 3],
 * bias_dev [cout] or NULL, y_dev [B, cout, H, W].  act: 0 none, 1 GELU(erf), 2 tanh, 3 ReLU, 4 SiLU.
 * ------------------------------------------------------------------------------------------ */
int32_t dlwp_conv3x3_cyl_f32(const float* x0_dev, int32_t c0, const float* x1_dev, int32_t c1,
                             const float* weight_dev, const float* bias_dev, float* y_dev, int32_t batch,
                             int32_t height, int32_t width, int32_t cout, int32_t act, void* stream);

/* The same convolution with two more fusions and either padding rule: pre_act is applied to the input while it is staged
 * (pre-activation residual blocks, unet.py:886 `h = act(norm1(x))` when norm1 is the identity), resid_dev [B, cout, H, W]
 * or NULL is added after the bias and before `act` (the block's shortcut, unet.py:901).  ring_table NULL: CylinderPad;
 * otherwise the HEALPix halo table of dlwp_conv3x3_hpx_f32 (batch = 12 * samples faces). */
int32_t dlwp_conv3x3_ex_f32(const float* x0_dev, int32_t c0, const float* x1_dev, int32_t c1, const float* weight_dev,
                            const float* bias_dev, const float* resid_dev, float* y_dev, int32_t batch, int32_t height,
                            int32_t width, int32_t cout, int32_t pre_act, int32_t act, const int32_t* ring_table, void* stream);

/* dlwp_conv3x3_ex_f32 as an implicit GEMM on the bf16 matrix instructions (csrc/conv_mfma.hip; same reference lines:
 * utils/utils.py:11-26; models/unet/unet.py:456-470, :512-525, :553, :886, :901; models/convlstm/convlstm.py:47-55, :94,
 * :148-157; utils/healpix.py:316-368).  The weight [cout, cin, 3, 3] is packed once into MFMA operand order (three bf16
 * images, tap-major, cin zero-filled to 32 and cout to 16): dlwp_conv3x3_mfma_packed_bytes gives the size (0 = unsupported
 * shape), dlwp_conv3x3_mfma_pack_f32 fills it.  form 0 "bf16x6": exact three-part bf16 splits of both operands, six products,
 * fp32 accumulation -- fp32-grade; form 1 "bf16": RNE bf16 operands (first image only), fp32 accumulation.  Every other
 * argument and check as dlwp_conv3x3_ex_f32; shapes whose per-sample offsets leave 32 bits return DLWP_ERR_UNSUPPORTED.
 * One writer per output element: results are bit-identical from run to run.
 * dlwp_conv3x3_mfma_variant names the kernel instance the launcher takes for a shape: 16 * tile width (16: 8 x 16 pixels,
 * 8: 16 x 8) + output fragments per workgroup (4, 2 or 1); 0 for a non-positive size or a map past the 32-bit offsets: it is
 * dlwp_conv2d_mfma_variant(0, batch, height, width, cout, 3, 1, 1), as dlwp_conv3x3_mfma_packed_bytes(cout, cin) is
 * dlwp_conv2d_mfma_packed_bytes(cout, cin, 3).  For tests and tools. */
size_t dlwp_conv3x3_mfma_packed_bytes(int32_t cout, int32_t cin);
int32_t dlwp_conv3x3_mfma_variant(int32_t batch, int32_t height, int32_t width, int32_t cout);
int32_t dlwp_conv3x3_mfma_pack_f32(const float* weight_dev, int32_t cout, int32_t cin, void* packed_dev, void* stream);
int32_t dlwp_conv3x3_mfma_f32(const float* x0_dev, int32_t c0, const float* x1_dev, int32_t c1, const void* packed_dev,
                              const float* bias_dev, const float* resid_dev, float* y_dev, int32_t batch, int32_t height,
                              int32_t width, int32_t cout, int32_t pre_act, int32_t act, const int32_t* ring_table,
                              int32_t form, void* stream);

/* dlwp_conv2d_f32 and dlwp_conv_transpose2d_f32 as implicit GEMMs on the bf16 matrix instructions (csrc/conv_mfma.hip, the kernel of
 * dlwp_conv3x3_mfma_f32 under another geometry policy; the
 * same reference lines: models/unet/unet.py:583 (3x3, stride 2, zero padding 1), :584 and :879-881 (1x1), :450 / :533 (1x1
 * head) for the convolution, :719 (4x4, stride 2, padding 1) and :523 (2x2, stride 2) for the transposed one).  The weight
 * ([cout, cin, k, k]; transposed != 0: [cin, cout, k, k]) is packed once into MFMA operand order, [image][tap][slab][16-channel
 * fragment][lane][8 bf16] for the k * k taps, cin zero-filled to 32 and cout to 16: dlwp_conv2d_mfma_packed_bytes gives the
 * size, 3 * k^2 * ceil(cin / 32) * ceil(cout / 16) * 1024 (0 = unsupported: a non-positive size, k > 4, or 2 GiB and more),
 * dlwp_conv2d_mfma_pack_f32 fills it.  form 0 "bf16x6" / 1 "bf16" as dlwp_conv3x3_mfma_f32; every other argument as the direct
 * entries.  Geometries: the convolution takes k <= 4, stride 1 or 2, pad < k; the transposed one k = 4 s = 2 p = 1 and
 * k = 2 s = 2 p = 0 (y_dev 8-byte aligned); anything else, and shapes whose per-sample offsets leave 32 bits, return
 * DLWP_ERR_UNSUPPORTED before any launch.  One writer per output element: results are bit-identical from run to run.
 * dlwp_conv2d_mfma_variant names the kernel instance a launcher takes: 16 * fragment width (16: rows of 16 GEMM pixels, 8: two
 * rows of 8) + output fragments per workgroup (4, 2 or 1; stride-2 convolutions 4 or 2); 0 for arguments the launcher
 * refuses.  For tests and tools. */
size_t dlwp_conv2d_mfma_packed_bytes(int32_t cout, int32_t cin, int32_t k);
int32_t dlwp_conv2d_mfma_variant(int32_t transposed, int32_t batch, int32_t height, int32_t width, int32_t cout, int32_t k,
                                 int32_t stride, int32_t pad);
int32_t dlwp_conv2d_mfma_pack_f32(const float* weight_dev, int32_t cout, int32_t cin, int32_t k, int32_t transposed,
                                  void* packed_dev, void* stream);
int32_t dlwp_conv2d_mfma_f32(const float* x_dev, const void* packed_dev, const float* bias_dev, const float* resid_dev,
                             float* y_dev, int32_t batch, int32_t cin, int32_t height, int32_t width, int32_t cout, int32_t k,
                             int32_t stride, int32_t pad, int32_t pre_act, int32_t act, int32_t form, void* stream);
int32_t dlwp_conv_transpose2d_mfma_f32(const float* x_dev, const void* packed_dev, const float* bias_dev, float* y_dev,
                                       int32_t batch, int32_t cin, int32_t height, int32_t width, int32_t cout, int32_t k,
                                       int32_t stride, int32_t pad, int32_t act, int32_t form, void* stream);

/* The input gradient of the zero-padded Conv2d(cin -> cout, k, stride, pad) on the same kernel, form "bf16x6" (the gradient of
 * the training step's loss.backward(), scripts/train.py:271, through unet.py:450, :533, :583-584, :879-881):
 *   dx[b, ci, ih, iw] = sum_{co, kh, kw : ih = stride oh - pad + kh, iw = stride ow - pad + kw} weight[co, ci, kh, kw] gz[b, co, oh, ow]
 * gz_dev [batch, cout, SH, SW] with SH = (height + 2 pad - k) / stride + 1 (SW alike), dx_dev [batch, cin, height, width] at any
 * 4-byte offset.  EVERY element of dx is written: rows and columns that no output read (k2 s2 on an odd map, the holes of a
 * 1x1 s2) are computed zeros, no memset is needed.
 *   stride 1: the Conv2d forward of gz with padding k - 1 - pad; the pack has the channels exchanged and both tap axes reversed.
 *   stride 2: the parity form of the transposed layer on the GEMM pixel grid ceil(height / 2) x ceil(width / 2), an odd k
 *             zero-extended to k + 1 at the high tap index, stores cropped to height x width.  k 1 or 2 take pad 0, k 3 or 4
 *             pad 0, 1 or 2.
 * Anything else -- k > 4, stride > 2, pad >= k, the remaining stride-2 paddings, shapes whose per-sample offsets leave 32 bits --
 * returns DLWP_ERR_UNSUPPORTED before any launch.
 * dlwp_conv2d_mfma_pack_ex_f32 is dlwp_conv2d_mfma_pack_f32 with the two further modes: a pack of k_packed x k_packed taps
 * (k_packed >= k; dlwp_conv2d_mfma_packed_bytes(cout, cin, k_packed) bytes) whose taps at index k and above are zero, and
 * flip != 0: pack tap (th, tw) holds weight tap (k - 1 - th, k - 1 - tw).  cout and cin are the GEMM's output and input
 * channels; exchange != 0 reads the tensor as [cin, cout, k, k].  The adjoint pack of a Conv2d weight [cout, cin, k, k] is
 * pack_ex(weight, cin, cout, k, k_packed, 1, flip), with k_packed and flip from dlwp_conv2d_dgrad_mfma_variant.
 * dlwp_conv2d_dgrad_mfma_variant runs the launcher's own checks: 0 for what it refuses, otherwise 4096 * k_packed + 1024 * policy
 * (0: stride 1, the reversed pack; 1: stride 2, the parity form, unreversed) + 16 * fragment width + output fragments per
 * workgroup.  The ConvTranspose2d input gradient needs no entry: it is dlwp_conv2d_mfma_f32 on gz with the [cin, cout, k, k]
 * weight packed as a Conv2d weight of cin output and cout input channels. */
int32_t dlwp_conv2d_mfma_pack_ex_f32(const float* weight_dev, int32_t cout, int32_t cin, int32_t k, int32_t k_packed,
                                     int32_t exchange, int32_t flip, void* packed_dev, void* stream);
int32_t dlwp_conv2d_dgrad_mfma_variant(int32_t batch, int32_t cin, int32_t cout, int32_t height, int32_t width, int32_t k,
                                       int32_t stride, int32_t pad);
int32_t dlwp_conv2d_dgrad_mfma_f32(const float* gz_dev, const void* packed_dev, float* dx_dev, int32_t batch, int32_t cin,
                                   int32_t height, int32_t width, int32_t cout, int32_t k, int32_t stride, int32_t pad,
                                   void* stream);

/* ------------------------------------------------------------------------------------------
 * fp32 Linear layers on the bf16 matrix pipe with the block's pointwise work fused (csrc/linear.hip): the qkv / proj /
 * fc1 / fc2 Linears, GELU and residual adds of the Swin and Pangu blocks (swin_transformer.py:21-39, :107-120, :254-262;
 * panguweather.py:176-211, :318-322).
 *   out[m][n] = act(sum_k x[m][k] W[n][k] + bias[n]) + resid[m][n],  act: 0 none, 1 exact-erf GELU
 * fp32 tensors, fp32-GEMM accuracy (exact three-way bf16 splits of both operands, six cross products, fp32 accumulation).
 * weight_dev [out, in] (nn.Linear layout) is split once by dlwp_linear_pack_f32 into `packed_dev`
 * (dlwp_linear_packed_bytes bytes, caller-owned; 0 = unsupported: in % 32 != 0 or out % 4 != 0); bias / resid may be NULL,
 * resid may alias out (in-place residual).
 * ------------------------------------------------------------------------------------------ */
size_t dlwp_linear_packed_bytes(int32_t out_features, int32_t in_features);
int32_t dlwp_linear_pack_f32(const float* weight_dev, int32_t out_features, int32_t in_features, void* packed_dev, void* stream);
int32_t dlwp_linear_f32(const float* x_dev, const void* packed_dev, const float* bias_dev, const float* resid_dev,
                        float* out_dev, int64_t rows, int32_t in_features, int32_t out_features, int32_t act, void* stream);
/* The same Linear with bf16 operands (x rounded to bf16 on the fly, the first bf16 image of the weight) and fp32
 * accumulation -- what torch.autocast(bfloat16) makes of nn.Linear; one matrix-pipe product instead of six. */
int32_t dlwp_linear_bf16(const float* x_dev, const void* packed_dev, const float* bias_dev, const float* resid_dev,
                         float* out_dev, int64_t rows, int32_t in_features, int32_t out_features, int32_t act, void* stream);
/* The same Linear in the "f16x3" form: both operands split exactly into two f16 parts (22 significant bits; the weight
 * residual stored scaled by 2^11, so any weight magnitude keeps them), three products on the f16 matrix instructions
 * instead of six bf16 ones.  fp32-GEMM accuracy for |x| < 65504 (an x beyond the f16 range turns into inf: the caller's
 * contract; LayerNorm / GELU / attention outputs are orders of magnitude inside it) and for activations that are not
 * all tiny (the residual of |x| < 0.125 is an f16 subnormal, absolute spacing 2^-24).  `packed_dev` comes from
 * dlwp_linear_pack_f16x3 (same byte count as dlwp_linear_packed_bytes). */
/* dlwp_linear_bf16 with a bf16 TENSOR on one side -- how the MLP of a block hands its hidden activation from fc1 to fc2 in the
 * bf16 form (swin_transformer.py:21-39 under autocast): x_is_bf16: x_dev is bf16 [rows][in] (the values dlwp_linear_bf16 would round
 * its fp32 input to: bit-identical result); out_is_bf16: out_dev is bf16 [rows][out], rounded to nearest even after bias / GELU,
 * resid_dev must be NULL.  At least one of the two flags.  dlwp_layernorm_prebias_bf16out (below the LayerNorm entry points)
 * produces such an input. */
int32_t dlwp_linear_bf16_io(const void* x_dev, const void* packed_dev, const float* bias_dev, const float* resid_dev,
                            void* out_dev, int64_t rows, int32_t in_features, int32_t out_features, int32_t act,
                            int32_t x_is_bf16, int32_t out_is_bf16, void* stream);
int32_t dlwp_linear_pack_f16x3(const float* weight_dev, int32_t out_features, int32_t in_features, void* packed_dev, void* stream);
int32_t dlwp_linear_f16x3(const float* x_dev, const void* packed_dev, const float* bias_dev, const float* resid_dev,
                          float* out_dev, int64_t rows, int32_t in_features, int32_t out_features, int32_t act, void* stream);

/* ------------------------------------------------------------------------------------------
 * The remaining U-Net / ModernUNet operators (csrc/conv2.hip; GroupNorm: csrc/groupnorm_bwd.hip), NCHW fp32, activations as
 * above.
 *   dlwp_groupnorm_act_f32     y = act(GroupNorm(groups)(x)): unet.py:739 (+ GELU :761), :887-888; gamma / beta [C] or NULL
 *   dlwp_conv2d_f32            zero-padded Conv2d k x k, stride s: unet.py:583 (3x3 s2 p1), :584 / :879 / :450 (1x1);
 *                              optional pre_act on the input and resid_dev [N, cout, OH, OW] before `act`
 *   dlwp_conv_transpose2d_f32  ConvTranspose2d k x k, stride s, padding p (weight [cin, cout, k, k]): unet.py:719, :523
 *   dlwp_avgpool2x2_f32        AvgPool2d(2): unet.py:450
 * ------------------------------------------------------------------------------------------ */
int32_t dlwp_groupnorm_act_f32(const float* x_dev, const float* gamma_dev, const float* beta_dev, float* y_dev, int32_t batch,
                               int32_t channels, int32_t hw, int32_t groups, float eps, int32_t act, void* stream);
int32_t dlwp_conv2d_f32(const float* x_dev, const float* weight_dev, const float* bias_dev, const float* resid_dev, float* y_dev,
                        int32_t batch, int32_t cin, int32_t height, int32_t width, int32_t cout, int32_t k, int32_t stride,
                        int32_t pad, int32_t pre_act, int32_t act, void* stream);
int32_t dlwp_conv_transpose2d_f32(const float* x_dev, const float* weight_dev, const float* bias_dev, float* y_dev, int32_t batch,
                                  int32_t cin, int32_t height, int32_t width, int32_t cout, int32_t k, int32_t stride,
                                  int32_t pad, int32_t act, void* stream);
int32_t dlwp_avgpool2x2_f32(const float* x_dev, float* y_dev, int64_t planes, int32_t height, int32_t width, void* stream);
/* its adjoint: dx[2i + u][2j + v] = 0.25 gy[i][j] for gy_dev [planes, height / 2, width / 2]; every element of dx_dev [planes,
 * height, width] is written, a trailing odd row or column with 0 */
int32_t dlwp_avgpool2x2_bwd_f32(const float* gy_dev, float* dx_dev, int64_t planes, int32_t height, int32_t width, void* stream);

/* GroupNorm + activation for training (csrc/groupnorm_bwd.hip): unet.py:739 (+ GELU :761), :887-888 under the
 * `loss.backward()` of scripts/train.py:271.  With v = xh gamma_c + beta_c, xh = (x - mean) rstd, y = act(v):
 *   dlwp_groupnorm_act_fwd_stats_f32: dlwp_groupnorm_act_f32 (the same kernel, y bit for bit) that also writes
 *     stats_dev [batch * groups][2] = (mean, rstd) -- with x all that the backward needs; no v, y or xh is kept.
 *   dlwp_groupnorm_act_bwd_f32: dx = rstd (gv gamma_c - a - xh b), dgamma_c = sum_n sum_hw gv xh, dbeta_c = sum_n sum_hw gv
 *     with gv = gy act'(v) recomputed from x and stats, a / b the group means of gamma gv / gamma gv xh.  gamma_dev / beta_dev
 *     may be NULL (gamma = 1, beta = 0); dx_dev, dgamma_dev, dbeta_dev may each be NULL (not wanted, not computed).  Every
 *     sum has a fixed order (dgamma / dbeta: n ascending) and one writer: reruns are bitwise identical.  16-byte loads are
 *     used only when hw % 4 == 0 and x_dev, gy_dev, dx_dev are 16-byte aligned; any other input takes the scalar form.
 *     workspace_dev: dlwp_groupnorm_act_bwd_workspace_bytes(batch, channels) bytes (the per-row sums).
 *   dlwp_groupnorm_act_bwd_workspace_bytes: 2 * batch * channels floats (0 for a non-positive size). */
int32_t dlwp_groupnorm_act_fwd_stats_f32(const float* x_dev, const float* gamma_dev, const float* beta_dev, float* y_dev,
                                         float* stats_dev, int32_t batch, int32_t channels, int32_t hw, int32_t groups,
                                         float eps, int32_t act, void* stream);
size_t dlwp_groupnorm_act_bwd_workspace_bytes(int32_t batch, int32_t channels);
int32_t dlwp_groupnorm_act_bwd_f32(const float* x_dev, const float* stats_dev, const float* gamma_dev, const float* beta_dev,
                                   const float* gy_dev, float* dx_dev, float* dgamma_dev, float* dbeta_dev,
                                   void* workspace_dev, int32_t batch, int32_t channels, int32_t hw, int32_t groups, int32_t act,
                                   void* stream);

/* ------------------------------------------------------------------------------------------
 * HEALPix mesh.  Faces are folded into the batch, [(B*12), C, H, W], face index fastest
 * (reference models/unet/unet.py:413-426 `b c f h w -> (b f) c h w`).  The neighbour topology of
 * reference utils/healpix.py:165-368 (`HEALPixPadding`: rotated polar neighbours, synthesised corners) is
 * handed over as a device table of int32 pairs (a, b): source cells face*H*W + pixel inside the same
 * sample; b < 0 = copy a, else 0.5*a + 0.5*b.
 *   dlwp_healpix_pad_f32: the padding layer on its own, table [12][(H+2p)*(W+2p)][2], y [(B*12), C, H+2p, W+2p].
 *   dlwp_conv3x3_hpx_f32: HEALPixLayer(Conv2d 3x3) = HEALPixPadding(1) + Conv2d(padding 0) + bias +
 *   activation (healpix.py:69-114) in one kernel, ring table [12][(H+2)*(W+2)][2]; other arguments as
 *   dlwp_conv3x3_cyl_f32 with batch = n_faces = B*12.
 * ------------------------------------------------------------------------------------------ */
int32_t dlwp_healpix_pad_f32(const float* x_dev, float* y_dev, const int32_t* table_dev, int32_t n_faces,
                             int32_t channels, int32_t height, int32_t width, int32_t pad, void* stream);
int32_t dlwp_conv3x3_hpx_f32(const float* x0_dev, int32_t c0, const float* x1_dev, int32_t c1,
                             const float* weight_dev, const float* bias_dev, float* y_dev, int32_t n_faces,
                             int32_t height, int32_t width, int32_t cout, int32_t act,
                             const int32_t* ring_table_dev, void* stream);

/* Backward of the HEALPix padding and of HEALPixLayer(Conv2d 3x3) (the reference lines differentiated: utils/healpix.py:69-114
 * and :165-368).  The adjoint of the padding table is handed over as a CSR over the 12*H*W source cells of one sample
 * (healpix.pad_adjoint_table): adj_indptr_dev [12*H*W + 1], adj_index_dev [nnz] padded positions face*(H+2p)*(W+2p) + pixel
 * of the padded face, adj_weight_dev [nnz] 1 or 0.5 (a synthesised corner is the mean of two cells).  Both kernels gather
 * through it: every element of dx_dev is written once, no atomics, bitwise reproducible; dx_dev may not alias dy_dev.
 * Faces are square; n_faces a multiple of 12 and at most 65535 (DLWP_ERR_UNSUPPORTED above).
 *   dlwp_healpix_pad_bwd_f32: the adjoint of dlwp_healpix_pad_f32 for every pad it takes (1 <= pad <= H):
 *   dy_dev [n_faces, C, H+2p, W+2p] -> dx_dev [n_faces, C, H, W], dx[s] = sum over the entries of s of weight * dy[q].
 *   dlwp_conv3x3_hpx_bwd_data_f32: the gradient of HEALPixPadding(1) + Conv2d(3x3, padding 0) with respect to its input:
 *   dy_dev [n_faces, cout, H, W] (the gradient of the convolution's output), weight_dev [cout, cin, 3, 3] in the forward
 *   layout (flipped and transposed as it is loaded) -> dx_dev [n_faces, cin, H, W]; the adjoint table of pad 1.  Any channel
 *   counts (cin up to 65535).  Two launches on `stream`: the transposed 3x3 at the halo positions of every face into the
 *   workspace (a ring of 2 (W+2) + 2 H cells per face and channel), then the interior transposed 3x3 plus, on face borders,
 *   the ring values of the neighbouring faces through the adjoint table.
 *   dlwp_conv3x3_hpx_bwd_data_workspace_bytes: n_faces * cin * (2 (W+2) + 2 H) floats (0 for a non-positive size); a
 *   smaller workspace returns DLWP_ERR_WORKSPACE. */
size_t dlwp_conv3x3_hpx_bwd_data_workspace_bytes(int32_t n_faces, int32_t height, int32_t width, int32_t cin);
int32_t dlwp_healpix_pad_bwd_f32(const float* dy_dev, float* dx_dev, const int32_t* adj_indptr_dev,
                                 const int32_t* adj_index_dev, const float* adj_weight_dev, int32_t n_faces,
                                 int32_t channels, int32_t height, int32_t width, int32_t pad, void* stream);
int32_t dlwp_conv3x3_hpx_bwd_data_f32(const float* dy_dev, const float* weight_dev, float* dx_dev, int32_t n_faces,
                                      int32_t height, int32_t width, int32_t cin, int32_t cout,
                                      const int32_t* adj_indptr_dev, const int32_t* adj_index_dev,
                                      const float* adj_weight_dev, void* workspace, size_t workspace_bytes,
                                      void* stream);

/* HEALPix -> lat-lon remap of rollouts for scoring (csrc/healpix_remap.hip).  Replaces reference scripts/evaluate.py:79-116
 * (`HEALPixRemap.hpx2ll`, data/processing/healpix_mapping.py:372-404, once per (sample, step, variable) plane in a pool of host
 * processes: a Python loop over the pixels plus reproject's bilinear interpolation), as called at evaluate.py:298-303 and
 * scripts/train.py:430-441.  The geometry is handed over as a table of four taps per lat-lon cell (healpix.latlon_table: the
 * HEALPix library's bilinear interpolation in the reference's face layout, weights rounded once from float64):
 *   x_dev [planes, 12 * nside^2] (a plane = one [12, nside, nside] field), index_dev int32 [cells, 4] with every entry in
 *   0 .. 12 nside^2 - 1 (checked by the host builder, NOT here), weight_dev float [cells, 4], both 16-byte aligned,
 *   y_dev [planes, cells]:  y[p][q] = ((w0 x[p][i0] + w1 x[p][i1]) + w2 x[p][i2]) + w3 x[p][i3] in fp32, in this order; a tap
 *   of weight zero is still read (a NaN there gives NaN, as in numpy).
 * Any planes >= 1 (64-bit; planes sit on the 31-bit grid axis, DLWP_ERR_UNSUPPORTED beyond it) and any cells >= 1.  One launch
 * on `stream`, no host synchronisation, no atomics; y_dev may not alias x_dev. */
int32_t dlwp_healpix_to_latlon_f32(const float* x_dev, const int32_t* index_dev, const float* weight_dev, float* y_dev,
                                   int64_t planes, int32_t nside, int32_t cells, void* stream);

/* Weight and bias gradient of pad(1) + Conv2d(3x3, padding 0) on cat([x0, x1], 1), either padding rule (csrc/conv_wgrad.hip;
 * the reference lines differentiated: scripts/train.py:271 through models/unet/unet.py:456-470, :512-525, :886,
 * models/convlstm/convlstm.py:94, :148-157, utils/healpix.py:69-114):
 *   dw[co][ci][ky][kx] = sum_{b,y,x} dz[b][co][y][x] * P(act_pre(xcat))[b][ci][y+ky][x+kx],   db[co] = sum_{b,y,x} dz[b][co][y][x]
 * x0_dev, c0, x1_dev, c1, pre_act and ring_table as dlwp_conv3x3_ex_f32 (ring_table NULL: CylinderPad, else the HEALPix halo
 * table with batch = 12 * samples faces): the padded, pre-activated input is read the way the forward reads it, no cat, activated
 * or padded copy is made.  dz_dev [batch, cout, H, W] is the gradient of the convolution's output (after the post-activation
 * derivative); dw_dev [cout, c0+c1, 3, 3]; db_dev [cout] or NULL.  Exact-fp32 matrix instructions (an fmaf chain per element).
 * Two launches on `stream`: partial sums of the K-slices (runs of consecutive 8 x 8 pixel tiles) into the workspace, then their
 * sum in slice order.  One writer per element, no atomics, a slice count that depends on the shape arguments only: results are
 * bit-identical from run to run.  No pointer needs more than 4-byte alignment.
 * Envelope: c0 >= 1, c1 >= 0, cout >= 1, c0 + c1 and cout up to 1024, any H, W >= 1, per-sample offsets (channels * H * W)
 * within 32 bits, HEALPix batches a multiple of 12; anything else returns DLWP_ERR_UNSUPPORTED before any launch.
 *   dlwp_conv3x3_wgrad_workspace_bytes: slices * (cout * cin * 9 + cout) floats, cin = c0 + c1 (0 = unsupported shape); a
 *   smaller workspace returns DLWP_ERR_WORKSPACE.
 *   dlwp_conv3x3_wgrad_slices: the K-slices the launcher takes (0 = unsupported shape).  For tests and tools. */
size_t dlwp_conv3x3_wgrad_workspace_bytes(int32_t batch, int32_t height, int32_t width, int32_t cin, int32_t cout);
int32_t dlwp_conv3x3_wgrad_slices(int32_t batch, int32_t height, int32_t width, int32_t cin, int32_t cout);
int32_t dlwp_conv3x3_wgrad_f32(const float* x0_dev, int32_t c0, const float* x1_dev, int32_t c1, const float* dz_dev,
                               float* dw_dev, float* db_dev, int32_t batch, int32_t height, int32_t width, int32_t cout,
                               int32_t pre_act, const int32_t* ring_table, void* workspace, size_t workspace_bytes,
                               void* stream);

/* Weight and bias gradient of the zero-padded Conv2d (dlwp_conv2d_f32's layer) and of ConvTranspose2d (dlwp_conv_transpose2d_f32's,
 * output_padding 0) with a square k x k kernel (csrc/conv_wgrad.hip; the reference lines differentiated: scripts/train.py:271
 * through models/unet/unet.py:450, :583-584, :879 (Conv2d 1x1, 3x3 stride 2) and :523, :719 (ConvTranspose2d 2x2 s2, 4x4 s2 p1)):
 *   transposed == 0: dw[co][ci][ky][kx] = sum_{b,i,j} dz[b][co][i][j] * act_pre(x)[b][ci][i s - p + ky][j s - p + kx]
 *   transposed != 0: dw[ci][co][ky][kx] = sum_{b,i,j} x[b][ci][i][j] * dz[b][co][i s - p + ky][j s - p + kx]
 *   db[co] = sum_{b,y,x} dz[b][co][y][x]
 * with the map under the taps zero outside its bounds: one kernel, the two maps exchanging roles.  x_dev [batch, cin, H, W] is
 * the layer's input, read where it lies with pre_act (the codes of dlwp_conv2d_f32; 0 for the transposed layer) applied at
 * load; dz_dev [batch, cout, OH, OW] the gradient of the layer's output before its activation, OH = (H + 2p - k) / s + 1
 * (Conv2d, rounded down: trailing rows / columns of x that no output reads are skipped) or (H - 1) s - 2p + k (transposed).
 * dw_dev in torch's layout ([cout, cin, k, k], transposed [cin, cout, k, k]) or NULL; db_dev [cout] or NULL.  No padded,
 * activated, unfolded or zero-stuffed copy is made.  Exact-fp32 matrix instructions (an fmaf chain per element).  Two launches
 * on `stream`: partial sums of the K-slices (runs of consecutive pixel tiles of the smaller map) into the workspace, then their
 * sum in slice order.  One writer per element, no atomics, a slice count that depends on the shape arguments only: results are
 * bit-identical from run to run.  No pointer needs more than 4-byte alignment.
 * Envelope: k 1..4, stride 1 or 2, 0 <= pad < k, cin and cout 1..1024, any H, W >= 1 that leave OH, OW >= 1, per-sample offsets
 * (channels * map) within 32 bits; anything else returns DLWP_ERR_UNSUPPORTED before any launch.
 *   dlwp_conv2d_wgrad_workspace_bytes: slices * (cout * cin * k * k + cout) floats (0 = unsupported shape); a smaller workspace
 *   returns DLWP_ERR_WORKSPACE.
 *   dlwp_conv2d_wgrad_slices: the K-slices the launcher takes (0 = unsupported shape).  For tests and tools. */
size_t dlwp_conv2d_wgrad_workspace_bytes(int32_t batch, int32_t cin, int32_t height, int32_t width, int32_t cout, int32_t k,
                                         int32_t stride, int32_t pad, int32_t transposed);
int32_t dlwp_conv2d_wgrad_slices(int32_t batch, int32_t cin, int32_t height, int32_t width, int32_t cout, int32_t k,
                                 int32_t stride, int32_t pad, int32_t transposed);
int32_t dlwp_conv2d_wgrad_f32(const float* x_dev, const float* dz_dev, float* dw_dev, float* db_dev, int32_t batch, int32_t cin,
                              int32_t height, int32_t width, int32_t cout, int32_t k, int32_t stride, int32_t pad,
                              int32_t pre_act, int32_t transposed, void* workspace, size_t workspace_bytes, void* stream);

/* ConvLSTM cell gate math (models/convlstm/convlstm.py:96-109): gates_dev [B, 4*hidden, H, W] in the
 * order (netin, igate, fgate, ogate), c_prev_dev [B, hidden, H, W] -> h_out_dev, c_out_dev. */
int32_t dlwp_convlstm_gates_f32(const float* gates_dev, const float* c_prev_dev, float* h_out_dev,
                                float* c_out_dev, int32_t batch, int32_t hidden, int32_t height,
                                int32_t width, void* stream);

/* Backward of dlwp_convlstm_gates_f32 (csrc/convlstm_bwd.hip; the forward it differentiates: models/convlstm/convlstm.py:96-109,
 * under scripts/train.py:271).  From the forward's INPUTS alone -- gates_dev [B, 4*hidden, H, W] (netin, igate, fgate, ogate,
 * pre-activation) and c_prev_dev [B, hidden, H, W]; the activations, c and tanh(c) are recomputed with the forward's arithmetic:
 *   si, sf, so = sigma(i), sigma(f), sigma(o)     tn = tanh(netin)     c = sf c_prev + si tn     tc = tanh(c)
 *   dct = dc + dh so (1 - tc^2)
 *   d_o = dh tc so (1 - so)     d_f = dct c_prev sf (1 - sf)     d_i = dct tn si (1 - si)     d_netin = dct si (1 - tn^2)
 *   dc_prev = dct sf
 * dh_dev, dc_dev [B, hidden, H, W]: the gradients of h_out and c_out; either may be NULL (a zero gradient, not read; results are
 * those of a zero tensor bit for bit), both NULL is DLWP_ERR_INVALID_ARGUMENT.  dgates_dev [B, 4*hidden, H, W]: every element
 * written; dc_prev_dev [B, hidden, H, W] or NULL (not wanted, not stored).  Outputs may not alias inputs or each other.  One
 * launch on `stream`, one writer per element, no atomics, no workspace: reruns are bitwise identical. */
int32_t dlwp_convlstm_gates_bwd_f32(const float* gates_dev, const float* c_prev_dev, const float* dh_dev, const float* dc_dev,
                                    float* dgates_dev, float* dc_prev_dev, int32_t batch, int32_t hidden, int32_t height,
                                    int32_t width, void* stream);

/* LayerNorm over the last dimension of a token-major tensor x_dev [rows, channels] (channels % 4 == 0,
 * <= 2048): y = (x - mean) * rsqrt(var + eps) * gamma + beta, biased variance (torch.nn.LayerNorm).
 * Reference call sites: models/fourcastnet/fourcastnet.py:180-193, models/swintransformer/
 * swin_transformer.py:213,262,304,440,664, models/panguweather/panguweather.py:73,127,281,321. */
int32_t dlwp_layernorm_f32(const float* x_dev, const float* gamma_dev, const float* beta_dev, float* y_dev,
                           int64_t rows, int32_t channels, float eps, void* stream);
/* y = LayerNorm(x + pre_bias): pre_bias_dev [channels] (or NULL) is added before the statistics.  Lets the transformer
 * blocks (swin_transformer.py:254-262, panguweather.py:318-322: `x = shortcut + proj(attn)`, `x = x + mlp(norm2(x))`) run
 * their residual adds as the beta = 1 accumulation of the proj / fc2 GEMMs, in place on x, with the Linear biases
 * carried as ONE pending per-channel vector that only the LayerNorms (here) and the end of the layer ever apply. */
int32_t dlwp_layernorm_prebias_f32(const float* x_dev, const float* pre_bias_dev, const float* gamma_dev,
                                   const float* beta_dev, float* y_dev, int64_t rows, int32_t channels, float eps,
                                   void* stream);
/* The same LayerNorm with a bf16 result (y_bf16_dev [rows][channels], round to nearest even): the input of a bf16-form Linear
 * (dlwp_linear_bf16_io with x_is_bf16), which would round the fp32 result the same way -- bit-identical, half the bytes. */
int32_t dlwp_layernorm_prebias_bf16out(const float* x_dev, const float* pre_bias_dev, const float* gamma_dev,
                                       const float* beta_dev, void* y_bf16_dev, int64_t rows, int32_t channels, float eps,
                                       void* stream);

/* LayerNorm for training (csrc/layernorm_bwd.hip): the `loss.backward()` of scripts/train.py:271 through the nn.LayerNorm
 * layers above (fourcastnet.py:180-193, swin_transformer.py:213,262, panguweather.py:281,321).  For y = LayerNorm(x) gamma + beta
 * over the last dimension, x_dev and gy_dev [rows, channels], with xh = (x - mean) rstd and g = gy gamma:
 *   dx = rstd (g - mean_C(g) - xh mean_C(g xh)),  dgamma_c = sum_rows gy xh,  dbeta_c = sum_rows gy.
 * mean and rstd are recomputed from x with the forward's own arithmetic: a training step keeps x and gamma only, and one
 * pass reads x and gy once and writes dx once.  dx_dev, dgamma_dev, dbeta_dev may each be NULL (not wanted, not computed;
 * without dgamma / dbeta there is one launch and no workspace).  The row sums run in a fixed order with one writer per
 * element (no atomics): reruns are bitwise identical.  The envelope is the forward's (channels % 4 == 0, <= 2048, 64-bit row
 * offsets) with x_dev, gamma_dev, gy_dev, dx_dev and workspace_dev 16-byte aligned; anything else returns
 * DLWP_ERR_UNSUPPORTED before any launch, a smaller workspace DLWP_ERR_WORKSPACE.  No pre_bias form (inference only).
 *   dlwp_layernorm_bwd_partials: the number of partial sums per channel the first launch leaves for the fixed-order sum
 *     (one launch up to 32 partials, two above), a function of (rows, channels) alone, at most 2048 (0 outside the envelope).
 *   dlwp_layernorm_bwd_workspace_bytes: 2 * (partials + 32 above 32 partials) * channels floats, at most 4.5 MB (0 outside the
 *     envelope). */
int32_t dlwp_layernorm_bwd_partials(int64_t rows, int32_t channels);
size_t dlwp_layernorm_bwd_workspace_bytes(int64_t rows, int32_t channels);
int32_t dlwp_layernorm_bwd_f32(const float* x_dev, const float* gamma_dev, const float* gy_dev, float* dx_dev, float* dgamma_dev,
                               float* dbeta_dev, void* workspace_dev, size_t workspace_bytes, int64_t rows, int32_t channels,
                               float eps, void* stream);

/* The pointwise part of a Linear's training step (csrc/bias_act.hip): bias, activation and their gradients around the GEMMs of
 * dlwp_linear_f32, for the nn.Linear layers of swin_transformer.py:21-39, :107-120, panguweather.py:176-211 and
 * fourcastnet.py:40-53 under scripts/train.py:271.  Activation codes as for the convolutions (0 none, 1 exact-erf GELU,
 * 2 tanh, 3 ReLU, 4 SiLU); sizes multiples of 4 and 16-byte aligned tensors, otherwise DLWP_ERR_UNSUPPORTED.
 *   dlwp_act_f32: h = act(z) over n values, with the arithmetic of the dlwp_linear_f32 epilogue (h is bit for bit what the
 *     fused inference call stores).
 *   dlwp_bias_act_bwd_f32: gz = gy act'(z) and db_n = sum_rows gz in one pass over gy_dev, z_dev [rows, n].  act == 0 reads
 *     neither z_dev nor gz_dev (both may be NULL) and only sums; gz_dev may be gy_dev; db_dev may be NULL (then no
 *     workspace).  The column sum has a fixed order and one writer: reruns are bitwise identical.
 *   dlwp_bias_act_bwd_workspace_bytes: the partial column sums (at most 272 * n floats; 0 for a size outside the envelope). */
int32_t dlwp_act_f32(const float* z_dev, float* h_dev, int64_t n, int32_t act, void* stream);
size_t dlwp_bias_act_bwd_workspace_bytes(int64_t rows, int32_t n);
int32_t dlwp_bias_act_bwd_f32(const float* gy_dev, const float* z_dev, float* gz_dev, float* db_dev, void* workspace_dev,
                              size_t workspace_bytes, int64_t rows, int32_t n, int32_t act, void* stream);

/* FourCastNet block glue fused with the layout change the FFT needs (models/fourcastnet/fourcastnet.py
 * :180-193 around AFNO2D :78-127).  x is token-major [B, tokens, C] ("NHWC"), y / f / l channel-major
 * [B, C, tokens] ("NCHW"); C % 4 == 0, C <= 256.
 *   dlwp_layernorm_nhwc_to_nchw_f32: y = LayerNorm1(x), written channel-major (:182 norm1 + the transpose
 *       torch.fft.rfft2(dim=(1,2)) would otherwise do with a strided copy)
 *   dlwp_afno_merge_f32: sum = f + l + x  (irfft2 output + AFNO2D "+ bias" :127 + first skip :187),
 *       norm = LayerNorm2(sum) (:191); both token-major.  sum_bias_dev [C] or NULL is added to the STORED sum only:
 *       the host passes mlp.fc2.bias so that `mlp(norm) + sum` (:192) becomes one GEMM with beta = 1.
 *       norm_nhwc_dev NULL (then gamma / beta may be NULL too): only the sum is produced -- for callers whose next
 *       kernel normalises on the fly (dlwp_token_mlp_f32 with ln_eps >= 0). */
int32_t dlwp_layernorm_nhwc_to_nchw_f32(const float* x_dev, const float* gamma_dev, const float* beta_dev,
                                        float* y_dev, int32_t batch, int64_t tokens, int32_t channels, float eps,
                                        void* stream);
int32_t dlwp_afno_merge_f32(const float* f_nchw_dev, const float* l_nchw_dev, const float* x_nhwc_dev,
                            const float* gamma_dev, const float* beta_dev, const float* sum_bias_dev,
                            float* sum_nhwc_dev, float* norm_nhwc_dev, int32_t batch, int64_t tokens, int32_t channels, float eps,
                            void* stream);

/* Patch embedding for 1x1 patches + position embedding (reference fourcastnet.py:530-543 `PatchEmbed` =
 * Conv2d(kernel = stride = patch) -> flatten(2).transpose(1, 2), and `x + pos_embed` at :286-288) in one pass:
 *   out[b][t][c] = bias[c] + pos[t][c] + sum_ci w[c][ci] x[b][ci][t]
 * x_dev [batch][in_channels][tokens] (NCHW with tokens = H*W), w_dev [channels][in_channels] (the conv weight with its
 * 1x1 kernel dims dropped), bias_dev [channels] or NULL, pos_dev [tokens][channels] or NULL, out_dev token-major.
 * in_channels <= 32, channels a power of two in [4, 256]; other shapes: DLWP_ERR_UNSUPPORTED. */
int32_t dlwp_patch_embed_1x1_f32(const float* x_dev, const float* w_dev, const float* bias_dev, const float* pos_dev,
                                 float* out_dev, int32_t batch, int32_t in_channels, int64_t tokens, int32_t channels,
                                 void* stream);

/* Head of a 1x1-patch token backbone (reference fourcastnet.py:144 `head = nn.Linear(embed_dim, out_chans * p1 * p2, bias=False)`, applied
 * at :296-303 with the rearrange "b h w (p1 p2 c_out) -> b c_out (h p1) (w p2)"; p1 = p2 = 1):
 *   out[b][co][t] = bias[co] + sum_c w[co][c] tokens[b][t][c]
 * tokens_dev [batch][tokens][channels] token-major, w_dev [out_channels][channels], bias_dev [out_channels] or NULL, out_dev
 * [batch][out_channels][tokens] channels-first (NCHW with tokens = H*W).  channels a multiple of 4, <= 256; out_channels <= 16. */
int32_t dlwp_patch_recover_1x1_f32(const float* tokens_dev, const float* w_dev, const float* bias_dev, float* out_dev,
                                   int32_t batch, int64_t tokens, int32_t channels, int32_t out_channels, void* stream);

/* `_prepare_inputs` of the rollout loop (reference swin_transformer.py:679-692 and its copies in fno.py:49-62, fourcastnet.py:294-307,
 * panguweather.py:442-455, unet.py:316-329): cat([constants[:, 0], prescribed window, prognostic window], dim = 1).  n_segments <= 8 blocks
 * [batch][seg_channels[i]][plane] whose samples lie seg_batch_strides[i] floats apart (views into the inputs / the trajectory buffer) are
 * copied into out_dev [batch][sum channels][plane], contiguous.  The three arrays are HOST arrays; plane a multiple of 4, 16-byte alignment. */
int32_t dlwp_concat_channels_f32(const float* const* seg_dev_ptrs, const int32_t* seg_channels, const int64_t* seg_batch_strides,
                                 int32_t n_segments, float* out_dev, int32_t batch, int64_t plane, void* stream);

/* Token MLP of the AFNO block (reference fourcastnet.py:41-57 `Mlp` = fc1 -> GELU -> fc2, called at :191-192 as
 * `x = mlp(norm2(x)) + residual`):  out[t] = resid[t] + b2 + W2 gelu(W1 n[t] + b1), all token-major [tokens][channels].
 * One launch; the [tokens][hidden] activation never reaches memory (both GEMMs on the bf16 matrix pipe as six-term
 * exact splits = fp32-GEMM accuracy).  channels == 64, hidden % 64 == 0, hidden <= 256 (weights are LDS resident);
 * anything else returns DLWP_ERR_UNSUPPORTED and the caller keeps its GEMM path.
 *   dlwp_token_mlp_packed_bytes: size of the packed-weight buffer (0 if the shape is unsupported)
 *   dlwp_token_mlp_pack_f32:     w1_dev [hidden][channels] (fc1.weight), w2_dev [channels][hidden] (fc2.weight) -> packed.
 *                                With ln_gamma_dev / ln_beta_dev [channels] (both or neither) the affine part of the
 *                                LayerNorm in front of fc1 (`norm2`, :191) is folded in: W1 diag(gamma), and
 *                                b1 + W1 beta (b1_dev [hidden] or NULL) is stored in the packed buffer.
 *                                merged_layout != 0: the k-slot order dlwp_afno_block_tail_f32 wants (below).
 *   dlwp_token_mlp_f32:          ln_eps < 0: n_dev is the fc1 input, b1_dev required.  ln_eps >= 0: n_dev is the
 *                                UN-normalised token (normally the same buffer as resid_dev); the kernel normalises
 *                                it (two-pass statistics over the channels) and takes b1 from a buffer packed WITH
 *                                gamma / beta (b1_dev ignored).  resid_dev, b2_dev may be NULL; out_dev may alias
 *                                resid_dev / n_dev (a wave reads all it needs of its 32 tokens before it writes). */
size_t dlwp_token_mlp_packed_bytes(int32_t channels, int32_t hidden);
int32_t dlwp_token_mlp_pack_f32(const float* w1_dev, const float* w2_dev, const float* ln_gamma_dev,
                                const float* ln_beta_dev, const float* b1_dev, int32_t channels, int32_t hidden,
                                int32_t merged_layout, void* packed_dev, void* stream);
int32_t dlwp_token_mlp_f32(const float* n_dev, const float* resid_dev, const void* packed_dev, const float* b1_dev,
                           const float* b2_dev, float* out_dev, int64_t tokens, int32_t channels, int32_t hidden,
                           float ln_eps, void* stream);
/* dlwp_token_mlp_f32 that ALSO emits next = LayerNorm(out; next_gamma, next_beta, next_eps) CHANNELS-FIRST,
 * next_cf_dev [tokens / tokens_per_sample][channels][tokens_per_sample]: what the following AFNO block computes first
 * (`norm1`, fourcastnet.py:182, + the layout rfft2 wants), taken from the accumulators instead of a separate pass over
 * `out`.  tokens_per_sample % 32 == 0 and tokens % tokens_per_sample == 0, else DLWP_ERR_UNSUPPORTED. */
int32_t dlwp_token_mlp_emit_norm_f32(const float* n_dev, const float* resid_dev, const void* packed_dev,
                                     const float* b1_dev, const float* b2_dev, float* out_dev, int64_t tokens,
                                     int32_t channels, int32_t hidden, float ln_eps, const float* next_gamma_dev,
                                     const float* next_beta_dev, float next_eps, float* next_cf_dev,
                                     int64_t tokens_per_sample, void* stream);

/* The whole tail of an AFNO block in ONE launch (reference fourcastnet.py:127 `+ bias`, :187 first skip, :191 `norm2`,
 * :41-57 `Mlp`, :192 second skip -- and, optionally, :182 `norm1` of the NEXT block):
 *   sum = f_cf + l_cf + x;  out = sum + b2 + W2 gelu(W1 LayerNorm(sum) + b1);  next_cf = LayerNorm_next(out) channels-first
 * f_cf_dev (irfft2 output) and l_cf_dev (norm1 output, the AFNO2D `bias` path) CHANNELS-FIRST [batch][channels][tokens_per_sample],
 * x_nhwc_dev / out_nhwc_dev token-major (may alias), packed_dev from dlwp_token_mlp_pack_f32 WITH ln_gamma / ln_beta and
 * merged_layout = 1, next_cf_dev (and its gamma / beta) NULL to skip the last part.  Replaces dlwp_afno_merge_f32 +
 * dlwp_token_mlp_f32 (+ dlwp_layernorm_nhwc_to_nchw_f32 of the next block).  channels == 64, tokens_per_sample % 32 == 0. */
int32_t dlwp_afno_block_tail_f32(const float* f_cf_dev, const float* l_cf_dev, const float* x_nhwc_dev,
                                 const void* packed_dev, const float* b2_dev, float* out_nhwc_dev, int32_t batch,
                                 int64_t tokens_per_sample, int32_t channels, int32_t hidden, float ln_eps,
                                 const float* next_gamma_dev, const float* next_beta_dev, float next_eps,
                                 float* next_cf_dev, void* stream);
/* The same block tail in the "f16x3" product form (exact two-part f16 splits of both operands, three products on the f16
 * matrix instructions instead of six bf16 ones; both weight images fit the LDS, nothing is re-read from global memory).
 * packed_dev from dlwp_token_mlp_pack_f16x3 (same arguments and byte count as dlwp_token_mlp_pack_f32).  fp32-GEMM
 * accuracy; its operands are LayerNorm and GELU outputs, orders of magnitude inside the f16 range. */
int32_t dlwp_token_mlp_pack_f16x3(const float* w1_dev, const float* w2_dev, const float* ln_gamma_dev,
                                  const float* ln_beta_dev, const float* b1_dev, int32_t channels, int32_t hidden,
                                  int32_t merged_layout, void* packed_dev, void* stream);
int32_t dlwp_afno_block_tail_f16x3(const float* f_cf_dev, const float* l_cf_dev, const float* x_nhwc_dev,
                                   const void* packed_dev, const float* b2_dev, float* out_nhwc_dev, int32_t batch,
                                   int64_t tokens_per_sample, int32_t channels, int32_t hidden, float ln_eps,
                                   const float* next_gamma_dev, const float* next_beta_dev, float next_eps,
                                   float* next_cf_dev, void* stream);

/* On-device evaluation sums (reference scripts/evaluate.py:786-821 `compute_metrics` + the
 * de-normalisation of :281-296): out_dev, target_dev [B, K, C, H, W]; climatology_dev [K, C, H, W] or NULL;
 * lat_weights_dev [H] (cos(lat)/mean(cos(lat))); scale_dev [C] (per-variable std) or NULL.
 * sums_dev: double [4, K, C], zeroed by the call:  0: sum w (s (out-tar))^2,  1: sum w s^2 (out-clim)(tar-clim),
 * 2: sum w (s (out-clim))^2,  3: sum w (s (tar-clim))^2  (1-3 only with a climatology).
 * RMSE[k,c] = sqrt(sums[0] / (B_total H W)),  ACC = sums[1] / sqrt(sums[2] sums[3]). */
int32_t dlwp_weighted_error_sums_f32(const float* out_dev, const float* target_dev, const float* climatology_dev,
                                     const float* lat_weights_dev, const float* scale_dev, double* sums_dev,
                                     int32_t batch, int32_t steps, int32_t channels, int32_t height, int32_t width,
                                     void* stream);
/* The same sums ADDED to the contents of sums_dev (the running sums of an evaluation over many batches: evaluate.py:786-821
 * accumulates before it takes the root); the caller zeroes sums_dev once. */
int32_t dlwp_weighted_error_sums_acc_f32(const float* out_dev, const float* target_dev, const float* climatology_dev,
                                         const float* lat_weights_dev, const float* scale_dev, double* sums_dev,
                                         int32_t batch, int32_t steps, int32_t channels, int32_t height, int32_t width,
                                         void* stream);

/* On-device zonal energy spectrum sums (reference scripts/losses.py:16-152 `ZonalSpectrum` / `MELRCalculator`):
 * out_dev, target_dev [B, K, C, H, W] fp32, contiguous, 16-byte aligned; circumference_dev double [H] (circ_h =
 * cos(lat_h) 2 pi R, losses.py:20-23).  For every row, F = rfft(norm='forward') over W and P[m] = |F[m]|^2 (doubled for
 * m > 0, the Nyquist bin included; losses.py:39-43).  sums_dev: double [2, K, C, W/2 + 1], written by the call:
 *   0: sum_{b,h} circ_h P_out,  1: the same for target.
 * E = sums / (B_total H) (losses.py:107-108); log ratio ln((E_0 + 1e-10) / (E_1 + 1e-10)) and its mean over m (MELR,
 * :117-121) are left to the caller.  W a power of two from 32 to 512 (else DLWP_ERR_UNSUPPORTED), any H, K C <= 65535.
 * fp32 transforms, fp64 weights and sums; fixed-order reduction through the workspace (no atomics: bitwise reproducible),
 * two launches on `stream`, no host synchronisation.
 *   dlwp_zonal_power_workspace_bytes: the per-workgroup partials (0 for an unsupported shape); a smaller workspace
 *   returns DLWP_ERR_WORKSPACE. */
size_t dlwp_zonal_power_workspace_bytes(int32_t batch, int32_t steps, int32_t channels, int32_t height, int32_t width);
int32_t dlwp_zonal_power_sums_f32(const float* out_dev, const float* target_dev, const double* circumference_dev,
                                  double* sums_dev, int32_t batch, int32_t steps, int32_t channels, int32_t height,
                                  int32_t width, void* workspace_dev, size_t workspace_bytes, void* stream);
/* The same sums ADDED to the contents of sums_dev (running sums over the batches of an evaluation). */
int32_t dlwp_zonal_power_sums_acc_f32(const float* out_dev, const float* target_dev, const double* circumference_dev,
                                      double* sums_dev, int32_t batch, int32_t steps, int32_t channels, int32_t height,
                                      int32_t width, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Climate sums of a rollout chunk (csrc/climate_sums.hip): the reductions over lead time of the reference's physical-soundness
 * scores (scripts/evaluate.py:832-872).  out_dev, target_dev [B, K, C, H, W] fp32, contiguous: K consecutive rollout steps.
 *   zonal_dev  double [2, B, C, H]:    += sum over the chunk's steps and the W longitudes   (0 = out, 1 = target; :839-840)
 *   window_dev double [2, B, C, H, W]: += sum over steps [win_begin, win_end) of THIS chunk (:868-869); may be null
 * Both are RUNNING sums the caller zeroes once and divides at the end.  0 <= win_begin <= win_end <= K (an empty window leaves
 * window_dev untouched), every dimension >= 1, else DLWP_ERR_INVALID_ARGUMENT; no limit on B C H, any W (16-byte loads where
 * W % 4 == 0 and out / target are 16-byte aligned, 4-byte loads of the same elements otherwise).  Every add is fp64 from the
 * first one; one lane group owns a row (b, c, h) for the whole call and adds in an order fixed by W alone, no atomics: the sums
 * of a horizon are bit-identical however it is cut into chunks.  out and target are read once.  One launch on `stream`. */
int32_t dlwp_climate_sums_acc_f32(const float* out_dev, const float* target_dev, double* zonal_dev, double* window_dev,
                                  int32_t batch, int32_t steps, int32_t channels, int32_t height, int32_t width,
                                  int32_t win_begin, int32_t win_end, void* stream);

/* Ensemble scores of a forecast chunk (csrc/ensemble_scores.hip; the reference: only the commented sketch of
 * scripts/train.py:352-371 -- the definitions are the usual ensemble-verification forms).  ens_dev is
 * `members` planes [B, K, C, H, W] fp32, member_stride elements apart (at least one plane: a group view of a wider buffer
 * works); target_dev [B, K, C, H, W]; lat_weights_dev [H]; scale_or_null_dev [C].  With x_(0) <= ... <= x_(M-1) the members at
 * a grid point, y the target, w the row's weight and s the variable's scale (1 when null) the call ADDS, for the steps
 * k' = step_begin + k of sums_dev double [4][steps_total][C] and ranks_dev int64 [steps_total][C][M + 1]:
 *   sums[0] += sum w (s (mean_m x_m - y))^2               sums[1] += sum w s^2 1/(M-1) sum_m (x_m - mean)^2   (two-pass)
 *   sums[2] += sum w s 1/M sum_m |x_m - y|                sums[3] += sum w s sum_{i<j} |x_i - x_j|            (unnormalised)
 *   ranks[..][r] += 1 with r = #{m : x_m < y}             (strict, unweighted)
 * Per-point arithmetic is fp32, every accumulation across points fp64 in a fixed order (per-workgroup partials in
 * workspace_dev, then one ordered sum per (k, c)): no floating-point atomics, two runs give the same bits; the rank counts are
 * integer atomics.  NaNs are not treated.  2 <= members <= 64 (any value, chosen at run time), else DLWP_ERR_UNSUPPORTED;
 * steps * channels and batch at most 65535.  Every member value is read once; nothing but the partials is written.
 * dlwp_ensemble_sums_workspace_bytes: the size of the partials (0 for a bad shape); a smaller workspace is DLWP_ERR_WORKSPACE.
 * No allocation, no synchronisation. */
size_t dlwp_ensemble_sums_workspace_bytes(int32_t batch, int32_t steps, int32_t channels, int32_t height, int32_t width);
int32_t dlwp_ensemble_sums_acc_f32(const float* ens_dev, const float* target_dev, const float* lat_weights_dev,
                                   const float* scale_or_null_dev, double* sums_dev, int64_t* ranks_dev, int32_t members,
                                   int64_t member_stride, int32_t batch, int32_t steps, int32_t channels, int32_t height,
                                   int32_t width, int32_t steps_total, int32_t step_begin, void* workspace_dev,
                                   size_t workspace_bytes, void* stream);

/* Top-of-atmosphere insolation on the device (csrc/insolation.hip; reference data/datasets/add_insolation.py:9-73):
 *   out[t, p] = fp32(S (sin lat_p sin dec_t - cos lat_p cos dec_t cos h) rho_t^-2),  cos h = cd_t cl_p - sd_t sl_p
 * date_table_dev double [dates, 5] = { sin dec, cos dec, rho^-2, cd = cos 2 pi frac(day), sd = sin 2 pi frac(day) },
 * point_table_dev double [points, 4] = { sin lat, cos lat, cl = cos 2 pi lon/360, sl = sin 2 pi lon/360 } (lon / 360 taken in
 * fp32 as the reference takes it, :54,:62), out_dev fp32 [dates, points].  fp64 FMAs, one rounding; clip_zero != 0 clips
 * negative values (:70-71); normalise != 0 then applies (x - mean) / scale in fp32 (data/datasets/datasets.py:371), scale
 * non-zero.  No device transcendental.  One writer per element. */
int32_t dlwp_insolation_f32(const double* date_table_dev, const double* point_table_dev, float* out_dev, int32_t dates,
                            int64_t points, double solar_constant, int32_t clip_zero, int32_t normalise, float mean, float scale,
                            void* stream);

/* Global multi-head self-attention of the diffusion U-Net's AttentionBlock (reference
 * models/diffusion_models/modern_unet/modern_unet.py:565-571: einsum -> softmax(dim=1) -> einsum, between the `projection`
 * and `output` Linears), fp32-accurate (v_mfma_f32_16x16x4_f32), with no N x N tensor anywhere.
 * qkv_dev [batch, tokens, heads, 3, head_dim] (the projection output viewed [B, N, heads, 3 d_k] and chunked in three);
 * out_dev [batch, tokens, heads * head_dim].  The softmax runs over the QUERY axis, as the reference's dim=1: every key's
 * weights over all queries sum to one.  Two launches on `stream`: per-key log-sum-exp statistics into the workspace, then
 * the output.  Any shape with positive sizes runs; head_dim % 4 == 0 with 16-byte aligned pointers takes 16-byte loads.
 *   dlwp_global_attn_workspace_bytes: batch * heads * tokens floats (0 for a non-positive size)
 * After the call the workspace holds the per-key statistics [batch, heads, tokens] in base 2, L_j log2(e) with
 * L_j = m_j + ln sum_i exp(s_ij - m_j): the `stats_dev` of dlwp_global_attn_bwd_f32. */
size_t dlwp_global_attn_workspace_bytes(int32_t batch, int32_t heads, int32_t tokens);
int32_t dlwp_global_attn_f32(const float* qkv_dev, float* out_dev, int32_t batch, int32_t tokens, int32_t heads,
                             int32_t head_dim, float scale, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of dlwp_global_attn_f32: from grad_out_dev [batch, tokens, heads * head_dim] (the gradient of out_dev) and the
 * forward's workspace as it stands (stats_dev, L_j log2(e)), writes dqkv_dev in the layout of qkv_dev
 * [batch, tokens, heads, 3, head_dim] -- every element, so it needs no zeroing -- with the same scale.  fp32-accurate
 * (v_mfma_f32_16x16x4_f32), no N x N tensor, no atomics: bitwise reproducible.  Three launches on `stream` (dV; the per-key
 * delta D_j = v_j . dV_j into the workspace and dK; dQ), no host synchronisation.  head_dim 1 .. 1024 and any positive
 * batch / tokens / heads; head_dim above 1024 returns DLWP_ERR_UNSUPPORTED.  dqkv_dev may not alias an input.
 *   dlwp_global_attn_bwd_workspace_bytes: batch * heads * tokens floats (0 for a non-positive size) */
size_t dlwp_global_attn_bwd_workspace_bytes(int32_t batch, int32_t heads, int32_t tokens);
int32_t dlwp_global_attn_bwd_f32(const float* qkv_dev, const float* grad_out_dev, const float* stats_dev, float* dqkv_dev,
                                 int32_t batch, int32_t tokens, int32_t heads, int32_t head_dim, float scale,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * MeshGraphNet message passing (reference models/mgn/meshgraphnet.py:412-423 `update_nodes_and_edges`, built from
 * models/graphcast/gnn_layers/mesh_graph_mlp.py MeshGraphMLP / MeshGraphEdgeMLPConcat, mesh_edge_block.py,
 * mesh_node_block.py and utils.py concat_message_function :96-111, agg_concat_dgl :340-380)
 * ------------------------------------------------------------------------------------------ */
/* One MeshGraphMLP: n_linear Linears (hidden_layers + 1, 2..5) with ReLU between them, then an optional LayerNorm.
 * dims[0] is the input width, dims[i + 1] the output width of Linear i.  wt[i] is Linear i's weight TRANSPOSED,
 * [dims[i]][dims[i + 1]] row-major (nn.Linear keeps [out][in]); bias[i] has dims[i + 1] values.  ln_gamma / ln_beta:
 * both NULL (no LayerNorm) or both of width dims[n_linear]. */
typedef struct dlwp_mgn_mlp_desc {
  int32_t n_linear;
  int32_t dims[6];
  const float* wt[5];
  const float* bias[5];
  const float* ln_gamma;
  const float* ln_beta;
  float ln_eps;
} dlwp_mgn_mlp_desc;

/* The MLP row by row over batch * rows rows (mesh_graph_mlp.py MeshGraphMLP.default_forward; meshgraphnet.py:418-419 and
 * :422 -- the node / edge encoders and the node decoder).  layout 0: [batch * rows, C] row-major; layout 1: channels-first
 * [batch, C, rows] (the node encoder reads x_t [B, C, H, W] and the decoder writes [B, C, H, W]: the reference's
 * "b d h w -> (b h w) d" rearranges of :480 and :486 without a copy).  Envelope: input width <= 2048, hidden and output
 * widths <= 512; otherwise DLWP_ERR_UNSUPPORTED.  One launch, no atomics (bitwise reproducible). */
int32_t dlwp_mgn_mlp_f32(const dlwp_mgn_mlp_desc* mlp, const float* in_dev, float* out_dev, int32_t batch, int32_t rows,
                         int32_t in_layout, int32_t out_layout, void* stream);

/* One processor layer, MeshEdgeBlock then MeshNodeBlock (meshgraphnet.py:541 pairs them), in ONE launch.  The graph is
 * one graph shared by the batch, in CSC order by destination: row_ptr_dev [n_nodes + 1], src_dev / dst_dev [n_edges];
 * edge i of the CSC order runs src_dev[i] -> dst_dev[i], and dst_dev[i] = n for row_ptr[n] <= i < row_ptr[n + 1].
 *   e'  = LN(edge_mlp([e, x[src], x[dst]])) + e                        (mesh_edge_block.py, concat order utils.py:110)
 *   x'  = LN(node_mlp([agg_{edges into n} e', x])) + x                 (mesh_node_block.py, concat order utils.py:379)
 * aggregation 0 = sum, 1 = mean (a node without incoming edges aggregates to 0).  edge_mlp: 3D -> D, node_mlp: 2D -> D,
 * hidden widths <= D <= 512, both with a LayerNorm; otherwise DLWP_ERR_UNSUPPORTED.  D >= 64 runs the products on
 * v_mfma_f32_16x16x4_f32, narrower layers as fp32 FMA chains; both are fp32-exact products.
 * x_in_dev / x_out_dev: [batch, n_nodes, D] (distinct buffers).  e_in_dev: sample b's edges at e_in_dev + b *
 * e_in_batch_stride (0: one table shared by the batch, the encoded edge features; else n_edges * D); e_out_dev
 * [batch, n_edges, D] may equal e_in_dev when the stride is n_edges * D (each edge is read and written by one workgroup),
 * never when it is 0 (DLWP_ERR_INVALID_ARGUMENT).  Sums run in CSC order,
 * every output has one writer: bitwise reproducible. */
int32_t dlwp_mgn_processor_layer_f32(const dlwp_mgn_mlp_desc* edge_mlp, const dlwp_mgn_mlp_desc* node_mlp,
                                     int32_t aggregation, const int32_t* row_ptr_dev, const int32_t* src_dev,
                                     const int32_t* dst_dev, int32_t n_nodes, int32_t n_edges, int32_t batch, const float* x_in_dev,
                                     float* x_out_dev, const float* e_in_dev, int64_t e_in_batch_stride,
                                     float* e_out_dev, void* stream);

/* MeshGraphNet training (csrc/mgn_bwd.hip): the backward of the two entry points above, which reference
 * scripts/train.py:271 `loss.backward()` reaches through mesh_graph_mlp.py MeshGraphMLP.default_forward, mesh_edge_block.py,
 * mesh_node_block.py and utils.py concat_message_function :96-111 / agg_concat_dgl :340-380.  Nothing of the forward is
 * stored: each launch recomputes the forward of the rows it owns from the saved INPUTS.
 * Parameter gradients are written as one flat fp32 array per MLP, in this order: for each Linear i, its weight gradient
 * TRANSPOSED like wt[i] ([dims[i]][dims[i + 1]]) then its bias gradient (dims[i + 1]); then, with a LayerNorm, the
 * gamma and beta gradients (dims[n_linear] each).
 * Backward envelope: 2..5 Linears, hidden and output widths <= 64, input width <= 256 (the MLP) or 3D / 2D (the layer);
 * otherwise DLWP_ERR_UNSUPPORTED (and the workspace queries return 0).  fp32 FMA chains (exact fp32 products).
 * Parameter gradients: a capped grid of 512 workgroups (two per CU) each sums its tiles into its own partial -- in LDS
 * when it fits beside the tile, else in its row of the workspace -- and a second launch adds the rows in workgroup order.  Every output
 * element has one writer, every sum runs in a fixed order, no atomics: bitwise reproducible, and a sample's input
 * gradients do not depend on its batch neighbours.
 *
 *   dlwp_mgn_mlp_bwd_f32: in_dev / grad_out_dev in the layouts of dlwp_mgn_mlp_f32 (in_layout / out_layout).  grad_in_dev
 *   (optional, NULL: not computed -- the edge encoder's constant input) in in_layout.  param_grad_dev: the flat array above.
 *   dlwp_mgn_mlp_bwd_workspace_bytes: the partial rows (0 outside the envelope). */
size_t dlwp_mgn_mlp_bwd_workspace_bytes(const dlwp_mgn_mlp_desc* mlp, int32_t batch, int32_t rows);
int32_t dlwp_mgn_mlp_bwd_f32(const dlwp_mgn_mlp_desc* mlp, const float* in_dev, const float* grad_out_dev,
                             float* grad_in_dev, float* param_grad_dev, int32_t batch, int32_t rows, int32_t in_layout,
                             int32_t out_layout, void* workspace, size_t workspace_bytes, void* stream);

/* The backward of dlwp_mgn_processor_layer_f32 (same graph, MLPs, aggregation, x_in_dev and e_in_dev / stride).
 * src_row_ptr_dev [n_nodes + 1] / src_perm_dev [n_edges]: the CSC edges sorted by source (stable), a CSR by source:
 * src_perm_dev[j] for src_row_ptr[n] <= j < src_row_ptr[n + 1] are the CSC indices of the edges leaving n.
 * dx_out_dev [batch, n_nodes, D]; de_out_dev [batch, n_edges, D] or NULL (the last layer of a message-passing step, whose
 * e' nothing reads).  Outputs: dx_in_dev [batch, n_nodes, D]; de_in_dev [batch, n_edges, D], or [n_edges, D] summed over
 * the batch in sample order when the stride is 0 (the shared encoded edge table); edge_grad_dev / node_grad_dev the flat
 * parameter gradients.  Outputs may not alias inputs.  Launches: the destination-owner pass (edge MLP and node MLP
 * recomputed and backpropagated in LDS; x_src parts of the edge-input gradient to a [batch, n_edges, D] scratch), the
 * source-side gather into dx_in, and the fixed-order sums of the parameter partials (and of a shared table's de_in).
 *   dlwp_mgn_processor_layer_bwd_workspace_bytes: partial rows + the x_src scratch (+ the per-sample de_in when e_shared). */
size_t dlwp_mgn_processor_layer_bwd_workspace_bytes(const dlwp_mgn_mlp_desc* edge_mlp, const dlwp_mgn_mlp_desc* node_mlp,
                                                    int32_t n_nodes, int32_t n_edges, int32_t batch, int32_t e_shared);
int32_t dlwp_mgn_processor_layer_bwd_f32(const dlwp_mgn_mlp_desc* edge_mlp, const dlwp_mgn_mlp_desc* node_mlp,
                                         int32_t aggregation, const int32_t* row_ptr_dev, const int32_t* src_dev,
                                         const int32_t* dst_dev, const int32_t* src_row_ptr_dev, const int32_t* src_perm_dev,
                                         int32_t n_nodes, int32_t n_edges, int32_t batch, const float* x_in_dev,
                                         const float* e_in_dev, int64_t e_in_batch_stride, const float* dx_out_dev,
                                         const float* de_out_dev, float* dx_in_dev, float* de_in_dev, float* edge_grad_dev,
                                         float* node_grad_dev, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * GraphCastNet (reference models/graphcast/graph_cast_net.py; MeshGraphMLP / MeshGraphEdgeMLPConcat of
 * gnn_layers/mesh_graph_mlp.py, aggregate_and_concat of gnn_layers/utils.py): a wide gather-GEMM (csrc/graphcast.hip)
 * ------------------------------------------------------------------------------------------ */
/* One Linear over batch * rows rows:  out[m][j] = act(sum_k A[m][k] wt[k][j] + bias[j] + src_products[src[p]][j]
 * + dst_products[dst[p]][j]) + res[m][j], row m = b * rows + p.  wt is the weight TRANSPOSED, [k][n] row-major.
 * A operand (a_mode):
 *   0  A[m][k] = a[b * a_batch_stride + p * lda + k]            (a_batch_stride 0: one table shared by the batch)
 *   1  A[m][k] = a[b * a_batch_stride + k * rows + p]           (channels-first [B, K, rows])
 *   2  A[m][k] = agg_{row_ptr[p] <= i < row_ptr[p + 1]} agg_e[b * agg_batch_stride + i * agg_width + k]  for k < agg_width
 *               (sum in CSC order; agg_mean 1 divides by the count; an empty row is 0),
 *      A[m][k] = a[b * a_batch_stride + p * lda + k - agg_width]  above: the node MLP's [agg, x] without the concat.
 * The gathered products (each optional, with its index array of `rows` entries) are the first edge Linear's node terms.
 * act: 0 none, 1 ReLU, 2 SiLU.  out_layout 0: out[m * ldo + j]; 1: channels-first out[(b * n + j) * rows + p].
 * res (optional) in the output's layout, sample b at res + b * res_batch_stride.  Envelope: k <= 4096, n <= 512, batch <=
 * 65535, otherwise DLWP_ERR_UNSUPPORTED.  out may not alias a or agg_e.  No atomics: bitwise reproducible. */
typedef struct dlwp_gc_linear_args {
  int32_t a_mode;
  const float* a;
  int64_t a_batch_stride;
  int32_t lda;
  const float* agg_e;
  int64_t agg_batch_stride;
  int32_t agg_width;
  const int32_t* row_ptr;
  int32_t agg_mean;
  const float* wt;
  const float* bias;
  int32_t k;
  int32_t n;
  int32_t batch;
  int32_t rows;
  const float* src_products;
  const int32_t* src_index;
  int64_t src_products_batch_stride;
  int32_t ld_src_products;
  const float* dst_products;
  const int32_t* dst_index;
  int64_t dst_products_batch_stride;
  int32_t ld_dst_products;
  int32_t act;
  float* out;
  int32_t out_layout;
  int32_t ldo;
  const float* res;
  int64_t res_batch_stride;
  /* training (zero: off; every earlier field keeps its meaning) */
  int32_t a_act;              /* A[m][k] <- act(A[m][k]) as it is loaded (a_mode 0 / 1; act codes as `act`) */
  const float* act_grad_z;    /* optional: out[m][j] *= act'(act_grad_z[m * ld_act_grad_z + j]) before res (out_layout 0) */
  int32_t act_grad;           /* 1 ReLU, 2 SiLU */
  int32_t ld_act_grad_z;
} dlwp_gc_linear_args;

int32_t dlwp_gc_linear_f32(const dlwp_gc_linear_args* args, void* stream);

/* out[m] = LayerNorm(in[m]) (two-pass mean / biased variance, like torch) [+ res], rows of `width` <= 512 over batch * rows
 * rows; res (optional) [rows, width] per sample at res_dev + b * res_batch_stride (0: shared).  out may equal in. */
int32_t dlwp_gc_layernorm_f32(const float* in_dev, float* out_dev, int32_t batch, int32_t rows, int32_t width,
                              const float* gamma, const float* beta, float eps, const float* res_dev,
                              int64_t res_batch_stride, void* stream);

/* ---- GraphCastNet backward (csrc/graphcast_bwd.hip) -------------------------------------------------------------------
 * The data gradients dA = dZ W of every Linear are dlwp_gc_linear_f32 with torch's [out][in] weight as its [k][n] operand
 * (and the act' epilogue above); the entry points below add the weight gradients, the LayerNorm backward and the
 * fixed-order segment sums.  No atomics: every result is bitwise reproducible. */

/* dW = A^T dZ (+ db = column sums of dZ) over batch * rows rows, dW written in torch's [n][k] layout at
 * dw[j * ldw + k] (ldw >= k: a column block of a wider weight), db[j] (optional).  The A operand takes the A fields of
 * dlwp_gc_linear_args (a_mode 0 / 1 / 2, a, a_batch_stride, lda, agg_e, agg_batch_stride, agg_width, row_ptr, agg_mean,
 * a_act; k, n, batch, rows); dZ is row-major dz[m * ldz + j] (dz_layout 0) or channels-first dz[(b * n + j) * rows + p]
 * (dz_layout 1).  The rows are split into slices; each workgroup writes its partial tile to the workspace and a second
 * kernel adds the slices in order.  Envelope as dlwp_gc_linear_f32 with k and n exchanged: k <= 4096, n <= 512.
 *   dlwp_gc_weight_grad_workspace_bytes: the slice partials (bounded: at most 32 MiB of dW partials), 0 outside. */
size_t dlwp_gc_weight_grad_workspace_bytes(int32_t k, int32_t n, int32_t batch, int32_t rows);
int32_t dlwp_gc_weight_grad_f32(const dlwp_gc_linear_args* a_operand, const float* dz, int32_t dz_layout, int32_t ldz,
                                float* dw, int32_t ldw, float* db, void* workspace, size_t workspace_bytes, void* stream);

/* LayerNorm backward over batch * rows rows of `width` <= 512, one wave per row, mean / rstd recomputed from the saved
 * LayerNorm input x.  The row's output gradient is
 *   g[m] = gy[m] (optional) + g_agg[b * g_agg_batch_stride + idx[p] * width] (optional) / deg[idx[p]] (deg optional)
 * (the residual edge gradient plus the node MLP's aggregate gradient gathered by the edge's destination).  Writes g to
 * g_total (optional), the input gradient to gx, and dgamma / dbeta (fixed-order per-workgroup partials, then summed in
 * order).  dlwp_gc_layernorm_bwd_workspace_bytes: the partials. */
size_t dlwp_gc_layernorm_bwd_workspace_bytes(int32_t batch, int32_t rows, int32_t width);
int32_t dlwp_gc_layernorm_bwd_f32(const float* x, const float* gamma, float eps, const float* gy, const float* g_agg,
                                  int64_t g_agg_batch_stride, const int32_t* idx, const int32_t* deg, int32_t batch,
                                  int32_t rows, int32_t width, float* g_total, float* gx, float* dgamma, float* dbeta,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* out[b'][n][c] = sum over the segment of n of in[b][i][c], i = perm[j] (perm optional) for row_ptr[n] <= j <
 * row_ptr[n + 1] (row_ptr NULL: the segment of n is row n alone), in order; an empty segment is 0.  in: sample b at
 * in + b * in_batch_stride.  batch_sum 0: b' = b; 1: one output, summed over the batch in sample order (the gradient of
 * a table the batch shares). */
int32_t dlwp_gc_segment_sum_f32(const float* in, int64_t in_batch_stride, const int32_t* row_ptr, const int32_t* perm,
                                int32_t n_segments, int32_t width, int32_t batch, int32_t batch_sum, float* out,
                                void* stream);

/* The tail of a training step (csrc/optim.hip): everything scripts/train.py:186-312 does once the gradients exist.  All
 * arithmetic is fp32 unless stated; every reduction has a fixed order and one writer (no float atomics): reruns are bitwise
 * identical.  No entry point reads a device value on the host, and no step-dependent value is an argument: a recorded step
 * replays.
 *
 * The multi-tensor table (the dlwp_mt_* calls) is a set of device arrays, built once by the caller:
 *   per tensor t   p_ptrs_dev[t], g_ptrs_dev[t]: the addresses of the parameter and of its gradient as int64 (g 0: no
 *                  gradient this step, the tensor is skipped); numel_dev[t]; state_off_dev[t]: its element offset into the
 *                  flat state arenas (exp_avg, exp_avg_sq, shadow), a multiple of 4; group_dev[t]: its parameter group;
 *                  step_dev[t]: its step count; derived_dev[t][8]: scratch the AdamW header kernel fills
 *   per group g    hyper_dev[g][5] doubles: lr, beta1, beta2, eps, weight_decay
 *   per chunk c    chunk_tensor_dev[c], chunk_first_dev[c]: dlwp_mt_chunk_elems() consecutive elements of one tensor (fewer
 *                  at its end), chunk_first a multiple of that number; the chunks cover every element exactly once
 * A workgroup takes whole chunks; the grid is capped at 2048 workgroups and strided above.  16-byte accesses where the
 * tensor's pointers are 16-byte aligned, 4-byte ones for a tensor that is not and for every ragged tail. */
int32_t dlwp_mt_chunk_elems(void);
/* criterion(output, target) of train.py:263 with CustomMSELoss (scripts/losses.py:175-188): mean((t - x)^2 w) over x_dev,
 * t_dev viewed as [outer, inner] and w_dev [inner] (NULL: unweighted; w_is_f64: a float64 weight, used as float64 as the
 * reference's promotion does).  One pass reads x and t once, leaves dlwp_mse_loss_partials(outer * inner) per-workgroup
 * partial sums in partials_dev (doubles) and, when grad_dev is given, writes d loss / d x = 2 (x - t) w / N in the same pass;
 * a single-workgroup finish adds the partials in a fixed order in double.  out_dev is a 16-byte block: the mean as a double
 * in bytes 0-7 and as a float in bytes 8-11.  The per-element arithmetic is double.
 *   dlwp_mse_loss_partials: min(ceil(n / 4096), 2048), 0 for n <= 0.
 *   dlwp_mse_loss_scale_grad_f32: grad *= upstream (a device scalar, float or double): the backward under an upstream
 *     gradient; reads and writes nothing when the scalar is exactly 1. */
int32_t dlwp_mse_loss_partials(int64_t n);
int32_t dlwp_mse_loss_f32(const float* x_dev, const float* t_dev, const void* w_dev, int32_t w_is_f64, float* grad_dev,
                          double* partials_dev, double* out_dev, int64_t outer, int64_t inner, void* stream);
int32_t dlwp_mse_loss_scale_grad_f32(float* grad_dev, const void* upstream_dev, int32_t upstream_is_f64, int64_t n,
                                     void* stream);
/* th.nn.utils.clip_grad_norm_(model.parameters(), max_norm) of train.py:299-305, norm type 2, with the arithmetic of
 * torch/nn/utils/clip_grad.py:165-169 (torch 2.10):  dlwp_mt_grad_norm_f32 writes one sum of squares per chunk to partials_dev [n_chunks] and
 * a finish kernel adds them in double, then writes scal_dev[0] = total_norm and scal_dev[1] = clip_coef =
 * min(1, max_norm / (total_norm + 1e-6)) (a NaN stays NaN).  dlwp_mt_scale_f32: g *= scal_dev[1] in place, also when it
 * is 1, as torch does. */
int32_t dlwp_mt_grad_norm_f32(const int64_t* g_ptrs_dev, const int64_t* numel_dev, const int32_t* chunk_tensor_dev,
                              const int64_t* chunk_first_dev, int32_t n_chunks, float* partials_dev, float max_norm,
                              float* scal_dev, void* stream);
int32_t dlwp_mt_scale_f32(const int64_t* g_ptrs_dev, const int64_t* numel_dev, const int32_t* chunk_tensor_dev,
                          const int64_t* chunk_first_dev, int32_t n_chunks, const float* scal_dev, void* stream);
/* optimizer.zero_grad() of train.py:186 with the gradient storage kept: every gradient of the table becomes 0. */
int32_t dlwp_mt_zero_f32(const int64_t* g_ptrs_dev, const int64_t* numel_dev, const int32_t* chunk_tensor_dev,
                         const int64_t* chunk_first_dev, int32_t n_chunks, void* stream);
/* optimizer.step() of train.py:309 with th.optim.AdamW (train.py:59; torch 2.10's
 * torch/optim/adam.py:347-547, _single_tensor_adam with decoupled weight decay), one pass
 * over p, g, exp_avg, exp_avg_sq (16 bytes read, 12 written per element):
 *   p *= 1 - lr wd;  m = lerp(m, g, 1 - beta1);  v = beta2 v + (1 - beta2) g g;  p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
 * A header kernel (one thread per tensor) first advances step_dev[t] of every tensor with a gradient and derives lr / bc1
 * and 1 / sqrt(bc2) from it in double into derived_dev; a tensor without a gradient is skipped and keeps its step.
 * scal_dev non-NULL: the kernel consumes g * scal_dev[1] (the clip coefficient dlwp_mt_grad_norm_f32 left) without
 * writing the gradient back -- the fused last clip, bit for bit dlwp_mt_scale_f32 followed by the plain call. */
int32_t dlwp_mt_adamw_f32(const int64_t* p_ptrs_dev, const int64_t* g_ptrs_dev, const int64_t* numel_dev,
                          const int64_t* state_off_dev, const int32_t* group_dev, int32_t* step_dev, float* derived_dev,
                          const double* hyper_dev, int32_t n_tensors, const int32_t* chunk_tensor_dev,
                          const int64_t* chunk_first_dev, int32_t n_chunks, float* exp_avg_dev, float* exp_avg_sq_dev,
                          const float* scal_dev, void* stream);
/* ema.update() of train.py:312: shadow = decay shadow + (1 - decay) p over every tensor of the table, shadow_dev the flat
 * arena state_off_dev indexes. */
int32_t dlwp_mt_ema_f32(const int64_t* p_ptrs_dev, const int64_t* numel_dev, const int64_t* state_off_dev,
                        const int32_t* chunk_tensor_dev, const int64_t* chunk_first_dev, int32_t n_chunks, float* shadow_dev,
                        float decay, float one_minus_decay, void* stream);

/* The PDE-Refiner noise scheduler on the device (csrc/refiner.hip, csrc/philox_normal.hpp): the noise, the ancestral step and
 * the training pair of the diffusion backbones, one elementwise pass each.  256 threads per workgroup, one thread per block of
 * 4 consecutive elements, the grid capped at 1024 workgroups and strided above (dlwp_refiner_grid_span() = the elements one
 * sweep of a full grid covers); 16-byte accesses where every pointer of the call is 16-byte aligned, 4-byte ones for an
 * unaligned view and for the ragged tail.  One writer per element; no entry point allocates, synchronises or reads a device
 * value on the host.
 *
 * The noise stream is a pure function of (seed, global element index g): Philox4x32-10 with key = (seed low word, seed high
 * word) and counter = (q low word, q high word, 0, 0) for q = g / 4; word pair (x0, x1) gives lanes 0 / 1 and (x2, x3) lanes
 * 2 / 3 of the block by Box-Muller, u = float(x) 2^-32 + 2^-33, r = sqrt(-2 ln u_a), theta = 6.2831855f u_b, r cos theta /
 * r sin theta.  `offset` is the global index of element 0 of a call: a non-negative multiple of 4.  `seed` carries 64 bits
 * (an unsigned value reinterpreted). */
int64_t dlwp_refiner_grid_span(void);
/* y_noised = torch.randn(target_shape) of modern_unet.py:184 (and the variance noise inside noise_scheduler.step, :201),
 * drawn on the device: out_dev[e] = normal(seed, offset + e) for e < n. */
int32_t dlwp_philox_normal_f32(float* out_dev, int64_t n, int64_t seed, int64_t offset, void* stream);
/* noise_scheduler.step(pred, k, y_noised).prev_sample of modern_unet.py:201 (DDPM ancestral step, v-prediction, variance
 * "fixed_small") in one pass:
 *   prev = c0 (sa sample - sb model_output) + c1 sample + sigma z
 * coef (HOST doubles, read at the call) = { c0 sa, c0 sb, c1, sigma }; the launch folds them to A = c0 sa + c1 and B = -c0 sb in
 * double and rounds once to fp32.  z is read from noise_or_null_dev when given, else drawn at the element's own index exactly
 * as dlwp_philox_normal_f32 would draw it; with sigma == 0 (t = 0) no noise is drawn or read.  out_dev may be sample_dev. */
int32_t dlwp_ddpm_step_f32(const float* sample_dev, const float* model_output_dev, const float* noise_or_null_dev,
                           float* out_dev, int64_t n, const double coef[4], int64_t seed, int64_t offset, void* stream);
/* The training pair of train.py:228-255 in one pass:
 *   res = target - prog_last;  y_noised = sqrt_abar res + sqrt_1m_abar eps;  v_target = sqrt_abar eps - sqrt_1m_abar res
 * target_dev is [batch, 1, channels, faces, plane] (plane = h w), prog_last_dev the frame prognostic[:, context_size - 1] read
 * in place: [channels, faces, plane] contiguous per batch entry, the entries target_batch_stride / prog_batch_stride elements
 * apart.  The outputs are [(batch faces), 1, channels, plane] contiguous: faces > 1 is the einops.rearrange
 * "b t c f h w -> (b f) t c h w" of train.py:232-233 by index arithmetic, faces = 1 the lat-lon case.  eps is indexed by the
 * OUTPUT's linear index: read from noise_or_null_dev when given, else drawn as dlwp_philox_normal_f32 would draw it. */
int32_t dlwp_refiner_pair_f32(const float* target_dev, const float* prog_last_dev, const float* noise_or_null_dev,
                              float* y_noised_dev, float* v_target_dev, int32_t batch, int32_t faces, int32_t channels,
                              int64_t plane, int64_t target_batch_stride, int64_t prog_batch_stride, float sqrt_abar,
                              float sqrt_1m_abar, int64_t seed, int64_t offset, void* stream);
/* Member streams, for ensembles of one initial condition: normal(seed, member, g) is the stream above with counter word 2 =
 * member (a uint32; word 3 stays 0), so member 0 is the stream of the entry points above bit for bit.  The two entry points
 * below are dlwp_philox_normal_f32 and dlwp_ddpm_step_f32 on member-major tensors [members][n_per_member]: element (m, e) uses
 * normal(seed, first_member + m, offset + e), with 0 <= first_member and first_member + members <= 2^31.  The definition is
 * per element: n_per_member need not be a multiple of 4 (a thread's block of four may then straddle a member boundary), and
 * members first_member .. first_member + members - 1 drawn in one call are bitwise the members of any split of that range into
 * several calls.  Launch rules as above; with sigma == 0 nothing is drawn or read, with noise_or_null_dev given it is read
 * ([members][n_per_member], like the sample) and nothing is drawn. */
int32_t dlwp_philox_normal_members_f32(float* out_dev, int64_t n_per_member, int32_t members, int32_t first_member,
                                       int64_t seed, int64_t offset, void* stream);
int32_t dlwp_ddpm_step_members_f32(const float* sample_dev, const float* model_output_dev, const float* noise_or_null_dev,
                                   float* out_dev, int64_t n_per_member, int32_t members, int32_t first_member,
                                   const double coef[4], int64_t seed, int64_t offset, void* stream);

/* The device-resident WeatherBench dataset (csrc/dataset.hip; data.DeviceWeatherDataset drives these).  The fields are ONE
 * float32 store_dev [n_times, n_vars, plane], contiguous: time first, variables with levels flattened into n_vars by the host,
 * plane = H W on a lat-lon grid and 12 n n on HEALPix.  The store may hold more than 2^31 elements: every offset into it is
 * 64-bit; a time index is an int32.  256 threads per workgroup, a thread per 4 consecutive plane elements, a workgroup per tile
 * of 256 such units of one plane, the grid capped at dlwp_dataset_grid_blocks() workgroups and strided above; 16-byte accesses
 * where plane % 4 == 0 and the pointer in question is 16-byte aligned, 4-byte ones of the same elements otherwise.  No atomics;
 * no entry point allocates, synchronises or reads a device value on the host.  A frame index outside [0, n_times) is never
 * dereferenced. */
int32_t dlwp_dataset_grid_blocks(void);
/* One batch of WeatherBenchDataset.__getitem__ + default_collate (reference data/datasets/datasets.py:330-416) in one launch.
 *   frames_dev      int32 [batch, seq + 1]: the store time index of every frame of every window, -1 = no such frame
 *   items_dev       int32 [batch]: the dataset item of every sample = the member of its noise stream; read only with noise != 0
 *   *_table_dev     int32 [n, 4], 16-byte aligned: {source variable, mean as fp32 bits, std as fp32 bits, replace-NaN-by-0 flag}
 *   prescribed_dev  [batch, seq, n_pres, plane]            = frames 0 .. seq - 1 (:345, :371, :375); may be null
 *   prognostic_dev  [batch, seq, n_prog, plane]            = frames 0 .. seq - 1, plus noise eps (:384-403, :414); may be null
 *   target_dev      [batch, seq - context, n_prog, plane]  = frames 1 + context .. seq, never noised (:413, :416); may be null
 * A value is (x - mean) / std with two correctly rounded fp32 operations when `normalize` (else x), then 0 where it is NaN and
 * the channel's flag is set (:397, :401); a frame -1 is zeros (:405-409).  Frame j of a window is loaded ONCE and serves
 * prognostic[:, j] and target[:, j - 1 - context]; a frame no output asks for is not loaded.  eps for sample b is the member
 * stream (seed, member = items_dev[b], offset) of dlwp_philox_normal_members_f32 over the sample's own [seq, n_prog, plane]
 * elements, evaluated in the kernel: prognostic = x + noise eps (an fp32 product, then an fp32 sum).  All pointers are device
 * memory read at execution time: a recorded launch follows a frame table that is overwritten in place. */
int32_t dlwp_dataset_gather_f32(const float* store_dev, int64_t n_times, int32_t n_vars, int64_t plane,
                                const int32_t* frames_dev, const int32_t* items_dev, int32_t batch, int32_t seq,
                                int32_t context, const int32_t* prog_table_dev, int32_t n_prog, const int32_t* pres_table_dev,
                                int32_t n_pres, float* prescribed_dev, float* prognostic_dev, float* target_dev,
                                int32_t normalize, float noise, int64_t seed, int64_t offset, void* stream);
/* compute_statistics (datasets.py:419-453; xarray's .mean() / .std() skip NaN, .std() has ddof 0) over the frames
 * frames_dev int32 [n_frames] (the used times after the timedelta stride, :291).  out_dev double [n_vars, 3] = {count of non-NaN
 * values, their sum, the sum of squared deviations from sum / count}: mean = sum / count and std = sqrt(ssd / count) are the
 * caller's.  Two passes over the resident store, four launches on `stream`; every add is fp64, each pass writes 128 workgroup
 * partials per variable into the workspace and one thread adds them in workgroup order: repeated calls give the same bits. */
size_t dlwp_dataset_stats_workspace_bytes(int32_t n_vars);
int32_t dlwp_dataset_stats_f64(const float* store_dev, int64_t n_times, int32_t n_vars, int64_t plane, const int32_t* frames_dev,
                               int64_t n_frames, double* out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
/* groupby(...).mean() over time (the monthly climatology of climatology.py:41 and scripts/build_baselines.py:64).
 * groups_dev int32 [n_frames]: the group 0 .. n_groups - 1 of every listed frame, any other value = skip.
 * out_dev [n_groups, n_vars, plane]: the mean of the group's non-NaN values per element, summed in fp64 in list order by the one
 * thread that owns the element, divided in fp64 and rounded to fp32 once; NaN where the group has no value.  Each stored value
 * of a listed frame is read once. */
int32_t dlwp_dataset_group_mean_f32(const float* store_dev, int64_t n_times, int32_t n_vars, int64_t plane,
                                    const int32_t* frames_dev, const int32_t* groups_dev, int64_t n_frames, int32_t n_groups,
                                    float* out_dev, void* stream);
/* ds.coarsen(lat=k, lon=k).mean() (datasets.py:303-305): in_dev [planes, height, width] -> out_dev [planes, height / k,
 * width / k], the mean of the non-NaN values of each k x k block (NaN for a block without one), summed in fp64 in row-major
 * block order and rounded to fp32 once.  height and width must be multiples of k (xarray's boundary="exact").  16-byte accesses
 * for k = 2, 4 where width / k % 4 == 0 and both pointers are 16-byte aligned. */
int32_t dlwp_coarsen_mean_f32(const float* in_dev, float* out_dev, int64_t planes, int32_t height, int32_t width, int32_t k,
                              void* stream);

/* Real spherical harmonic transforms and the per-degree channel mix of the SFNO backbone (csrc/sht.hip; the reference reaches
 * them through torch_harmonics from models/fno/fno.py:183-200 -- PARITY UNPINNED, the conventions are those of
 * dlwp_benchmark_amd/sphere.py and DESIGN.md section 35).  All tables are fp32, made on the host (sphere.device_tables):
 *   wleg_dev [nlat][lmax][mmax] = P[m, l, k] w_k,  leg_dev [lmax][nlat][mmax] = P[m, l, k]  (zero for l < m, never read there),
 *   tw_dev [nlon][2] = (cos, -sin)(2 pi t / nlon), indexed by (j m) mod nlon: no transcendental runs on the device.
 * Envelope: 2 <= nlat <= 256, 2 <= nlon <= 512 and even, 1 <= lmax <= nlat, 1 <= mmax <= nlon / 2 + 1, planes >= 1 (64-bit);
 * DLWP_ERR_UNSUPPORTED outside it.  One launch each on `stream`, fixed summation order, no atomics: a call repeated gives the
 * same bits.  Outputs may not alias inputs.
 *
 * dlwp_sht_f32:   x_dev [planes, nlat, nlon] -> coeffs_dev [planes, lmax, mmax, 2] (re, im):
 *   X[k][m] = (2 pi / nlon) sum_j x[k][j] tw[(j m) mod nlon],   c[l][m] = sum_k wleg[k][l][m] X[k][m]   (l >= m; zero below)
 * dlwp_isht_f32:  coeffs_dev [planes, lmax, mmax, 2] -> y_dev [planes, nlat, nlon]:
 *   X[k][m] = f_m sum_{l >= m} leg[l][k][m] c[l][m]  with f_m = 1 for m = 0 and m = nlon / 2 (imaginary part dropped), else 2,
 *   y[k][j] = sum_m Re(X[k][m]) tw[(j m) mod nlon].re + Im(X[k][m]) tw[(j m) mod nlon].im   -- irfft(n = nlon, norm = "forward")
 *   Entries of coeffs_dev with l < m are not read. */
int32_t dlwp_sht_f32(const float* x_dev, const float* wleg_dev, const float* tw_dev, float* coeffs_dev, int64_t planes,
                     int32_t nlat, int32_t nlon, int32_t lmax, int32_t mmax, void* stream);
int32_t dlwp_isht_f32(const float* coeffs_dev, const float* leg_dev, const float* tw_dev, float* y_dev, int64_t planes,
                      int32_t nlat, int32_t nlon, int32_t lmax, int32_t mmax, void* stream);
/* Spherical power spectra of a rollout and its targets (csrc/sph_power.hip; the reference has no
 * spherical spectrum -- PARITY UNPINNED).  out_dev, target_dev [b, k, c, nlat, nlon] fp32, contiguous; wleg_dev, tw_dev: the
 * forward tables of dlwp_sht_f32, in its envelope (DLWP_ERR_UNSUPPORTED outside it).  With c = sht(x) and f_m = 1 for m = 0 and
 * 2 m = nlon (the imaginary part of c is dropped there, as dlwp_isht_f32 ignores it), f_m = 2 otherwise,
 *   power(x)[l] = sum_{m <= min(l, mmax - 1)} f_m |c[l][m]|^2,   cross(x, y)[l] = sum_m f_m Re(c_x[l][m] conj c_y[l][m]).
 * sums_dev: double [4, k, c, lmax], written by the call (dlwp_sph_power_sums_f32) or added to (dlwp_sph_power_sums_acc_f32):
 *   0: sum_b power(out)   1: sum_b power(target)   2: sum_b power(out - target)   3: sum_b cross(out, target)
 * The difference of index 2 is formed in the FIELD domain, in fp32, before it is transformed.  A north-south flip of both
 * inputs on a symmetric grid changes none of the four.  fp32 transforms (the two stages of dlwp_sht_f32; no coefficient is
 * written to memory), fp64 from the squares on.  First launch: one fp64 partial per ((b, k, c), m tile, quantity, l) into the
 * workspace, the terms of a degree added over the tile's m in ascending order; second launch: one thread per (quantity, k, c, l)
 * adds the partials in one chain, b ascending and m tiles ascending inside a b, starting from zero or (_acc) from what sums_dev
 * holds -- a batch cut anywhere and fed through _acc gives the bits of the one-shot call.  The tiling depends on (nlat, nlon,
 * lmax, mmax) alone.  No atomics, no host synchronisation; tw_dev, sums_dev and workspace_dev 8-byte aligned.
 *   dlwp_sph_power_workspace_bytes: the partials (0 for a shape outside the envelope); a smaller workspace returns
 *   DLWP_ERR_WORKSPACE. */
size_t dlwp_sph_power_workspace_bytes(int32_t b, int32_t k, int32_t c, int32_t nlat, int32_t nlon, int32_t lmax, int32_t mmax);
int32_t dlwp_sph_power_sums_f32(const float* out_dev, const float* target_dev, const float* wleg_dev, const float* tw_dev,
                                double* sums_dev, int32_t b, int32_t k, int32_t c, int32_t nlat, int32_t nlon, int32_t lmax,
                                int32_t mmax, void* workspace_dev, size_t workspace_bytes, void* stream);
int32_t dlwp_sph_power_sums_acc_f32(const float* out_dev, const float* target_dev, const float* wleg_dev, const float* tw_dev,
                                    double* sums_dev, int32_t b, int32_t k, int32_t c, int32_t nlat, int32_t nlon, int32_t lmax,
                                    int32_t mmax, void* workspace_dev, size_t workspace_bytes, void* stream);
/* Driscoll-Healy spectral convolution: c_out[b][o][l][m] = sum_i c_in[b][i][l][m] * weight[i][o][l] (complex) for
 * m <= min(l, mmax - 1); every other entry of c_out is written as zero and no entry of c_in with m > l is read.
 *   c_in_dev [batch, cin, lmax, mmax, 2], weight_dev [cin, cout, lmax, 2], c_out_dev [batch, cout, lmax, mmax, 2].
 * Per degree l a complex GEMM with rows (b, m <= l), K = cin, N = cout on the exact-fp32 matrix instruction
 * (v_mfma_f32_16x16x4_f32), products summed in the order i = 0, 1, ...  Any batch, cin, cout >= 1 with batch * mmax < 2^24,
 * 1 <= lmax, mmax <= 1024. */
int32_t dlwp_sph_mix_f32(const float* c_in_dev, const float* weight_dev, float* c_out_dev, int32_t batch, int32_t cin,
                         int32_t cout, int32_t lmax, int32_t mmax, void* stream);
/* The same product from the weight re-laid degree-major, packed_dev [lmax, cin, cout, 2], which dlwp_sph_mix_pack_f32 makes from
 * weight_dev [cin, cout, lmax, 2] (one transposing launch).  The parameter layout costs a workgroup a 128-byte line per 8 bytes
 * it uses; the packed one is read in 512-byte runs.  Same arithmetic in the same order: the two entry points give the same bits. */
int32_t dlwp_sph_mix_packed_f32(const float* c_in_dev, const float* packed_dev, float* c_out_dev, int32_t batch, int32_t cin,
                                int32_t cout, int32_t lmax, int32_t mmax, void* stream);
int32_t dlwp_sph_mix_pack_f32(const float* weight_dev, float* packed_dev, int32_t cin, int32_t cout, int32_t lmax, void* stream);

/* The backwards of the three operators above (training of the SFNO backbone; the reference differentiates torch_harmonics from
 * models/fno/fno.py:183-200 by autograd).  Gradients of complex tensors follow torch's convention g = dL/dRe + i dL/dIm.  Each
 * transform's adjoint is the OTHER transform's kernel over the table its forward reads, with the table strides exchanged: the
 * same envelope, tiling and LDS budget as the forward, fixed summation order, no atomics.
 * dlwp_sht_bwd_f32:   g_dev [planes, lmax, mmax, 2] (the cotangent of the spectrum) -> gx_dev [planes, nlat, nlon]:
 *   Y[k][m] = (2 pi / nlon) sum_{l >= m} wleg[k][l][m] g[l][m],   gx[k][j] = sum_m Re(Y) tw[(j m) mod nlon].re + Im(Y) tw[..].im
 *   Entries of g_dev with l < m are not read.
 * dlwp_isht_bwd_f32:  gy_dev [planes, nlat, nlon] -> gc_dev [planes, lmax, mmax, 2]:
 *   Z[k][m] = f_m sum_j gy[k][j] tw[(j m) mod nlon]  (f_m as in dlwp_isht_f32, imaginary part zero where f_m = 1),
 *   gc[l][m] = sum_k leg[l][k][m] Z[k][m]  (l >= m; written as zero below). */
int32_t dlwp_sht_bwd_f32(const float* g_dev, const float* wleg_dev, const float* tw_dev, float* gx_dev, int64_t planes,
                         int32_t nlat, int32_t nlon, int32_t lmax, int32_t mmax, void* stream);
int32_t dlwp_isht_bwd_f32(const float* gy_dev, const float* leg_dev, const float* tw_dev, float* gc_dev, int64_t planes,
                          int32_t nlat, int32_t nlon, int32_t lmax, int32_t mmax, void* stream);
/* Input gradient of dlwp_sph_mix_f32: gc_in[b][i][l][m] = sum_o g[b][o][l][m] conj(weight[i][o][l]) for m <= min(l, mmax - 1), zero
 * above; entries of g_dev above the diagonal are not read.  The forward kernel with the weight read conjugate-transposed in place.
 *   g_dev [batch, cout, lmax, mmax, 2], weight_dev [cin, cout, lmax, 2], gc_in_dev [batch, cin, lmax, mmax, 2].
 * dlwp_sph_mix_pack_adjoint_f32 makes the degree-major image of the conjugate transpose, packed_dev [lmax, cout, cin, 2], with
 * which dlwp_sph_mix_packed_f32(g_dev, packed_dev, gc_in_dev, batch, cout, cin, ...) gives the same bits. */
int32_t dlwp_sph_mix_dgrad_f32(const float* g_dev, const float* weight_dev, float* gc_in_dev, int32_t batch, int32_t cin,
                               int32_t cout, int32_t lmax, int32_t mmax, void* stream);
int32_t dlwp_sph_mix_pack_adjoint_f32(const float* weight_dev, float* packed_dev, int32_t cin, int32_t cout, int32_t lmax,
                                      void* stream);
/* Weight gradient of dlwp_sph_mix_f32: gw[i][o][l] = sum_b sum_{m <= min(l, mmax - 1)} conj(c_in[b][i][l][m]) g[b][o][l][m]; entries
 * of either operand above the diagonal are not read.  Per degree a complex GEMM with M = cin, N = cout, K = batch * rows_l on
 * v_mfma_f32_16x16x4_f32, summed over k = (b, m) in ascending order in one accumulator chain (no split-K, no atomics).
 *   c_in_dev [batch, cin, lmax, mmax, 2], g_dev [batch, cout, lmax, mmax, 2], gw_dev [cin, cout, lmax, 2].
 * dlwp_sph_mix_wgrad_packed_f32 writes the same values degree-major, gw_packed_dev [lmax, cin, cout, 2], and
 * dlwp_sph_mix_unpack_f32 (the inverse of dlwp_sph_mix_pack_f32) transposes them into the parameter layout.  The envelope of
 * all of these is that of dlwp_sph_mix_f32. */
int32_t dlwp_sph_mix_wgrad_f32(const float* c_in_dev, const float* g_dev, float* gw_dev, int32_t batch, int32_t cin, int32_t cout,
                               int32_t lmax, int32_t mmax, void* stream);
int32_t dlwp_sph_mix_wgrad_packed_f32(const float* c_in_dev, const float* g_dev, float* gw_packed_dev, int32_t batch, int32_t cin,
                                      int32_t cout, int32_t lmax, int32_t mmax, void* stream);
int32_t dlwp_sph_mix_unpack_f32(const float* packed_dev, float* weight_dev, int32_t cin, int32_t cout, int32_t lmax, void* stream);

/* Trajectories of the incompressible 2-D Navier-Stokes equations in vorticity form on the unit torus, solved pseudo-spectrally
 * (csrc/navier_stokes.hip).  The reference tree holds no solver -- PARITY UNPINNED: the scheme is the one
 * stated in DESIGN.md section 38.1 (the data law of Li et al. 2020, "Fourier Neural Operator for Parametric PDEs"), pinned by the
 * float64 restatement tests/ns_ref.py and by the closed-form decay of a Taylor-Green vortex.
 *   w0_dev [batch, n, n] fp32: the initial vorticity, axis 0 the coordinate a = i / n, axis 1 b = j / n
 *   filter_dev [n, n / 2 + 1] fp32 or NULL: a real factor on rfft2(w0) (the amplitude table of a Gaussian random field)
 *   forcing_dev [n, n] fp32 or NULL: the forcing f(a, b), NULL for none
 *   out_dev [batch, frames, n, n] fp32: frame t is the vorticity after t * substeps sub-steps of length dt; frame 0 is w0
 *   filtered, with every mode |ka| = n / 2 or kb = n / 2 removed.  With frames == 1 out_dev may be w0_dev itself.
 * With wh = rfft2(w) (unnormalised), lap = 4 pi^2 (ka^2 + kb^2), lapi = lap except lapi[0, 0] = 1, mask = |ka|, kb <= n / 3, one
 * sub-step is
 *   psi = wh / lapi,  (u, v) = irfft2(2 pi i kb psi, -2 pi i ka psi),  (wa, wb) = irfft2(2 pi i ka wh, 2 pi i kb wh),
 *   F = mask * rfft2(u wa + v wb),  wh <- (-dt F + dt fh + (1 - dt nu lap / 2) wh) / (1 + dt nu lap / 2)
 * (advective form, Crank-Nicolson on the viscous term).  The modes |ka| = n / 2 and kb = n / 2 of the forcing are dropped as
 * those of w0 are, so they stay zero; column kb = 0 is kept exactly Hermitian (its ka < 0 half is the conjugate of the other).
 * One workgroup integrates one trajectory with wh resident in LDS for the whole launch; the 2-D transforms are the radix
 * passes of csrc/fft_radix.hpp over LDS, the twiddles a float64 host table, the per-mode factors made in float64 at the head of
 * the kernel: no transcendental runs on the device.  Fixed summation order, no atomics, no inter-workgroup traffic: a
 * trajectory's bits depend on neither the batch beside it nor on how its sub-steps are divided into frames.
 * n is 32 or 64 (128 x 128 does not fit the 160 KiB of LDS: DLWP_ERR_UNSUPPORTED, as every other n); batch, frames >= 1,
 * substeps >= 1, frames * substeps at most the cap stated in csrc/navier_stokes.hip (DLWP_ERR_UNSUPPORTED above it: one
 * launch stays within seconds), dt > 0, nu >= 0, all finite. */
int32_t dlwp_ns2d_rollout_f32(const float* w0_dev, const float* filter_dev, const float* forcing_dev, float* out_dev, int32_t batch,
                              int32_t n, int32_t frames, int32_t substeps, double dt, double nu, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DLWP_HIP_H */
