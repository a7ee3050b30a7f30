// Host-side state of the FNO2d path, shared by fno2d.hip (plans, workspace, orchestration, C ABI), fno_unfused.hpp and
// fno_trunk.hpp: the plan and what it is made of, the workspace layout, and the host functions through which the
// orchestration launches the kernels of the two kernel files.
#pragma once

#include <atomic>

#include "fno_device.hpp"
#include "spectral_any.hpp"

namespace dlwp {
namespace fno {

struct SpectralCore {  // what one spectral convolution stage needs on the device
  int H = 0, W = 0, M1 = 0, M2 = 0, KP = 0;
  float fwd_scale = 1.f;
  DevBuf t, tt, ef, ei, ck;
  DevBuf tb, ttb;   // bf16x3 B operands of the W-direction DFTs for the fused kernel (W == 64, KP == 16 only)
  DevBuf tbh, ttbh; // the same twiddles as f16x3 parts (th, tm' = (t - th) * 2^11, 0) for the f16x3 step kernel

  int32_t build(int H_, int W_, int M1_, int M2_, const int32_t* rows_in, const int32_t* rows_out, float fwd, float inv,
                hipStream_t s);   // fno2d.hip
  size_t modes_lds_bytes() const { return (size_t)(2 * M1 * H + 18 * M1 * kC) * sizeof(float2); }
};

// kernels that need more than the default 48 KB of dynamic LDS
template <class K>
inline hipError_t allow_lds(K kernel, size_t bytes) {
  if (bytes <= 48 * 1024) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)bytes);
}

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

}  // namespace fno
}  // namespace dlwp

struct dlwp_fno2d_plan {
  using DevBuf = dlwp::DevBuf;
  dlwp::fno::FnoKnobs k;
  mutable std::atomic<unsigned> timeouts{0};   // statistics only: fused launches that timed out (re-run or reported)
  mutable std::atomic<unsigned> range_reruns{0};   // statistics only: f16x3 ranges repeated on the bf16x6 kernels (non-finite output)
  DevBuf sticky;                               // device word the fused kernels add to on a timeout (reset by dlwp_fno2d_status)
  int cin = 0, hid_l = 0, hid_p = 0, cout = 0, L = 0, H = 0, W = 0;
  int cin_steps = 0;
  dlwp::fno::SpectralCore sc;
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
  dlwp::sany::Fno* gen = nullptr;   // shapes outside the 32-channel kernels' domain: the width-generic plan (spectral_any.hip)
  ~dlwp_fno2d_plan() { dlwp::sany::fno_destroy(gen); }
};

namespace dlwp {
namespace fno {

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
inline FnoWorkspace carve(const dlwp_fno2d_plan* p, int B, void* base) {
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

struct TrunkState {   // the fused kernels' hand-off bookkeeping across the launches of one call
  bool on = false;
  unsigned epoch = 0;    // group barriers already counted since the counters were zeroed
  unsigned layers = 0;   // spectral layers run since the exchange buffers were armed (flag-in-data protocol)
};

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

// ---- fno_unfused.hpp: one launch per stage
enum class LayerForm {
  kFnoHidden,      // skip convolution + bias + GELU, and the W-direction DFT of the result for the next layer
  kFnoLast,        // skip convolution + bias (neuralop FNOBlocks: no activation behind the last layer)
  kSpectralConv,   // SpectralConv2d: the spectral term alone
};
int32_t fno_lift(const dlwp_fno2d_plan* p, const ChanTable& xt, int B, const FnoWorkspace& ws, hipStream_t s, KernelTimer* timer);
int32_t launch_fwd_dft(const SpectralCore& sc, const float* x, float* ybuf, int B, hipStream_t s);
int32_t launch_modes(const SpectralCore& sc, const float* ybuf, float* zbuf, const float2* wt, int B, hipStream_t s);
int32_t launch_layer(const SpectralCore& sc, const LayerParams& lp, LayerForm form, hipStream_t s, bool bf16x6 = true);
int32_t fno_project(const dlwp_fno2d_plan* p, const float* hin, int B, float* out, long long out_bstride, const float* resid,
                    long long resid_bstride, hipStream_t s, KernelTimer* timer);
int32_t launch_pack_spectral(const float2* src, float2* dst, int Ci, int Co, int R, int K, bool adjoint, hipStream_t s);

// ---- fno_trunk.hpp: all spectral layers, a whole step or a whole rollout range in one launch
int fused_resident_per_cu(int G);
bool step_eligible(const dlwp_fno2d_plan* p);
int32_t trunk_begin(const dlwp_fno2d_plan* p, const FnoWorkspace& ws, int B, TrunkState& st, hipStream_t s, bool force_unfused = false);
int32_t launch_trunk(const dlwp_fno2d_plan* p, const FnoWorkspace& ws, int B, const float* hin, float* hout, TrunkState& st,
                     hipStream_t s, const StepIO* io = nullptr);

// ---- fno_lift_table.hip (host only) exports the dlwp_fno2d_lift_table_* C ABI of include/dlwp_hip.h and nothing else

}  // namespace fno
}  // namespace dlwp
