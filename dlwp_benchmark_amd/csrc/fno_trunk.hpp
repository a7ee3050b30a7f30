// The fused FNO2d kernel ("trunk"): all spectral layers of a backbone step, the whole step, or a whole rollout range in ONE
// launch -- the kernel of launch forms 0 and 1 and of the benchmark.  This file holds the kernel with its hand-off
// primitives, the host functions that arm the exchange buffers and launch it (declared in fno_plan.hpp), and the
// DLWP_TRUNK_TRACE diagnostics.  A part of the translation unit fno_kernels.hip (see there), included nowhere else.
#pragma once
#include "fno_plan.hpp"

namespace dlwp {
namespace fno {

// ---------------------------------------------------------------------------------------------
// Fused trunk: ALL spectral layers of one backbone step in one launch (W = 64, H % 8 == 0, KP = 16).
//
// One workgroup = 8 consecutive grid rows of one sample, one wave per row; the G = H/8 workgroups of a
// sample form a group and every workgroup of the grid is resident at once (one per CU).  The hidden
// activation of a row (32 channels x 64 pixels) lives in 32 VGPRs of its wave from the first layer to the
// last: it is read from HBM/Infinity Cache once and written once per STEP instead of once per layer.
// What crosses workgroups is only the spectrum, M1 x M2 x 32 complex numbers per sample and layer:
//
//   per layer   P1  X_part[r][ky][c] = sum over this workgroup's 8 rows of EF[r][h] * Y[h][ky][c]   (MFMA, LDS)
//               -- group barrier --                 (X_part published with agent-scope sc1 stores)
//               P2  the group's M1*M2 modes are dealt out to its workgroups: sum the G partials,
//                   O[r][ky][o] = fwd_scale * sum_c X[r][ky][c] * Wt[ky][r][c][o]
//               -- group barrier --
//               P3  Z[h][ky][o] = ck[ky] * sum_r EI[r][h] * O[r][ky][o] for the 8 own rows          (MFMA -> LDS)
//               row y = act(bias + Wskip * x + Z * T)   skip conv on the bf16 pipe (bf16x6, B operand
//                   taken straight from the resident registers), inverse W-DFT on fp32 MFMA, packed GELU;
//                   forward W-DFT of the result -> Y row in LDS for the next layer
//
// The group barrier is an agent-scope counter: stores drained (s_waitcnt vmcnt(0)) + workgroup barrier,
// one lane adds and polls (bounded: a timeout poisons the output with NaN instead of hanging the GPU).
// Handed-off data is written and read with relaxed agent-scope atomics (sc1: write-through, L1 bypass);
// tools/ubench_groupsync.hip measures 1.3-1.6 us per barrier, 2.1 us with the payload when the group shares
// an XCD (workgroup i runs on XCD i % 8, so a sample's workgroups are i, i+8, ...).
// ---------------------------------------------------------------------------------------------
constexpr int kTrunkMaxLayers = 8;
// Seam between two steps of the fused kernel when the lifting MLP is read from the plan's table:
// the exact path's weights are staged only in a step in which some wave of the workgroup falls back to it (the "vote").
// Tried and rejected: staging them in every step (the earlier seam: request before the end-of-step
// barrier, LDS write and a second barrier behind it, a third one behind the lifting), and gathering a wave's next row from
// the table BEFORE the barrier of the seam (304 instead of 184 bytes of scratch per lane).
constexpr int kSyStride = 528;   // floats per Y row in LDS: 16 k' x 32 c + 16 (bank spread for the P1 B reads)

struct TrunkParams {
  const float* x;      // [B][32][H][64] hidden activation from the lifting kernel
  float* y;            // [B][32][H][64] output for the projection kernel
  const float* ybuf;   // [B][H][16][32] W-direction DFT of x (emitted by the lifting kernel)
  const float* t;      // T[16][64]
  const float* tt;     // TT[64][16]
  const u32x4* tb;     // [4 q][3][64]   bf16x3 B operands of the inverse W-DFT
  const u32x4* ttb;    // [2 kb][3][64]  bf16x3 B operands of the forward W-DFT
  const float2* ef;    // [M1][H]
  const float2* ei;    // [M1][H]
  const float* ck;     // [M2]
  const u32x4* wsb[kTrunkMaxLayers];   // skip weights, bf16x3 A operands with the k order of the resident layout
  const float* bias[kTrunkMaxLayers];
  const float2* wt[kTrunkMaxLayers];   // [M2][M1][32][32]
  float* xpart;        // [S][G][M2][M1][2][32]
  float* obuf;         // [S][M2][M1][2][32]
  long long xpart_par, obuf_par;   // LL protocol: distance (floats) to the second (odd-layer) copy of each buffer
  unsigned layer0;     // LL protocol: spectral layers already run on these buffers since they were armed
  unsigned* xcc_tab;   // LL protocol: [S][32] (tag << 4 | XCC id) of every workgroup of a sample's group
  unsigned* ctr;       // one counter per sample, 32 dwords apart
  unsigned epoch;      // barriers already counted on these counters
  float fwd_scale;
  int S, H, L, M1, M2, G, sample0;
  unsigned long long* trace;   // diagnostics (DLWP_TRUNK_TRACE): [workgroup][64] s_memrealtime stamps, or null
  int trace_tid;               // the thread that stamps (DLWP_TRUNK_TRACE_WAVE * 64)
  // STEP variant (lifting and projection inside the same launch):
  ChanTable in;            // the step's input channels (folds _prepare_inputs)
  int lift_ns, lift_hid;   // populated 4-deep k-steps of the input (<= 4), lifting width (<= 256, multiple of 32)
  int lift_cin1;           // exactly one input channel: lifting layer 1 as plain FMAs (lift_segment)
  const float* lift_w1p;   // [hid/16][ns][64]
  const float* lift_b1;    // [hid]
  const u32x4* lift_w2b;   // [hid/32][3][2][64]
  const float* lift_b2;    // [32]
  const float* lift_tab;   // one input channel: the lifting MLP tabulated (lift_from_table), or null = evaluate it (lift_segment)
  float lift_up, lift_down, proj_up, proj_down;   // f16x3 form: 2^(11+s) of the lifting W2 / projection W1 images and its inverse
  int proj_hid, proj_co, cout;   // projection width (<= 256), outputs the FMA layer 2 is built for (1, 2, 4), real outputs
  const u32x4* proj_w1b;   // [hid/16][3][64], k order of the resident activation
  const float* proj_b1;    // [hid]
  const float* proj_w2v;   // [hid/16][proj_co][16]
  const float* proj_b2;    // [16]
  float* out;              // out + b * out_bstride + co * H * W
  long long out_bstride;
  const float* resid;      // or null
  long long resid_bstride;
  // several steps in this launch (n_steps > 1): the per-step tables above are rebuilt on the device from
  const float* r_const;    // constants  [B, 1, n_const, H, W] or null
  const float* r_presc;    // prescribed [B, T, n_presc, H, W] or null
  const float* r_prog;     // prognostic [B, T, n_prog, H, W]
  float* r_out;            // out        [B, T - ctx, n_prog, H, W]
  int r_nconst, r_npresc, r_nprog, r_T, r_ctx, r_t0;   // first time index of this launch (ctx + step_begin)
  int feed_regs;           // n_steps > 1, no constants / prescribed channels, context 1, <= 4 prognostic channels: a step's whole
                           // input (and its residual) is the output the SAME lanes have just computed -- it stays in registers
  int n_steps;             // 0 / 1: one step described by in / out / resid
  // hand-off bounds (plan knobs): polls of a counter barrier / re-loads of a flag-in-data block before the workgroup
  // gives up; a workgroup that gives up poisons its outputs with NaN AND sets *fail_word (checked by the host)
  int spin_limit, try_limit;
  unsigned* fail_word;     // workspace word, zeroed at the start of every call (per-call check)
  unsigned* sticky_fails;  // plan-owned counter, only reset by dlwp_fno2d_status (deferred check of asynchronous calls)
};

__device__ __forceinline__ void trunk_group_barrier(unsigned* ctr, unsigned target, int* s_fail, int spin_limit) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_waitcnt(0);   // this wave's sc1 stores have reached the coherence point
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int spins = 0;
    while ((int)(__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) < 0) {
      __builtin_amdgcn_s_sleep(1);
      if (++spins > spin_limit) {   // default ~ 0.1 s: a peer workgroup never arrived; give up loudly, never hang
        *s_fail = 1;
        break;
      }
    }
  }
  __syncthreads();
}

// Split form: arrive (stores drained, one lane adds) ... independent work ... wait.
__device__ __forceinline__ void trunk_group_arrive(unsigned* ctr) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void trunk_group_wait(unsigned* ctr, unsigned target, int* s_fail, int spin_limit) {
  if (threadIdx.x == 0) {
    int spins = 0;
    while ((int)(__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) < 0) {
      __builtin_amdgcn_s_sleep(1);
      if (++spins > spin_limit) {
        *s_fail = 1;
        break;
      }
    }
  }
  __syncthreads();
}

__device__ __forceinline__ float ld_sc1(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_sc1(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Four independent 16-byte agent-scope (sc1: L1 bypass) loads in flight at once, then one wait.  hipcc puts
// `s_waitcnt vmcnt(0)` behind EVERY relaxed atomic load, which turned the 12-16 hand-off loads of a phase into
// as many serialized round trips to the Infinity Cache (first version of this kernel: P2 4.3 us, P3 2.9 us).
__device__ __forceinline__ void ld4_sc1_x4(const float* base, unsigned o0, unsigned o1, unsigned o2, unsigned o3,
                                           f32x4& v0, f32x4& v1, f32x4& v2, f32x4& v3) {
  // s_nop 4: the base may have just been restored into SGPRs by v_readlane / v_readfirstlane (SGPR spills), and a
  // VALU-written SGPR needs 5 wait states before a VMEM instruction reads it; the compiler's hazard recognizer
  // does not look inside inline asm (a build without this faulted with a garbage address).
  asm volatile(
      "s_nop 4\n\t"
      "global_load_dwordx4 %0, %4, %8 sc1\n\t"
      "global_load_dwordx4 %1, %5, %8 sc1\n\t"
      "global_load_dwordx4 %2, %6, %8 sc1\n\t"
      "global_load_dwordx4 %3, %7, %8 sc1\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3)
      : "v"(o0), "v"(o1), "v"(o2), "v"(o3), "s"(base)
      : "memory");
}
// Flag-in-data hand-off ("LL" protocol): the exchange buffers are armed with a sentinel bit pattern (a quiet NaN with a
// payload no arithmetic produces); a consumer re-loads until none of the dwords it needs is the sentinel, so the data
// itself is the flag: no store drain, no counter round trip, no workgroup barrier on the producer side.
constexpr unsigned kSentinel = 0x7fc0deadu;
__device__ __forceinline__ bool has_sentinel(const f32x4& v) {
  return __float_as_uint(v[0]) == kSentinel || __float_as_uint(v[1]) == kSentinel ||
         __float_as_uint(v[2]) == kSentinel || __float_as_uint(v[3]) == kSentinel;
}
// The closing `s_nop 1`: a 16-byte store reads its data registers late, and the compiler -- which sees the statement as one
// opaque instruction -- may overwrite them in the very next instruction (cdna_hip_programming.md 5.7 item 1).  Found in
// this file by tools/asm_hazard_check.py (rule C) in round 2: the re-arming sentinel stores were followed one wait state
// later by a VALU write to one of the four data registers.
__device__ __forceinline__ void st4_sc1(const float* base, unsigned off, const f32x4& v) {
  asm volatile("s_nop 4\n\tglobal_store_dwordx4 %0, %1, %2 sc1\n\ts_nop 1" : : "v"(off), "v"(v), "s"(base) : "memory");
}
__device__ __forceinline__ void st4_l2(const float* base, unsigned off, const f32x4& v) {   // stays in this XCD's L2
  asm volatile("s_nop 4\n\tglobal_store_dwordx4 %0, %1, %2\n\ts_nop 1" : : "v"(off), "v"(v), "s"(base) : "memory");
}
// Exchange stores of the flag-in-data protocol.  `fast` = every workgroup of the sample's group was FOUND to sit on the
// same XCD (HW_REG_XCC_ID exchanged during the first layer): a plain store keeps the line in that XCD's L2, where the
// group's L1-bypassing (sc1) loads hit it after ~0.2 us instead of going to the Infinity Cache (~0.9 us round trip).
// Otherwise the write-through sc1 form that is correct across XCDs.
__device__ __forceinline__ void st_xchg(float* p, float v, bool fast) {
  if (fast) *p = v;   // (not volatile: hipcc turns volatile stores into sc0 sc1 + a wait each, 6x slower)
  else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains vmcnt, i.e. it would wait for the
// weight prefetches that are meant to stay in flight across the barrier.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
// s_waitcnt immediate of gfx9 / CDNA: vmcnt = bits [3:0] and [15:14], expcnt = [6:4], lgkmcnt = [11:8].  vmcnt(0) alone: the other
// two counters at their maxima (no wait).  Given as a builtin, not inline asm: hipcc's wait-count model reads it.  Where the step
// loop uses it the wait only chooses WHERE the compiler waits (inside a rare branch, not where branches meet): correctness never
// depends on it and no measured gain rests on it (DESIGN.md section 4.6 "Step I/O": 1.0838 ms per launch with and without).
constexpr int kWaitVm0 = 0x0F70;
__device__ __forceinline__ f32x4 shfl_xor4(f32x4 v, int m) {
  return f32x4{__shfl_xor(v[0], m), __shfl_xor(v[1], m), __shfl_xor(v[2], m), __shfl_xor(v[3], m)};
}

// ROWS = grid rows (= waves) per workgroup, G = workgroups per sample = H / ROWS (see trunk_rows() for the choice).
// Output slot / input table / residual of rollout step t, exactly as fno_rollout_impl builds them on the host
// (fno.py:49-62, :79-103).  Three functions, each called only where its result is read: a step whose input and residual are
// still in registers (feed_regs) needs the output slot alone -- scalar multiplies in front of its one store.
__device__ __forceinline__ void rollout_step_out(const TrunkParams& p, int t, long long HW, float*& out, long long& out_bs) {
  out_bs = (long long)(p.r_T - p.r_ctx) * p.r_nprog * HW;
  out = p.r_out + (long long)(t - p.r_ctx) * p.r_nprog * HW;
}
// The window in FIXED slots: constants, prescribed[t-ctx:t], prognostic frames still taken from the input, frames already
// produced.  A part the step does not have is a slot of zero channels (chan_ptr skips it wherever it sits; its pointer is
// never formed into an address), so no slot is chosen by a run-time index and the table needs no private memory.
__device__ __forceinline__ void rollout_step_table(const TrunkParams& p, int t, long long HW, ChanTable& in) {
  const int T = p.r_T, ctx = p.r_ctx;
  const int f0 = t - ctx;
  const int n_in = (f0 < ctx) ? (ctx - f0 < ctx ? ctx - f0 : ctx) : 0;
  const int fo = f0 + n_in - ctx;   // first produced frame of the window; >= 0 always (0 while input frames remain, f0 - ctx after)
  in.seg[0] = ChanSeg{p.r_const, (long long)p.r_nconst * HW, p.r_nconst, 0};
  in.seg[1] = ChanSeg{p.r_presc + (long long)f0 * p.r_npresc * HW, (long long)T * p.r_npresc * HW, p.r_npresc * ctx, 0};
  in.seg[2] = ChanSeg{p.r_prog + (long long)f0 * p.r_nprog * HW, (long long)T * p.r_nprog * HW, p.r_nprog * n_in, 0};
  in.seg[3] = ChanSeg{p.r_out + (long long)fo * p.r_nprog * HW, (long long)(T - ctx) * p.r_nprog * HW, p.r_nprog * (ctx - n_in), 0};
}
// The residual: frame t - 1, from the input while t - 1 < ctx, from the frames already produced afterwards.
__device__ __forceinline__ void rollout_step_resid(const TrunkParams& p, int t, long long HW, const float*& resid, long long& resid_bs) {
  const int T = p.r_T, ctx = p.r_ctx;
  if (t - 1 < ctx) { resid = p.r_prog + (long long)(t - 1) * p.r_nprog * HW; resid_bs = (long long)T * p.r_nprog * HW; }
  else { resid = p.r_out + (long long)(t - 1 - ctx) * p.r_nprog * HW; resid_bs = (long long)(T - ctx) * p.r_nprog * HW; }
}

// STEP: the whole backbone step in this launch -- the lifting MLP produces the resident activation and its first Y row,
// the projection MLP (+ residual) consumes the last one; their staged weights time-share the transpose tiles' LDS.
// Forward W-direction DFT of the wave's 32 x 64 tile in its transpose area on the f16 matrix instructions (f16x3 step kernel):
// A = 8 consecutive pixels of a channel row (two 16-byte LDS reads, split on the fly), B = the pre-split twiddles.
// The bf16x6 kernels keep both W-direction DFTs on fp32 MFMA (exact fp32 FMA chains): the bf16x6 form of them was built,
// parity-green and measured NO gain (inverse 0.77 vs 0.88 us, forward 0.72 vs 0.76 us for the first wave of a SIMD, launch 1.891
// vs 1.887 ms) -- K is only 16 / 64 deep, so the extra LDS reads, the 11-slot splits and the six dependent MFMAs per
// accumulator cost what the freed fp32 lanes give back.  f16x3 halves both.
__device__ __forceinline__ void fwd_dft_f16x3(const float* s_tr, const u32x4* s_ttb, int lane, f32x4 (&yacc)[2]) {
  const int j = lane & 15, g = lane >> 4;
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
    u32x4 tb[3];
#pragma unroll
    for (int pp = 0; pp < 3; ++pp) tb[pp] = s_ttb[(kb * 3 + pp) * 64 + lane];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const float* src = s_tr + (16 * ct + j) * kTrStride + 32 * kb + 8 * g;
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(src), a1 = *reinterpret_cast<const f32x4*>(src + 4);
      u32x4 xa[3];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        unsigned hh, mm, ll;
        const float v0 = i < 2 ? a0[2 * i] : a1[2 * i - 4], v1 = i < 2 ? a0[2 * i + 1] : a1[2 * i - 3];
        split_pair_x<true>(v0, v1, hh, mm, ll);
        xa[0][i] = hh;
        xa[1][i] = mm;
        xa[2][i] = ll;
      }
      // data on the A side, 2^(11+3) times the true scale (kTrunkF16Down): (xh, tm') (xm', th) (xh, thB)
      yacc[ct] = mfma16x16x32_f16(xa[0], tb[1], yacc[ct]);
      yacc[ct] = mfma16x16x32_f16(xa[1], tb[0], yacc[ct]);
      yacc[ct] = mfma16x16x32_f16(xa[0], tb[2], yacc[ct]);
    }
  }
}

template <int ROWS, int G, bool LL, bool STEP = false, bool F16 = false>
__global__ __launch_bounds__(64 * ROWS, 2) void fno_trunk_kernel(const TrunkParams p) {
  extern __shared__ __align__(16) float smem[];
  constexpr int W = 64, KP = 16, C = kC, NT = 64 * ROWS;
  // F16 (f16x3): the W-direction DFTs of the row phase run on the f16 matrix instructions too -- the skip convolution and the
  // inverse W-DFT share one SCALED accumulator (common.hpp); otherwise they are fp32 MFMA (see fwd_dft_f16x3)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, g = lane >> 4;
  float* s_tr = smem + wave * (C * kTrStride);            // [8][32][68]   per-wave transpose tile
  float* s_y = smem + ROWS * C * kTrStride;               // [ROWS][528]   Y rows of this workgroup
  float* s_z = s_y + ROWS * kSyStride;                    // [ROWS][16][32] Z rows of this workgroup
  float* s_x = s_z + ROWS * KP * C;                       // [ROWS][2][64] per-wave reduced X of two modes
  float* s_t = s_x + ROWS * 128;                             // [16][64]      T  (inverse W-DFT twiddles)
  float* s_tt = s_t + KP * W;                             // [64][16]      TT (forward W-DFT twiddles)
  int* s_fail = reinterpret_cast<int*>(s_tt + W * KP);
  int* s_fast = s_fail + 1;                               // LL: the sample's group shares one XCD (found in layer 0)
  int* s_lflag = s_fail + 2;                              // STEP: [2] some wave evaluates the exact lifting MLP (by step parity)
  float2* s_ef = reinterpret_cast<float2*>(s_fail + 4);   // [16][ROWS]  EF rows of this workgroup's grid rows (0 beyond M1)
  float2* s_ei = s_ef + 16 * ROWS;                        // [16][ROWS]  EI likewise
  u32x4* s_tb = reinterpret_cast<u32x4*>(s_ei + 16 * ROWS);   // [4][3][64]  inverse W-DFT B operands (bf16x3)
  u32x4* s_ttb = s_tb + 4 * 3 * 64;                           // [2][3][64]  forward W-DFT B operands (bf16x3)
  const int H = p.H, M1 = p.M1, M2 = p.M2, NM = M1 * M2;
  int sample, member;
  {
    const int i = blockIdx.x;
    if ((p.S & 7) == 0) {          // a sample's workgroups share an XCD (workgroup i -> XCD i % 8)
      const int slot = i >> 3;
      sample = (i & 7) + 8 * (slot / G);
      member = slot % G;
    } else {
      sample = i / G;
      member = i % G;
    }
  }
  const int h = member * ROWS + wave;
  const long long HW = (long long)H * W;
  const int gs = p.sample0 + sample;                      // sample index in the activation tensors
  const long long pix = (long long)h * W + 4 * j;
  // g, s_tr and pix are shadowed by the step loop's own (derived there from an opaque thread index) and never read; they
  // stay because the generated code of the kernel depends on them being here (taking them out moves `member * ROWS` in all
  // 18 instantiations): whoever removes them checks the kernels with tools/kernel_isa_diff.py against the previous build
  (void)g; (void)s_tr; (void)pix;
  unsigned* ctr = p.ctr + sample * 32;
  if (tid == 0) {
    *s_fail = 0;
    *s_fast = 0;
    s_lflag[0] = s_lflag[1] = 0;
    if (LL) {
      const unsigned xcc = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11)) & 0xFu;   // HW_REG_XCC_ID
      __hip_atomic_store(p.xcc_tab + sample * 32 + member, ((p.layer0 + 1u) << 4) | xcc, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  for (int i = tid; i < ROWS * KP * C; i += NT) s_z[i] = 0.f;   // k' slots beyond 2*M2 stay zero
  for (int i = tid; i < KP * W; i += NT) {
    s_t[i] = p.t[i];
    s_tt[i] = p.tt[i];
  }
  for (int i = tid; i < 16 * ROWS; i += NT) {   // the persistent form re-derives its MFMA operands from these every step
    const int r = i / ROWS, hl = i % ROWS;
    s_ef[i] = r < M1 ? p.ef[r * H + member * ROWS + hl] : float2{0.f, 0.f};
    s_ei[i] = r < M1 ? p.ei[r * H + member * ROWS + hl] : float2{0.f, 0.f};
  }
  for (int i = tid; i < 4 * 3 * 64; i += NT) s_tb[i] = p.tb[i];
  for (int i = tid; i < 2 * 3 * 64; i += NT) s_ttb[i] = p.ttb[i];
  lds_barrier();   // the tables above are read by every wave right away

  // STEP: the steps of this launch (one, or a whole rollout range without the host in the loop: a row's next input
  // is what the same wave has just written, so steps need no synchronisation beyond the spectrum hand-offs)
  int n_stamp = 0;
  const int n_steps = (STEP && p.n_steps > 1) ? p.n_steps : 1;
  f32x4 vfeed = {0.f, 0.f, 0.f, 0.f};   // feed_regs: the previous step's output of this lane (channel g, pixels 4j..4j+3)
  // no live table: the lifting weights of the NEXT step are requested before the end-of-step barrier and written to LDS
  // behind it (staged = they are already there when the step starts)
  bool staged = false;
  for (int st = 0; st < n_steps; ++st) {
  // Everything lane-dependent is re-derived from an OPAQUE copy of the thread index inside the step loop: otherwise
  // hipcc hoists the step-invariant address arithmetic and MFMA operands of all phases out of the loop, keeps them
  // live across the lifting MLP and spills ~160 VGPRs per lane to scratch (664 bytes/lane in the first version).
  int tid_o = threadIdx.x;
  asm volatile("" : "+v"(tid_o));
  const int tid = tid_o, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  float* s_tr = smem + wave * (C * kTrStride);
  const int h = member * ROWS + wave;
  const long long pix = (long long)h * W + 4 * j;
  // no step I/O here: the input table, the residual pointer and the output slot are formed where they are read (the lifting's
  // loads, the projection's tail), so a step fed from registers builds no table and the top of the loop touches no memory
  // resident activation: vv[ot][r] = channel 16 ot + 4 g + r, pixels 4j..4j+3
  f32x4 vv[2][4];
  if constexpr (STEP) {
    // ---- lifting: weights staged where the transpose tiles will live (they are not needed before the first DFT)
    if (p.trace && tid == p.trace_tid && n_stamp < 64) p.trace[blockIdx.x * 64 + n_stamp++] = __builtin_amdgcn_s_memrealtime();
    const int ntile_l = p.lift_hid >> 4, npair = ntile_l >> 1;
    u32x4* l_w2 = reinterpret_cast<u32x4*>(smem);                          // [npair][3][2][64]
    float* l_w1 = reinterpret_cast<float*>(l_w2 + npair * 6 * 64);         // [ntile][ns][64]
    float* l_b1 = l_w1 + ntile_l * p.lift_ns * 64;                         // [hid]
    auto lift_stage = [&]() {
      for (int i = tid; i < npair * 6 * 64; i += NT) l_w2[i] = p.lift_w2b[i];
      for (int i = tid; i < ntile_l * p.lift_ns * 64; i += NT) l_w1[i] = p.lift_w1p[i];
      for (int i = tid; i < p.lift_hid; i += NT) l_b1[i] = p.lift_b1[i];
    };
    auto lift_stage_voted = [&]() {   // the same copy, rolled: rare, its latency is exposed anyway, and the step's input is live
#pragma unroll 1
      for (int i = tid; i < npair * 6 * 64; i += NT) l_w2[i] = p.lift_w2b[i];
#pragma unroll 1
      for (int i = tid; i < ntile_l * p.lift_ns * 64; i += NT) l_w1[i] = p.lift_w1p[i];
#pragma unroll 1
      for (int i = tid; i < p.lift_hid; i += NT) l_b1[i] = p.lift_b1[i];
    };
    // vote: with a live table the exact path's weights are staged only in a step in which some wave of the workgroup
    // falls back to it.  Every wave knows its next input row BEFORE the barrier of the step seam (the one that ends the
    // previous projection's reads of this LDS region), so a wave that will fall back raises a flag in front of that barrier
    // and every wave reads it behind it.  No flag: no weight request, no LDS write, and this barrier is the only one
    // between the projection and the transpose tiles.  Two flag words alternate by step: the word of step s is written
    // before and read behind the seam barrier of step s, and cleared behind the seam barrier of step s - 1 -- the
    // barriers of the spectral layers and of the projection lie between that clear and the next write.
    const bool vote = p.lift_tab != nullptr;
    if (!vote && !staged) lift_stage();
    f32x4 xs[4];
    if (p.feed_regs && st > 0) {
      xs[0] = vfeed;
#pragma unroll
      for (int s = 1; s < 4; ++s) xs[s] = f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
      ChanTable in;
      if (p.n_steps > 1) rollout_step_table(p, p.r_t0 + st, HW, in);
      else in = p.in;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float* cp = s < p.lift_ns ? chan_ptr(in, 4 * s + g, gs, (int)HW) : nullptr;
        xs[s] = cp ? *reinterpret_cast<const f32x4*>(cp + pix) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
      // vmcnt(0), spelled out in THIS branch: otherwise hipcc waits for these loads where the branches meet, in front of the
      // vote, and a fed step drains its previous output store there (one in-order counter for loads and stores).  Kept for the
      // listing of the fed path (no full wait in front of the vote); not measurable on its own (kWaitVm0)
      __builtin_amdgcn_s_waitcnt(kWaitVm0);
    }
    // layer-2 bias of the exact MLP: requested here only when every step evaluates it; a voting step asks for it once it
    // falls back, for the same reason -- no load may be in flight, behind the output store, when the vote reads the input
    // (like the waits: for the fed path's listing, no measured gain)
    f32x4 bias2[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    auto lift_bias2 = [&]() {
      bias2[0] = *reinterpret_cast<const f32x4*>(p.lift_b2 + 4 * g);
      bias2[1] = *reinterpret_cast<const f32x4*>(p.lift_b2 + 16 + 4 * g);
    };
    if (!vote) lift_bias2();
    // One input channel and a table from the plan: the wave reads lift(x) from it when EVERY pixel of its row lies inside the
    // table's domain (one ballot; NaN and +-inf fail the test) and evaluates the MLP as before otherwise -- the decision
    // depends on the row's own data only, and no load address is formed from an unchecked x.
    bool from_table = false;
    f32x4 xp = {0.f, 0.f, 0.f, 0.f};
    auto lift_pick = [&]() {
      // The gather runs in a PERMUTED lane order: lane 4 j' + g' reads what resident lane (j', g') needs, so the four lanes
      // of a pixel are neighbours and their 16-byte loads cover 64 contiguous bytes of one line (one tag look-up instead of
      // four: in the resident order every lane of a 16-lane pass touched a line of its own and the phase ran at the L1's
      // look-up rate, 11 us instead of the 2.6 us its bytes need).  The channel's pixels sit in lane group g = 0.
      bool inside = true;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        xp[q] = __shfl(xs[0][q], lane >> 2);
        inside = inside && (fabsf(xp[q]) < (float)kLiftTabRange);
      }
      from_table = __all(inside) != 0;
    };
    auto lift_gather = [&]() {
      f32x4 vp[2][4];
      lift_from_table(p.lift_tab, xp, lane & 3, vp);
#pragma unroll
      for (int ot = 0; ot < 2; ++ot)   // back to the resident order: lane (j, g) takes its values from lane 4 j + g
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int q = 0; q < 4; ++q) vv[ot][r][q] = __shfl(vp[ot][r][q], 4 * j + g);
    };
    auto lift_exact = [&]() {
      f32x4 acc2[2][4];
      lift_segment<4, F16>(xs, l_w1, l_b1, l_w2, npair, lane, bias2, acc2, p.lift_ns, p.lift_cin1 != 0, p.lift_up, p.lift_down);
#pragma unroll
      for (int ot = 0; ot < 2; ++ot)
#pragma unroll
        for (int r = 0; r < 4; ++r) vv[ot][r] = f32x4{acc2[ot][0][r], acc2[ot][1][r], acc2[ot][2][r], acc2[ot][3][r]};
    };
#define DLWP_LIFT_STAMP()                                                                              \
  do {                                                                                                 \
    if (p.trace && tid == p.trace_tid && n_stamp < 64) p.trace[blockIdx.x * 64 + n_stamp++] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
    if (vote) {
      lift_pick();
      if (!from_table) s_lflag[st & 1] = 1;
    }
    // (the gather needs no LDS, but running it BEFORE the seam barrier, while slower waves finish their projection, cost
    // 304 instead of 184 bytes of scratch per lane -- DESIGN.md section 4.6)
    bool weights_used = true;   // the exact path's weights are in LDS (or on their way) and some wave may read them
    if (vote) {
      DLWP_LIFT_STAMP();
      lds_barrier();   // the seam: every wave is done with the projection weights, every flag of this step is up
      weights_used = __builtin_amdgcn_readfirstlane(s_lflag[st & 1]) != 0;
      if (tid == 0) s_lflag[(st + 1) & 1] = 0;
    }
    if (vote && weights_used) lift_stage_voted();
    if (weights_used) lds_barrier();
    DLWP_LIFT_STAMP();
    if (!from_table) {
      if (vote) lift_bias2();
      lift_exact();
    } else {
      lift_gather();
    }
    if (!vote) DLWP_LIFT_STAMP();
    if (weights_used) lds_barrier();   // every wave is done with the lifting weights: the region turns into transpose tiles
    DLWP_LIFT_STAMP();
#undef DLWP_LIFT_STAMP
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        *reinterpret_cast<f32x4*>(s_tr + (16 * ot + 4 * g + r) * kTrStride + 4 * j) = vv[ot][r];
    wave_lds_fence();
    f32x4 yacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    if constexpr (F16) {
      fwd_dft_f16x3(s_tr, s_ttb, lane, yacc);
    } else {
#pragma unroll
      for (int s = 0; s < 16; ++s)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
          yacc[ct] = mfma16x16x4(s_tr[(16 * ct + j) * kTrStride + 4 * s + g], s_tt[(4 * s + g) * KP + j], yacc[ct]);
    }
    wave_lds_fence();
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
      *reinterpret_cast<f32x4*>(s_y + wave * kSyStride + j * C + 16 * ct + 4 * g) = F16 ? yacc[ct] * kTrunkF16Down : yacc[ct];
    if (p.trace && tid == p.trace_tid && n_stamp < 64) p.trace[blockIdx.x * 64 + n_stamp++] = __builtin_amdgcn_s_memrealtime();
  } else {
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        vv[ot][r] = *reinterpret_cast<const f32x4*>(p.x + ((long long)gs * C + 16 * ot + 4 * g + r) * HW + pix);
    const float* yr = p.ybuf + ((long long)gs * H + h) * KP * C;
#pragma unroll
    for (int u = 0; u < 2; ++u)
      *reinterpret_cast<f32x4*>(s_y + wave * kSyStride + 4 * lane + 256 * u) =
          *reinterpret_cast<const f32x4*>(yr + 4 * lane + 256 * u);
  }
  // loop-invariant operands
  constexpr int KS1 = ROWS / 2;   // k-steps of P1: K = (ROWS rows) x (re, im)
  float a_re[KS1], a_im[KS1];   // P1: A[(r = j)][k = (hl, ri)], hl = 2s + (g >> 1), ri = g & 1
#pragma unroll
  for (int s = 0; s < KS1; ++s) {
    const int hl = 2 * s + (g >> 1);
    float2 e = {0.f, 0.f};
    if (j < M1) e = s_ef[j * ROWS + hl];
    a_re[s] = (g & 1) ? -e.y : e.x;
    a_im[s] = (g & 1) ? e.x : e.y;
  }
  float a3[8];              // P3: A[m = (hl = j >> 1, ro = j & 1)][k = (r, ri)], r = 2s + (g >> 1), ri = g & 1
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const int r = 2 * s + (g >> 1);
    float2 e = {0.f, 0.f};
    if (r < M1 && (j >> 1) < ROWS) e = s_ei[r * ROWS + (j >> 1)];
    a3[s] = (j & 1) ? ((g & 1) ? e.x : e.y) : ((g & 1) ? -e.y : e.x);
  }
  const int ks3 = (2 * M1 + 3) / 4;
  const int per = (NM + G - 1) / G;                       // modes per workgroup in P2
  const int m_lo = member * per, m_hi = (m_lo + per < NM) ? m_lo + per : NM;
  // LL: the exchange buffers exist twice (layer parity), p.xpart / p.obuf point at parity 0 and the second copy
  // lies p.xpart_par / p.obuf_par floats further
  float* xp_mine0 = p.xpart + ((long long)sample * G + member) * NM * 64;
  const float* xp_grp0 = p.xpart + (long long)sample * G * NM * 64;
  float* ob0 = p.obuf + (long long)sample * NM * 64;
  unsigned target = p.epoch * (unsigned)G;

#define DLWP_STAMP()                                                                                   \
  do {                                                                                                 \
    if (p.trace && tid == p.trace_tid && n_stamp < 64) p.trace[blockIdx.x * 64 + n_stamp++] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
  // Polls of a hand-off: the traced wave leaves the poll issue that delivered its block (1 = the first; the last block of the
  // phase counts) in bits 56-63 of the slot of the phase's closing stamp, which is then OR-ed in (the 100 MHz counter does not
  // reach those bits; the buffer is zeroed before the launch; tools/trunk_trace.py).  Nothing is carried in registers.
  // Counted in the step kernel only: in the plain trunk the two extra stores cost <4, 32, true> eight more spilled dwords.
#define DLWP_STAMP_POLLS(n)                                                                            \
  do {                                                                                                 \
    if (STEP && p.trace && tid == p.trace_tid && n_stamp < 64)                                         \
      p.trace[blockIdx.x * 64 + n_stamp] = (unsigned long long)((n) < 255 ? (n) : 255) << 56;          \
  } while (0)
#define DLWP_STAMP_OR()                                                                                \
  do {                                                                                                 \
    if (p.trace && tid == p.trace_tid && n_stamp < 64) p.trace[blockIdx.x * 64 + n_stamp++] |= __builtin_amdgcn_s_memrealtime(); \
  } while (0)
  DLWP_STAMP();

  for (int l = 0; l < p.L; ++l) {
    const int par = LL ? (int)((p.layer0 + (unsigned)(st * p.L + l)) & 1u) : 0;
    float* xp_mine = xp_mine0 + par * p.xpart_par;
    const float* xp_grp = xp_grp0 + par * p.xpart_par;
    float* ob = ob0 + par * p.obuf_par;
    float* ob_other = ob0 + (par ^ 1) * p.obuf_par;
    if (LL) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's re-arming stores of the previous layer are done
    const bool fast = LL && (l > 0 || st > 0) && (*s_fast != 0);
    // operands that do not depend on data are requested before the barriers: the skip weights / bias of the row
    // phase and the weights of this wave's first two modes
    u32x4 wb[2][3];
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
      for (int pp = 0; pp < 3; ++pp) wb[ot][pp] = p.wsb[l][(ot * 3 + pp) * 64 + lane];
    f32x4 bias4[2];
#pragma unroll
    for (int ot = 0; ot < 2; ++ot) bias4[ot] = *reinterpret_cast<const f32x4*>(p.bias[l] + 16 * ot + 4 * g);
    float2 wreg[2][16];
    {
      const int m = m_lo + wave;
      const float2* w = p.wt[l] + ((long long)(m < m_hi ? m : 0) * C + (lane >> 5) * 16) * C + (lane & 31);
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) wreg[0][cc] = w[cc * C];
    }
    lds_barrier();   // s_y complete (all rows of the workgroup)
    DLWP_STAMP();
    // ---- P1: partial H-direction DFT of the own rows, columns (ky = wave, wave + ROWS, ..; c)
    for (int ky = wave; ky < M2; ky += ROWS) {
      // the four accumulator chains (2 channel halves x re / im) interleaved: a dependent fp32 matrix instruction waits ~40 cycles
      f32x4 dre[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}}, dim[2] = {dre[0], dre[0]};
#pragma unroll
      for (int s = 0; s < KS1; ++s) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          const float b = s_y[(2 * s + (g >> 1)) * kSyStride + (2 * ky + (g & 1)) * C + 16 * nt + j];
          dre[nt] = mfma16x16x4(a_re[s], b, dre[nt]);
          dim[nt] = mfma16x16x4(a_im[s], b, dim[nt]);
        }
      }
      // one wave-uniform decision for all 16 stores of the wave (st_xchg branched per store)
      auto publish = [&](auto fastc) {
        constexpr bool FAST = decltype(fastc)::value;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) {
            const int r = 4 * g + r4;
            if (r < M1) {
              float* dst = xp_mine + (long long)(ky * M1 + r) * 64 + 16 * nt + j;
              if constexpr (!LL) {
                st_sc1(dst, dre[nt][r4]);
                st_sc1(dst + 32, dim[nt][r4]);
              } else if constexpr (FAST) {
                dst[0] = dre[nt][r4];
                dst[32] = dim[nt][r4];
              } else {
                __hip_atomic_store(dst, dre[nt][r4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(dst + 32, dim[nt][r4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              }
            }
          }
      };
      if (fast) publish(std::true_type{}); else publish(std::false_type{});
    }
    DLWP_STAMP();
    target += (unsigned)G;
    if (!LL) trunk_group_arrive(ctr);
    // in the shadow of the barrier: the part of the row that does not need the spectrum, bias + 1x1 skip
    // convolution of the resident activation on the bf16 pipe (bf16x6)
    f32x4 acc[2][4];
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[ot][q] = F16 ? bias4[ot] * kTrunkF16Up : bias4[ot];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      u32x4 bx[3];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        unsigned hh, mm, ll;
        split_pair_x<F16>(vv[i >> 1][2 * (i & 1)][q], vv[i >> 1][2 * (i & 1) + 1][q], hh, mm, ll);
        bx[0][i] = hh;
        bx[1][i] = mm;
        bx[2][i] = ll;
      }
#pragma unroll
      for (int ot = 0; ot < 2; ++ot) acc[ot][q] = mfma_x<F16>(wb[ot], bx, acc[ot][q]);
    }
    if (!LL) trunk_group_wait(ctr, target, s_fail, p.spin_limit);
    DLWP_STAMP();
    // weights of the wave's second mode: requested now, they arrive while the partials are awaited.  Only by a wave that
    // has one (wave-uniform; at the headline shape three of a workgroup's eight): the requests stand in front of the poll
    // in the same in-order vmcnt.  The other waves' registers are zeroed, never read: left undefined they cost the headline
    // instantiation its spill-free allocation (DESIGN.md section 4.6 "hand-off polls")
    if (const int m = m_lo + wave + ROWS; m < m_hi) {
      const float2* w = p.wt[l] + ((long long)m * C + (lane >> 5) * 16) * C + (lane & 31);
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) wreg[1][cc] = w[cc * C];
    } else {
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) wreg[1][cc] = float2{0.f, 0.f};
    }
    // ---- P2: channel mixing of this workgroup's share of the modes, two modes per pass.
    // lane (q4 = lane >> 4, quad = lane & 15) fetches floats 4 quad..4 quad+3 of the partials q4, q4+4, ...
    for (int up = 0; up < 2; ++up) {
      const int ma = m_lo + wave + 2 * ROWS * up, mb = ma + ROWS;
      if (ma >= m_hi) break;
      const bool has_b = mb < m_hi;
      const int q4 = lane >> 4, quad = lane & 15;
      f32x4 sa = {0.f, 0.f, 0.f, 0.f}, sb = sa;
      constexpr int NI = (G + 3) / 4;   // partials per lane and mode
#pragma unroll
      for (int i0 = 0; i0 < NI; i0 += 2) {
        const int qa = q4 + 4 * i0, qb = q4 + 4 * (i0 + 1);
        const bool va = qa < G, vb = (i0 + 1 < NI) && qb < G;
        const unsigned oa0 = (unsigned)((((va ? qa : 0) * NM + ma) * 64 + 4 * quad) * 4);
        const unsigned oa1 = (unsigned)((((vb ? qb : 0) * NM + ma) * 64 + 4 * quad) * 4);
        const unsigned obo0 = (unsigned)((((va ? qa : 0) * NM + (has_b ? mb : ma)) * 64 + 4 * quad) * 4);
        const unsigned obo1 = (unsigned)((((vb ? qb : 0) * NM + (has_b ? mb : ma)) * 64 + 4 * quad) * 4);
        f32x4 v0, v1, v2, v3;
        ld4_sc1_x4(xp_grp, oa0, oa1, obo0, obo1, v0, v1, v2, v3);
        if (LL) {
          int tries = 0;
          while (__any((va && (has_sentinel(v0) || has_sentinel(v2))) || (vb && (has_sentinel(v1) || has_sentinel(v3))))) {
            if (++tries > p.try_limit) {
              *s_fail = 1;
              break;
            }
            __builtin_amdgcn_s_sleep(2);
            ld4_sc1_x4(xp_grp, oa0, oa1, obo0, obo1, v0, v1, v2, v3);
          }
          DLWP_STAMP_POLLS(tries + 1);
          // re-arm what was consumed (this wave is the only reader of these modes' partials)
          const f32x4 sent4 = {__uint_as_float(kSentinel), __uint_as_float(kSentinel), __uint_as_float(kSentinel),
                               __uint_as_float(kSentinel)};
          if (fast) {
            if (va) {
              st4_l2(xp_grp, oa0, sent4);
              if (has_b) st4_l2(xp_grp, obo0, sent4);
            }
            if (vb) {
              st4_l2(xp_grp, oa1, sent4);
              if (has_b) st4_l2(xp_grp, obo1, sent4);
            }
          } else {
            if (va) {
              st4_sc1(xp_grp, oa0, sent4);
              if (has_b) st4_sc1(xp_grp, obo0, sent4);
            }
            if (vb) {
              st4_sc1(xp_grp, oa1, sent4);
              if (has_b) st4_sc1(xp_grp, obo1, sent4);
            }
          }
        }
        if (va) { sa += v0; sb += v2; }
        if (vb) { sa += v1; sb += v3; }
      }
      sa += shfl_xor4(sa, 16);
      sb += shfl_xor4(sb, 16);
      sa += shfl_xor4(sa, 32);
      sb += shfl_xor4(sb, 32);
      if (lane < 16) {
        *reinterpret_cast<f32x4*>(s_x + wave * 128 + 4 * quad) = sa * p.fwd_scale;
        *reinterpret_cast<f32x4*>(s_x + wave * 128 + 64 + 4 * quad) = sb * p.fwd_scale;
      }
      wave_lds_fence();
      const int c0 = (lane >> 5) * 16;
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int m = a ? mb : ma;
        if (a && !has_b) break;
        const float* xr = s_x + wave * 128 + a * 64;
        float2 acc = {0.f, 0.f};
        if (up == 0) {
#pragma unroll
          for (int cc = 0; cc < 16; ++cc) acc = cfma(float2{xr[c0 + cc], xr[32 + c0 + cc]}, wreg[a][cc], acc);
        } else {
          const float2* w = p.wt[l] + ((long long)m * C + c0) * C + (lane & 31);
#pragma unroll
          for (int cc = 0; cc < 16; ++cc) acc = cfma(float2{xr[c0 + cc], xr[32 + c0 + cc]}, w[cc * C], acc);
        }
        acc.x += __shfl_xor(acc.x, 32);
        acc.y += __shfl_xor(acc.y, 32);
        if (LL) {
          st_xchg(ob_other + (long long)m * 64 + lane, __uint_as_float(kSentinel), fast);   // every reader of the older O is done
          st_xchg(ob + (long long)m * 64 + lane, lane < 32 ? acc.x : acc.y, fast);
        } else {
          st_sc1(ob + (long long)m * 64 + lane, lane < 32 ? acc.x : acc.y);
        }
      }
      wave_lds_fence();
    }
    DLWP_STAMP_OR();
    target += (unsigned)G;
    if (!LL) trunk_group_barrier(ctr, target, s_fail, p.spin_limit);
    DLWP_STAMP();
    // ---- P3: inverse H-direction DFT for the own rows, columns (ky = wave, wave + ROWS, ..; o) -> s_z
    for (int ky = wave; ky < M2; ky += ROWS) {
      const float ckw = p.ck[ky];
      // O[ky = wave][r][re/im][o]: M1 * 64 floats, fetched with coalesced 16-byte loads into the (idle) transpose tile
      {
        const int nflt = M1 * 64;
        unsigned o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int f = 4 * lane + 256 * i;
          o[i] = (unsigned)((ky * nflt + (f < nflt ? f : 0)) * 4);
        }
        f32x4 v0, v1, v2, v3;
        ld4_sc1_x4(ob, o[0], o[1], o[2], o[3], v0, v1, v2, v3);
        if (LL) {
          const bool k0 = 4 * lane < nflt, k1 = 4 * lane + 256 < nflt, k2 = 4 * lane + 512 < nflt, k3 = 4 * lane + 768 < nflt;
          int tries = 0;
          while (__any((k0 && has_sentinel(v0)) || (k1 && has_sentinel(v1)) || (k2 && has_sentinel(v2)) ||
                       (k3 && has_sentinel(v3)))) {
            if (++tries > p.try_limit) {
              *s_fail = 1;
              break;
            }
            __builtin_amdgcn_s_sleep(2);
            ld4_sc1_x4(ob, o[0], o[1], o[2], o[3], v0, v1, v2, v3);
          }
          DLWP_STAMP_POLLS(tries + 1);
        }
        if (LL && l == 0 && st == 0 && wave == 0 && ky == 0) {
          // O of layer 0 has arrived, so every workgroup of the group has run and published its XCC id: does the
          // whole group share this XCD?  (decides the store flavour of all later exchanges, see st_xchg)
          const unsigned want = (p.layer0 + 1u) << 4;
          unsigned id = __hip_atomic_load(p.xcc_tab + sample * 32 + (lane < G ? lane : 0), __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT);
          int tries = 0;
          while (__any((id & ~0xFu) != want) && ++tries < 64)
            id = __hip_atomic_load(p.xcc_tab + sample * 32 + (lane < G ? lane : 0), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
          const unsigned id0 = (unsigned)__builtin_amdgcn_readfirstlane((int)id);
          const bool same = !__any(id != id0);
          if (lane == 0) *s_fast = same ? 1 : 0;
        }
        *reinterpret_cast<f32x4*>(s_tr + 4 * lane) = v0;
        *reinterpret_cast<f32x4*>(s_tr + 4 * lane + 256) = v1;
        *reinterpret_cast<f32x4*>(s_tr + 4 * lane + 512) = v2;
        *reinterpret_cast<f32x4*>(s_tr + 4 * lane + 768) = v3;
        wave_lds_fence();
      }
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          if (s < ks3) {
            const int r = 2 * s + (g >> 1);
            const float b = r < M1 ? s_tr[r * 64 + (g & 1) * 32 + 16 * nt + j] : 0.f;
            d = mfma16x16x4(a3[s], b, d);
          }
        }
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4)
          if (2 * g + (r4 >> 1) < ROWS) {
            const int kq = 2 * ky + (r4 & 1), o = 16 * nt + j;   // f16 form keeps Z as [row][o][k'], fp32 form as [row][k'][o]
            s_z[(2 * g + (r4 >> 1)) * (KP * C) + (F16 ? o * KP + kq : kq * C + o)] = d[r4] * ckw;
          }
      }
      wave_lds_fence();   // the transpose tile is reused for the next ky
    }
    lds_barrier();
    DLWP_STAMP_OR();
    // ---- the row itself
    if constexpr (F16) {
      // inverse W-DFT, f16x3: A = Z[o = 16 ot + j][k' = 8g .. 8g+7] (lane groups 2, 3 carry zeros: K = 16 of 32)
      u32x4 za[2][3];
#pragma unroll
      for (int ot = 0; ot < 2; ++ot) {
        f32x4 z0 = {0.f, 0.f, 0.f, 0.f}, z1 = z0;
        if (g < 2) {
          const float* src = s_z + wave * (KP * C) + (16 * ot + j) * KP + 8 * g;
          z0 = *reinterpret_cast<const f32x4*>(src);
          z1 = *reinterpret_cast<const f32x4*>(src + 4);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          unsigned hh, mm, ll;
          const float v0 = i < 2 ? z0[2 * i] : z1[2 * i - 4], v1 = i < 2 ? z0[2 * i + 1] : z1[2 * i - 3];
          split_pair_x<true>(v0, v1, hh, mm, ll);
          za[ot][0][i] = hh;
          za[ot][1][i] = mm;
          za[ot][2][i] = ll;
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        u32x4 tb[3];
#pragma unroll
        for (int pp = 0; pp < 3; ++pp) tb[pp] = s_tb[(q * 3 + pp) * 64 + lane];
#pragma unroll
        for (int ot = 0; ot < 2; ++ot) {   // data on the A side, at the accumulator's scale 2^14: (zh, tm') (zm', th) (zh, thB)
          acc[ot][q] = mfma16x16x32_f16(za[ot][0], tb[1], acc[ot][q]);
          acc[ot][q] = mfma16x16x32_f16(za[ot][1], tb[0], acc[ot][q]);
          acc[ot][q] = mfma16x16x32_f16(za[ot][0], tb[2], acc[ot][q]);
        }
      }
    } else {
      float z[KP / 4][2];
#pragma unroll
      for (int s = 0; s < KP / 4; ++s)
#pragma unroll
        for (int ot = 0; ot < 2; ++ot) z[s][ot] = s_z[wave * (KP * C) + (4 * s + g) * C + 16 * ot + j];
#pragma unroll
      for (int s = 0; s < KP / 4; ++s) {
        const f32x4 tw = *reinterpret_cast<const f32x4*>(s_t + (4 * s + g) * W + 4 * j);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int ot = 0; ot < 2; ++ot) acc[ot][q] = mfma16x16x4(z[s][ot], tw[q], acc[ot][q]);
      }
    }
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        vv[ot][r] = f32x4{acc[ot][0][r], acc[ot][1][r], acc[ot][2][r], acc[ot][3][r]};
        if constexpr (F16) vv[ot][r] *= kTrunkF16Down;     // skip convolution + inverse DFT + bias, back at the true scale
      }
    DLWP_STAMP();
    if (l < p.L - 1) {
      // neuralop FNOBlocks.forward_with_postactivation: GELU after every layer but the last
#pragma unroll
      for (int ot = 0; ot < 2; ++ot) {
        gelu_erf8(vv[ot][0], vv[ot][1]);
        gelu_erf8(vv[ot][2], vv[ot][3]);
      }
      DLWP_STAMP();
#pragma unroll
      for (int ot = 0; ot < 2; ++ot)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          *reinterpret_cast<f32x4*>(s_tr + (16 * ot + 4 * g + r) * kTrStride + 4 * j) = vv[ot][r];
      wave_lds_fence();
      DLWP_STAMP();
      f32x4 yacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      if constexpr (F16) {
        fwd_dft_f16x3(s_tr, s_ttb, lane, yacc);
      } else {
#pragma unroll
        for (int s = 0; s < 16; ++s)
#pragma unroll
          for (int ct = 0; ct < 2; ++ct)
            yacc[ct] = mfma16x16x4(s_tr[(16 * ct + j) * kTrStride + 4 * s + g], s_tt[(4 * s + g) * KP + j], yacc[ct]);
      }
      wave_lds_fence();
      DLWP_STAMP();
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
        *reinterpret_cast<f32x4*>(s_y + wave * kSyStride + j * C + 16 * ct + 4 * g) = F16 ? yacc[ct] * kTrunkF16Down : yacc[ct];
    }
  }
  DLWP_STAMP();
#undef DLWP_STAMP
#undef DLWP_STAMP_POLLS
#undef DLWP_STAMP_OR
  if (*s_fail) {
    // loud failure: the host reads this word after the launch (DLWP_ERR_TIMEOUT / re-run on the unfused kernels)
    if (tid == 0 && p.fail_word) {
      atomicOr(p.fail_word, 1u);
      atomicAdd(p.sticky_fails, 1u);   // (per poisoned step of a workgroup: any non-zero value means failure)
    }
    const float nanv = __uint_as_float(0x7fc00000u);
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
      for (int r = 0; r < 4; ++r) vv[ot][r] = f32x4{nanv, nanv, nanv, nanv};
  }
  if (STEP && p.proj_hid > 0) {
    // ---- projection (+ residual): weights staged over the transpose tiles, B operand straight from the registers
    // the projection weights are requested BEFORE the barrier that frees their LDS (they travel while the slower waves
    // finish their rows) and written behind it
    const int ntile_p = p.proj_hid >> 4;
    const int n_q1 = ntile_p * 3 * 64, n_q2 = ntile_p * p.proj_co * 16;
    u32x4 pq1[6];
    float pq2[2], pqb;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int i = tid + k * NT;
      pq1[k] = p.proj_w1b[i < n_q1 ? i : 0];
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int i = tid + k * NT;
      pq2[k] = p.proj_w2v[i < n_q2 ? i : 0];
    }
    pqb = p.proj_b1[tid < p.proj_hid ? tid : 0];
    lds_barrier();
    u32x4* q_w1 = reinterpret_cast<u32x4*>(smem);                          // [ntile][3][64]
    float* q_b1 = reinterpret_cast<float*>(q_w1 + ntile_p * 3 * 64);       // [hid]
    float* q_w2 = q_b1 + p.proj_hid;                                       // [ntile][co][16]
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int i = tid + k * NT;
      if (i < n_q1) q_w1[i] = pq1[k];
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int i = tid + k * NT;
      if (i < n_q2) q_w2[i] = pq2[k];
    }
    if (tid < p.proj_hid) q_b1[tid] = F16 ? pqb * p.proj_up : pqb;
    u32x4 bx[4][3];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        unsigned hh, mm, ll;
        split_pair_x<F16>(vv[i >> 1][2 * (i & 1)][q], vv[i >> 1][2 * (i & 1) + 1][q], hh, mm, ll);
        bx[q][0][i] = hh;
        bx[q][1][i] = mm;
        bx[q][2][i] = ll;
      }
    lds_barrier();
    // the lifting weights of the next step, requested into registers right before the end-of-step barrier (~2 us of L2 latency
    // stay exposed behind it).  Requesting them BEFORE the projection, to travel under its 16 us, spilled 38 registers per lane
    // and lost 8 % (1.501 vs 1.385 ms per rollout).
    u32x4 pre_w2[6];
    float pre_w1[8], pre_b1 = 0.f;
    auto lift_prefetch = [&]() {
      const int n_w2p = (p.lift_hid >> 5) * 6 * 64, n_w1p = (p.lift_hid >> 4) * p.lift_ns * 64;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const int i = tid + k * NT;
        pre_w2[k] = p.lift_w2b[i < n_w2p ? i : 0];
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int i = tid + k * NT;
        pre_w1[k] = p.lift_w1p[i < n_w1p ? i : 0];
      }
      pre_b1 = p.lift_b1[tid < p.lift_hid ? tid : 0];
    };
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    auto run = [&](auto coc) {
      constexpr int CO = decltype(coc)::value;
      float po[CO][4];
      proj_segment<CO, F16>(bx, q_w1, q_b1, q_w2, ntile_p, lane, po, p.proj_down);
#pragma unroll
      for (int co = 0; co < CO; ++co)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float x = po[co][q];
          x += __shfl_xor(x, 16);
          x += __shfl_xor(x, 32);
          if (g == co) v[q] = x;
        }
    };
    if (p.proj_co == 1) run(std::integral_constant<int, 1>{});
    else if (p.proj_co == 2) run(std::integral_constant<int, 2>{});
    else run(std::integral_constant<int, 4>{});
    if (g < p.cout) {
      const float b2 = p.proj_b2[g];
      v += f32x4{b2, b2, b2, b2};
      if (p.feed_regs && st > 0) {
        v += vfeed;      // the residual is the previous output: still in this lane's registers
      } else {
        const float* resid_p = p.resid;
        long long resid_bs = p.resid_bstride;
        if (p.n_steps > 1) rollout_step_resid(p, p.r_t0 + st, HW, resid_p, resid_bs);
        if (resid_p) v += *reinterpret_cast<const f32x4*>(resid_p + (long long)gs * resid_bs + (long long)g * HW + pix);
      }
      if (*s_fail) v = f32x4{__uint_as_float(0x7fc00000u), __uint_as_float(0x7fc00000u), __uint_as_float(0x7fc00000u),
                             __uint_as_float(0x7fc00000u)};
      float* out_p = p.out;
      long long out_bs = p.out_bstride;
      if (p.n_steps > 1) rollout_step_out(p, p.r_t0 + st, HW, out_p, out_bs);
      *reinterpret_cast<f32x4*>(out_p + (long long)gs * out_bs + (long long)g * HW + pix) = v;
      if constexpr (F16) {
        // f16x3 range guard: an activation beyond the f16 range (|x| >= 65520) turns into inf and then NaN; a non-finite
        // OUTPUT sets bit 1 of the fail word (and the second sticky counter) and the host repeats the range on the
        // bf16x6 kernels, whose operands have the fp32 exponent range.  (Non-finite INPUTS take the same detour.)
        const float mag = fabsf(v[0]) + fabsf(v[1]) + fabsf(v[2]) + fabsf(v[3]);
        if (!(mag < 3.0e38f) && p.fail_word) {
          atomicOr(p.fail_word, 2u);
          atomicAdd(p.sticky_fails + 1, 1u);
        }
      }
    }
    if (p.trace && tid == p.trace_tid && n_stamp < 64) p.trace[blockIdx.x * 64 + n_stamp++] = __builtin_amdgcn_s_memrealtime();
    if (st + 1 < n_steps) {
      const int npair_n = p.lift_hid >> 5, n_w2 = npair_n * 6 * 64, n_w1 = (p.lift_hid >> 4) * p.lift_ns * 64;
      auto feed_next = [&]() {
        if (p.feed_regs) {
          vfeed = (g < p.cout) ? v : f32x4{0.f, 0.f, 0.f, 0.f};   // next input + residual: no store -> load round trip, no drain
        } else {
          // the next step's input rows are the ones this wave has just written: drain the stores, drop any L1 copy
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
      };
      if (p.lift_tab != nullptr) {
        feed_next();   // the next step votes: no weight request here, and the barrier of the seam is the one behind its vote
      } else {
        lift_prefetch();
        feed_next();
        lds_barrier();   // every wave is done with the projection weights: the lifting weights may overwrite them
        u32x4* l_w2n = reinterpret_cast<u32x4*>(smem);
        float* l_w1n = reinterpret_cast<float*>(l_w2n + n_w2);
        float* l_b1n = l_w1n + n_w1;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          const int i = tid + k * NT;
          if (i < n_w2) l_w2n[i] = pre_w2[k];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int i = tid + k * NT;
          if (i < n_w1) l_w1n[i] = pre_w1[k];
        }
        if (tid < p.lift_hid) l_b1n[tid] = pre_b1;
        // vmcnt(0): a request whose lane stores nothing is still pending for the compiler; without this it drains at the top
        // of the next step, on the path of the voting seam too (for the listing; not measurable on its own, kWaitVm0)
        __builtin_amdgcn_s_waitcnt(kWaitVm0);
        staged = true;
      }
    }
    continue;
  }
#pragma unroll
  for (int ot = 0; ot < 2; ++ot)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      *reinterpret_cast<f32x4*>(p.y + ((long long)gs * C + 16 * ot + 4 * g + r) * HW + pix) = vv[ot][r];
  }   // steps
}

// ---------------------------------------------------------------------------------------------
// host side: eligibility, counter reset, launch
// ---------------------------------------------------------------------------------------------
constexpr size_t trunk_lds(int rows) {
  return ((size_t)rows * kC * kTrStride + rows * kSyStride + rows * 16 * kC + rows * 128 + 2 * 16 * 64 + 4 + 2 * 2 * 16 * rows +
          6 * 3 * 64 * 4) *
         sizeof(float);
}
// rows (= waves) per workgroup.  8 = one workgroup per CU (default).  4 puts two workgroups on a CU (2 x 61 KB of
// LDS, 2 x 4 waves x 256 VGPRs) so that one can compute rows while the other sits in a group barrier -- measured
// SLOWER at the headline size (68 vs 51 us per launch: twice the partials to publish and sum, two ky columns per
// wave in P1/P3); kept for grids whose height is not a multiple of 8 and selectable with DLWP_TRUNK_ROWS=4.
static int trunk_rows(const dlwp_fno2d_plan* p) {
  const int forced = p->k.trunk_rows_forced;
  for (int rows : {8, 4}) {
    if (forced && rows != forced) continue;
    if (p->H % rows) continue;
    const int G = p->H / rows;
    if (G != 4 && G != 8 && G != 16 && G != 32) continue;          // instantiated group sizes
    if (rows == 4 && G == 4) continue;
    if (rows == 8 && G == 32) continue;
    if ((p->sc.M1 * p->sc.M2 + G - 1) / G > 4 * rows) continue;    // at most 4 modes per wave in P2
    if (G > p->k.cus * (8 / rows)) continue;                       // a sample's group must be resident at once
    return rows;
  }
  return 0;
}
static bool trunk_eligible(const dlwp_fno2d_plan* p) {
  if (!p->k.trunk || p->k.fp32_mfma) return false;
  if (p->W != 64 || p->sc.KP != 16 || p->sc.M1 > 16 || p->L > kTrunkMaxLayers) return false;
  return trunk_rows(p) != 0;
}
// Whole step in one launch (STEP variant of the trunk kernel): needs the flag-in-data protocol, 8 rows per workgroup,
// bf16x6 MLP weights that fit the transpose-tile LDS (widths <= 256, <= 16 input channels) and the FMA layer 2
// of the projection (<= 4 outputs).  DLWP_FNO_STEP=0 keeps lifting / trunk / projection as three launches.
bool step_eligible(const dlwp_fno2d_plan* p) {
  return p->k.step && trunk_eligible(p) && p->k.ll && trunk_rows(p) == 8 && p->cin_steps <= 4 &&
         p->hid_l % 32 == 0 && p->hid_l <= 256 && p->hid_p <= 256 && p->proj_co > 0 && p->lift_w2b.p != nullptr &&
         p->proj_w1bp.p != nullptr;
}
int fused_resident_per_cu(int G) {
  int n = 0;
  hipError_t oe = hipErrorInvalidValue;
  constexpr size_t lds = trunk_lds(8);
  auto query = [&](auto kern) {
    oe = allow_lds(kern, lds);
    if (oe == hipSuccess) oe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kern, 512, lds);
  };
  if (G == 4) query(fno_trunk_kernel<8, 4, true, true>);
  else if (G == 8) query(fno_trunk_kernel<8, 8, true, true>);
  else if (G == 16) query(fno_trunk_kernel<8, 16, true, true>);
  else { oe = hipSuccess; n = 1; }
  if (oe != hipSuccess) { (void)hipGetLastError(); n = 0; }
  // the fused kernels were tuned and verified at ONE workgroup per CU (the query says 1 at ~120 KB of LDS); never
  // size a grid beyond that even if a later compiler build would admit two
  return n >= 1 ? 1 : 0;
}
// xpart copy 0 | xpart copy 1 | obuf copy 0 | obuf copy 1, each as large as the B samples and the G = H / rows workgroups per sample
// in use need; 11 + 1.4 MB at the headline shape instead of the 22 + 1.4 MB the workspace reserves (fill time per rollout)
struct ExchangeLayout {
  float* xpart;
  float* obuf;
  long long xpart_par, obuf_par;
  size_t floats;
};
static ExchangeLayout exchange_layout(const dlwp_fno2d_plan* p, const FnoWorkspace& ws, int B) {
  const int rows = trunk_rows(p), G = rows ? p->H / rows : (p->H + 3) / 4;
  const size_t nm = (size_t)p->sc.M1 * p->sc.M2 * 64;                    // floats per (sample, member)
  ExchangeLayout x;
  x.xpart = ws.xpart;
  x.xpart_par = (long long)((size_t)B * G * nm);
  x.obuf = ws.xpart + 2 * (size_t)B * G * nm;
  x.obuf_par = (long long)((size_t)B * nm);
  x.floats = 2 * (size_t)B * G * nm + 2 * (size_t)B * nm;               // <= 2 xpart_half + 2 obuf_half (G <= H / 4)
  return x;
}
}  // namespace fno
}  // namespace dlwp
namespace {   // at global scope, where this kernel has always been: its symbol name stays what profiles and traces know
__global__ __launch_bounds__(256) void trunk_arm_kernel(dlwp::u32x4* __restrict__ xch, size_t quads, unsigned* __restrict__ ctr, size_t words) {
  const size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  const dlwp::u32x4 sent = {dlwp::fno::kSentinel, dlwp::fno::kSentinel, dlwp::fno::kSentinel, dlwp::fno::kSentinel};
  for (size_t i = i0; i < quads; i += stride) xch[i] = sent;
  for (size_t i = i0; i < words; i += stride) ctr[i] = 0u;
}
}  // namespace
namespace dlwp {
namespace fno {
int32_t trunk_begin(const dlwp_fno2d_plan* p, const FnoWorkspace& ws, int B, TrunkState& st, hipStream_t s, bool force_unfused) {
  st.on = trunk_eligible(p) && !force_unfused;
  st.epoch = 0;
  st.layers = 0;
  if (st.on) {
    // ONE launch: zero the group counters, the XCC-id table and the fail word behind them; arm both copies of both exchange buffers
    // with the sentinel (laid out back to back for the group size in use: exchange_layout()).  A kernel of our own rather than
    // hipMemset*Async: two fills were two more nodes in front of every rollout (~5 us each).
    const size_t zero_words = (2 * align_up((size_t)B * kCtrStrideBytes, 256) + kFailBytes) / 4;
    const ExchangeLayout x = exchange_layout(p, ws, B);
    const size_t arm_quads = p->k.ll ? x.floats / 4 : 0;             // nm is a multiple of 64 floats
    hipLaunchKernelGGL(trunk_arm_kernel, dim3(512), dim3(256), 0, s, reinterpret_cast<u32x4*>(x.xpart), arm_quads, ws.ctr, zero_words);
    DLWP_HIP_CHECK(hipGetLastError());
  }
  return DLWP_OK;
}
template <int G>
static hipError_t step_launch_one(const TrunkParams& tp, hipStream_t s, bool f16) {
  constexpr size_t lds = trunk_lds(8);
  if (f16) {
    hipError_t e = allow_lds(fno_trunk_kernel<8, G, true, true, true>, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((fno_trunk_kernel<8, G, true, true, true>), dim3(tp.S * G), dim3(512), lds, s, tp);
    return hipGetLastError();
  }
  hipError_t e = allow_lds(fno_trunk_kernel<8, G, true, true>, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((fno_trunk_kernel<8, G, true, true>), dim3(tp.S * G), dim3(512), lds, s, tp);
  return hipGetLastError();
}
template <int ROWS, int G>
static hipError_t trunk_launch_one(const TrunkParams& tp, hipStream_t s, bool ll) {
  constexpr size_t lds = trunk_lds(ROWS);
  if (ll) {
    hipError_t e = allow_lds(fno_trunk_kernel<ROWS, G, true>, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((fno_trunk_kernel<ROWS, G, true>), dim3(tp.S * G), dim3(64 * ROWS), lds, s, tp);
  } else {
    hipError_t e = allow_lds(fno_trunk_kernel<ROWS, G, false>, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((fno_trunk_kernel<ROWS, G, false>), dim3(tp.S * G), dim3(64 * ROWS), lds, s, tp);
  }
  return hipGetLastError();
}
int32_t launch_trunk(const dlwp_fno2d_plan* p, const FnoWorkspace& ws, int B, const float* hin, float* hout,
                     TrunkState& st, hipStream_t s, const StepIO* io) {
  const int rows = trunk_rows(p);
  DLWP_REQUIRE(rows > 0, DLWP_ERR_UNSUPPORTED, "fused trunk not available for this plan");
  const int G = p->H / rows;
  // residency: every workgroup of a launch must be on the chip at once (the hand-offs spin on peers).  The grid is
  // bounded by what the occupancy query admitted for the fused kernel at plan creation x the CU count.
  int per_launch = p->k.cus * (rows == 8 ? p->k.resident_per_cu : 8 / rows) / G;
  if (per_launch >= 8) per_launch &= ~7;   // keeps the same-XCD group mapping
  DLWP_REQUIRE(per_launch > 0, DLWP_ERR_UNSUPPORTED, "a sample needs %d workgroups, more than fit the device", G);
  const size_t nm = (size_t)p->sc.M1 * p->sc.M2 * 64;
  for (int s0 = 0; s0 < B; s0 += per_launch) {
    TrunkParams tp = {};
    tp.x = hin; tp.y = hout; tp.ybuf = ws.ybuf;
    tp.t = p->sc.t.as<float>(); tp.tt = p->sc.tt.as<float>();
    tp.tb = p->sc.tb.as<u32x4>(); tp.ttb = p->sc.ttb.as<u32x4>();
    tp.ef = p->sc.ef.as<float2>(); tp.ei = p->sc.ei.as<float2>(); tp.ck = p->sc.ck.as<float>();
    for (int l = 0; l < kTrunkMaxLayers; ++l) {
      const int ll = l < p->L ? l : 0;
      tp.wsb[l] = p->wsbp[ll].as<u32x4>(); tp.bias[l] = p->sbias[ll].as<float>(); tp.wt[l] = p->wt[ll].as<float2>();
    }
    tp.S = (B - s0 < per_launch) ? B - s0 : per_launch;
    const ExchangeLayout xl = exchange_layout(p, ws, B);
    tp.xpart = xl.xpart + (size_t)s0 * G * nm;
    tp.obuf = xl.obuf + (size_t)s0 * nm;
    tp.ctr = ws.ctr + (size_t)s0 * (kCtrStrideBytes / 4);
    tp.epoch = st.epoch; tp.fwd_scale = p->sc.fwd_scale;
    tp.xpart_par = xl.xpart_par; tp.obuf_par = xl.obuf_par; tp.layer0 = st.layers;
    tp.xcc_tab = ws.ctr + align_up((size_t)B * kCtrStrideBytes, 256) / 4 + (size_t)s0 * 32;
    tp.H = p->H; tp.L = p->L; tp.M1 = p->sc.M1; tp.M2 = p->sc.M2; tp.G = G; tp.sample0 = s0;
    tp.spin_limit = p->k.spin_limit; tp.try_limit = p->k.try_limit; tp.fail_word = ws.fail;
    tp.sticky_fails = p->sticky.as<unsigned>();
    // diagnostics: DLWP_TRUNK_TRACE=<file> dumps per-workgroup phase timestamps of the first few launches
    static const char* trace_path = getenv("DLWP_TRUNK_TRACE");
    static unsigned long long* trace_buf = nullptr;
    static int traced = 0;
    tp.trace = nullptr;
    static const char* trace_wave = getenv("DLWP_TRUNK_TRACE_WAVE");
    tp.trace_tid = trace_wave ? 64 * atoi(trace_wave) : 0;
    if (trace_path && traced < 4) {
      if (!trace_buf) DLWP_HIP_CHECK(hipMalloc(&trace_buf, (size_t)1024 * 64 * 8));
      DLWP_HIP_CHECK(hipMemsetAsync(trace_buf, 0, (size_t)1024 * 64 * 8, s));
      if (tp.S * G <= 1024) tp.trace = trace_buf;
    }
    hipError_t le = hipErrorInvalidValue;
    if (io) {
      tp.in = *io->in;
      tp.lift_ns = p->cin_steps; tp.lift_hid = p->hid_l; tp.lift_cin1 = p->cin == 1 ? 1 : 0;
      tp.lift_w1p = p->lift_w1p.as<float>(); tp.lift_b1 = p->lift_b1.as<float>();
      tp.lift_w2b = p->lift_w2b.as<u32x4>(); tp.lift_b2 = p->lift_b2.as<float>();
      tp.lift_tab = p->lift_tab_state == 1 ? p->lift_tab.as<float>() : nullptr;
      tp.proj_hid = p->hid_p; tp.proj_co = p->proj_co; tp.cout = p->cout;
      if (io->lift_only) { tp.proj_hid = 0; tp.y = hout; }   // diagnostics: the projection stays a launch of its own
      tp.proj_w1b = p->proj_w1bp.as<u32x4>(); tp.proj_b1 = p->proj_b1.as<float>();
      tp.proj_w2v = p->proj_w2v.as<float>(); tp.proj_b2 = p->proj_b2.as<float>();
      tp.out = io->out; tp.out_bstride = io->out_bstride; tp.resid = io->resid; tp.resid_bstride = io->resid_bstride;
      tp.n_steps = io->n_steps;
      if (io->n_steps > 1) {
        tp.r_const = io->constants; tp.r_presc = io->prescribed; tp.r_prog = io->prognostic; tp.r_out = io->rollout_out;
        tp.r_nconst = io->n_const; tp.r_npresc = io->n_presc; tp.r_nprog = io->n_prog; tp.r_T = io->T; tp.r_ctx = io->ctx;
        tp.r_t0 = io->t0;
        tp.feed_regs = (io->n_const == 0 && io->n_presc == 0 && io->ctx == 1 && io->n_prog <= 4 && p->cin_steps == 1 &&
                        p->cin == io->n_prog && p->k.feed_regs) ? 1 : 0;
      }
      const bool f16 = p->k.f16x3 && p->lift_w2h.p && p->proj_w1hp.p && !io->lift_only;
      tp.lift_up = tp.lift_down = tp.proj_up = tp.proj_down = 1.f;
      if (f16) {   // f16x3 operands (the unfused kernels and the plain trunk keep bf16x6)
        tp.lift_up = std::ldexp(1.f, 11 + p->lift_shift); tp.lift_down = std::ldexp(1.f, -(11 + p->lift_shift));
        tp.proj_up = std::ldexp(1.f, 11 + p->proj_shift); tp.proj_down = std::ldexp(1.f, -(11 + p->proj_shift));
        tp.lift_w2b = p->lift_w2h.as<u32x4>();
        tp.proj_w1b = p->proj_w1hp.as<u32x4>();
        tp.tb = p->sc.tbh.as<u32x4>(); tp.ttb = p->sc.ttbh.as<u32x4>();
        for (int l = 0; l < kTrunkMaxLayers; ++l) tp.wsb[l] = p->wshp[l < p->L ? l : 0].as<u32x4>();
      }
      if (G == 4) le = step_launch_one<4>(tp, s, f16);
      else if (G == 8) le = step_launch_one<8>(tp, s, f16);
      else if (G == 16) le = step_launch_one<16>(tp, s, f16);
    } else
    if (rows == 8 && G == 4) le = trunk_launch_one<8, 4>(tp, s, p->k.ll);
    else if (rows == 8 && G == 8) le = trunk_launch_one<8, 8>(tp, s, p->k.ll);
    else if (rows == 8 && G == 16) le = trunk_launch_one<8, 16>(tp, s, p->k.ll);
    else if (rows == 4 && G == 8) le = trunk_launch_one<4, 8>(tp, s, p->k.ll);
    else if (rows == 4 && G == 16) le = trunk_launch_one<4, 16>(tp, s, p->k.ll);
    else if (rows == 4 && G == 32) le = trunk_launch_one<4, 32>(tp, s, p->k.ll);
    DLWP_HIP_CHECK(le);
    if (tp.trace) {
      std::vector<unsigned long long> hbuf((size_t)tp.S * G * 64);
      DLWP_HIP_CHECK(hipStreamSynchronize(s));
      DLWP_HIP_CHECK(hipMemcpy(hbuf.data(), trace_buf, hbuf.size() * 8, hipMemcpyDeviceToHost));
      if (FILE* f = fopen(trace_path, traced ? "a" : "w")) {
        for (int wg = 0; wg < tp.S * G; ++wg) {
          fprintf(f, "%d %d", traced, wg);
          for (int k = 0; k < 64 && hbuf[(size_t)wg * 64 + k]; ++k) fprintf(f, " %llu", hbuf[(size_t)wg * 64 + k]);
          fprintf(f, "\n");
        }
        fclose(f);
      }
      ++traced;
    }
  }
  const unsigned steps = (io && io->n_steps > 1) ? (unsigned)io->n_steps : 1u;
  st.epoch += 2u * (unsigned)p->L * steps;
  st.layers += (unsigned)p->L * steps;
  return DLWP_OK;
}

}  // namespace fno
}  // namespace dlwp
