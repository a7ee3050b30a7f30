// Shared host/device helpers for libdlwp_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/dlwp_hip.h"

namespace dlwp {

// ---------------------------------------------------------------------------------------------
// error reporting: thread-local message, int status across the ABI
// ---------------------------------------------------------------------------------------------
std::string& last_error_slot();
int32_t fail(int32_t code, const char* fmt, ...);

#define DLWP_HIP_CHECK(expr)                                                                    \
  do {                                                                                          \
    hipError_t _e = (expr);                                                                     \
    if (_e != hipSuccess)                                                                       \
      return ::dlwp::fail(DLWP_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),  \
                          __FILE__, __LINE__);                                                  \
  } while (0)

#define DLWP_REQUIRE(cond, code, ...)                                                           \
  do {                                                                                          \
    if (!(cond)) return ::dlwp::fail(code, __VA_ARGS__);                                        \
  } while (0)

// RAII for device allocations owned by plans
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) {
    o.p = nullptr;
    o.bytes = 0;
  }
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t n) {
    if (p) {
      (void)hipFree(p);
      p = nullptr;
    }
    bytes = n;
    return hipMalloc(&p, n ? n : 4);
  }
  hipError_t upload(const void* host, size_t n, hipStream_t s) {
    if (p) {
      (void)hipFree(p);
      p = nullptr;
    }
    bytes = n;
    hipError_t e = hipMalloc(&p, n ? n : 4);
    if (e != hipSuccess) return e;
    if (n) e = hipMemcpyAsync(p, host, n, hipMemcpyHostToDevice, s);
    return e;
  }
  template <class T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
};

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---------------------------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));

// v_mfma_f32_16x16x4_f32: D[16x16] += A[16x4] * B[4x16], exact fp32 FMA chain.
//   lane l supplies A[i = l&15][k = l>>4] and B[k = l>>4][j = l&15];
//   D register r of lane l is D[row = 4*(l>>4) + r][col = l&15].
__device__ __forceinline__ f32x4 mfma16x16x4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// sum over the 64 lanes of a wave (xor tree); every lane returns the total
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// GELU (exact, erf form: torch.nn.functional.gelu default) without a libm call.
//   gelu(x) = 0.5 x (1 + erf(x/sqrt2)) = max(x, 0) - |x| * (0.5 erfc(|x|/sqrt2))
//   0.5 erfc(u/sqrt2), u >= 0, is evaluated as exp2(u * Q(u) - 1) with a degree-5 polynomial Q fitted to
//   (log2(0.5 erfc(u/sqrt2)) + 1) / u on u in [0, 4.5 sqrt2] (iteratively re-weighted towards the minimax of the GELU error;
//   u clamped at 4.5 sqrt2, where erfc = 2e-10).  Approximation error of the GELU value 8.7e-8; evaluated in fp32 the error
//   is 5.3e-7 -- set by the rounding of the exponent u Q(u), up to 30, NOT by the degree: the degree-8 polynomial this
//   replaced in round 2 reached 4.8e-7 with three more multiply-adds per element (tests/test_gelu_poly.py).  GELU issue
//   slots are the largest single vector cost of the FNO step (640 evaluations per grid point and step).
// The fp32 matrix instructions run on the same fp32 lanes as the VALU (they do not overlap,
// tools/ubench_fp32.hip), so GELU issue slots are as expensive as MFMA cycles: the 8-wide form below
// uses packed fp32 and costs ~7 issue slots per element (libm-free scalar code: ~19).
#define DLWP_GELU_UMAX 6.3639610306789276f
#define DLWP_GELU_QTOP 2.992443883e-05f
#define DLWP_GELU_COEFFS(X)                                                                    \
  X(-7.398762886e-04f) X(7.977468945e-03f) X(-5.323819506e-02f) X(-4.589156813e-01f) X(-1.151147084e+00f)

__device__ __forceinline__ float gelu_erf(float x) {
  const float u = fminf(fabsf(x), DLWP_GELU_UMAX);
  float p = DLWP_GELU_QTOP;
#define DLWP_STEP(c) p = fmaf(p, u, c);
  DLWP_GELU_COEFFS(DLWP_STEP)
#undef DLWP_STEP
  const float e = __builtin_amdgcn_exp2f(fmaf(p, u, -1.0f));  // 0.5 erfc(|x|/sqrt2)
  return fmaf(-fabsf(x), e, fmaxf(x, 0.f));
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// GELU of two accumulator fragments (8 values): four packed chains interleaved statement by
// statement.  gfx950 needs two wait states between a packed-fp32 op and a dependent VALU op; with
// fewer than three independent instructions in between hipcc pads with s_nop, each of which costs
// a full issue slot on the (shared) fp32 pipe.  volatile keeps the hand interleave.
__device__ __forceinline__ void gelu_erf8_stmt(f32x4& u, f32x4& v) {
  const float x0 = u[0], x1 = u[1], x2 = u[2], x3 = u[3], x4 = v[0], x5 = v[1], x6 = v[2], x7 = v[3];
  float t0, t1, t2, t3, t4, t5, t6, t7;
  // The clamp constant sits in an SGPR the compiler cannot see through: with a literal it emits v_max |x|,|x| + v_min
  // (a VOP3 instruction, which the |x| modifier needs, takes no literal on gfx9) -- one wasted issue slot per element.
  float umax = DLWP_GELU_UMAX;
  asm volatile("" : "+s"(umax));
  // The FIRST reads of the inputs are plain C, not asm: the inputs are often MFMA results, and a VALU read of a
  // register an MFMA has just written needs several wait states that hipcc only inserts for instructions it can see --
  // its hazard recognizer skips inline asm (a fused kernel whose schedule put `v_mfma ... v[64:67]` directly in front
  // of an asm `v_min_f32 v100, |v64|` computed garbage for exactly those elements).
  // (v_med3_f32 |x|, 0, umax = min(|x|, umax) in ONE instruction: fminf(fabsf(x), c) costs two, because IEEE mode makes
  // hipcc canonicalize the operand of a minimum with v_max |x|, |x| first)
#define DLWP_CLAMP(x) __builtin_amdgcn_fmed3f(__builtin_fabsf(x), 0.f, umax)
  t0 = DLWP_CLAMP(x0); t2 = DLWP_CLAMP(x2); t4 = DLWP_CLAMP(x4); t6 = DLWP_CLAMP(x6);
  t1 = DLWP_CLAMP(x1); t3 = DLWP_CLAMP(x3); t5 = DLWP_CLAMP(x5); t7 = DLWP_CLAMP(x7);
#undef DLWP_CLAMP
  const f32x2 ta = {t0, t1}, tb = {t2, t3}, tc = {t4, t5}, td = {t6, t7};
  f32x2 pa = {DLWP_GELU_QTOP, DLWP_GELU_QTOP}, pb = pa, pc = pa, pd = pa;
  float m0, m1, m2, m3, m4, m5, m6, m7;
#define DLWP_X(m, x) asm volatile("v_max_f32_e32 %0, 0, %1" : "=v"(m) : "v"(x));
  // A dependent v_pk_fma_f32 needs FOUR other instructions behind its producer (hipcc pads a group of four chains with
  // an s_nop, a full issue slot): the max(x, 0) of the final combination fill those slots instead.
#define DLWP_PKSTEP4(cf, FILL)                                                                 \
  {                                                                                            \
    const f32x2 cc = {cf, cf};                                                                 \
    asm volatile("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(pa) : "v"(pa), "v"(ta), "s"(cc));        \
    asm volatile("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(pb) : "v"(pb), "v"(tb), "s"(cc));        \
    asm volatile("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(pc) : "v"(pc), "v"(tc), "s"(cc));        \
    asm volatile("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(pd) : "v"(pd), "v"(td), "s"(cc));        \
    FILL                                                                                       \
  }
#define DLWP_C5(c0, c1, c2, c3, c4)                                                            \
  DLWP_PKSTEP4(c0, DLWP_X(m0, x0)) DLWP_PKSTEP4(c1, DLWP_X(m1, x1)) DLWP_PKSTEP4(c2, DLWP_X(m2, x2))     \
  DLWP_PKSTEP4(c3, DLWP_X(m3, x3)) DLWP_PKSTEP4(c4, DLWP_X(m4, x4))
#define DLWP_CX(c) c,
#define DLWP_C5_APPLY(...) DLWP_C5_EXPAND(__VA_ARGS__)
#define DLWP_C5_EXPAND(c0, c1, c2, c3, c4, ...) DLWP_C5(c0, c1, c2, c3, c4)
  DLWP_C5_APPLY(DLWP_GELU_COEFFS(DLWP_CX) 0)
#undef DLWP_C5_APPLY
#undef DLWP_C5_EXPAND
#undef DLWP_CX
#undef DLWP_C5
  DLWP_PKSTEP4(-1.0f, DLWP_X(m5, x5) DLWP_X(m6, x6) DLWP_X(m7, x7))   // exponent u Q(u) - 1
#undef DLWP_PKSTEP4
#undef DLWP_X
  float e0, e1, e2, e3, e4, e5, e6, e7;
  const float a0 = pa.x, a1 = pa.y, a2 = pb.x, a3 = pb.y, a4 = pc.x, a5 = pc.y, a6 = pd.x, a7 = pd.y;
#define DLWP_E(e, a) asm volatile("v_exp_f32_e32 %0, %1" : "=v"(e) : "v"(a));
  DLWP_E(e0, a0) DLWP_E(e1, a1) DLWP_E(e2, a2) DLWP_E(e3, a3) DLWP_E(e4, a4) DLWP_E(e5, a5) DLWP_E(e6, a6) DLWP_E(e7, a7)
#undef DLWP_E
  float r0, r1, r2, r3, r4, r5, r6, r7;
#define DLWP_F(r, x, h, m) asm volatile("v_fma_f32 %0, -|%1|, %2, %3" : "=v"(r) : "v"(x), "v"(h), "v"(m));
  DLWP_F(r0, x0, e0, m0) DLWP_F(r1, x1, e1, m1) DLWP_F(r2, x2, e2, m2) DLWP_F(r3, x3, e3, m3)
  DLWP_F(r4, x4, e4, m4) DLWP_F(r5, x5, e5, m5) DLWP_F(r6, x6, e6, m6) DLWP_F(r7, x7, e7, m7)
#undef DLWP_F
  u = f32x4{r0, r1, r2, r3};
  v = f32x4{r4, r5, r6, r7};
}

// gelu_erf8 (the form every kernel uses; gelu_erf8_stmt above is the statement-per-instruction form it replaced, kept for A/B:
// 1.515 -> 1.467 ms per FNO rollout): the whole polynomial in ONE asm block, exponentials / final combination in two more.  hipcc
// pads every inline-asm statement it cannot see into (an s_nop per group of four packed FMAs, ~8 issue slots per call)
// and reloads the seven coefficient pairs of the statement-per-instruction form from spilled SGPRs (v_readlane) when the
// surrounding kernel is short of them.  Here the seven constants ride in three SGPR pairs (op_sel picks the half; the
// final -1 is an inline constant), a dependent packed FMA has four other instructions behind its producer by construction
// (three sibling chains + one max(x, 0)), and v_exp -> v_fma pairs are eight instructions apart.
__device__ __forceinline__ void gelu_erf8(f32x4& u, f32x4& v) {
  const float x0 = u[0], x1 = u[1], x2 = u[2], x3 = u[3], x4 = v[0], x5 = v[1], x6 = v[2], x7 = v[3];
  float umax = DLWP_GELU_UMAX;
  asm volatile("" : "+s"(umax));
  // first reads of the inputs in plain C (MFMA -> VALU wait states are hipcc's to insert, see gelu_erf8)
#define DLWP_CLAMP(x) __builtin_amdgcn_fmed3f(__builtin_fabsf(x), 0.f, umax)
  const f32x2 ta = {DLWP_CLAMP(x0), DLWP_CLAMP(x1)}, tb = {DLWP_CLAMP(x2), DLWP_CLAMP(x3)};
  const f32x2 tc = {DLWP_CLAMP(x4), DLWP_CLAMP(x5)}, td = {DLWP_CLAMP(x6), DLWP_CLAMP(x7)};
#undef DLWP_CLAMP
#define DLWP_CX(c) c,
  constexpr float kc[6] = {DLWP_GELU_COEFFS(DLWP_CX) 0.f};
#undef DLWP_CX
  const f32x2 c01 = {DLWP_GELU_QTOP, kc[0]}, c23 = {kc[1], kc[2]}, c45 = {kc[3], kc[4]};
  f32x2 pa, pb, pc, pd;
  float m0, m1, m2, m3, m4, m5, m6, m7;
  asm volatile(
      "v_pk_fma_f32 %0, %20, %12, %20 op_sel:[0,0,1] op_sel_hi:[0,1,1]\n\t"
      "v_pk_fma_f32 %1, %20, %13, %20 op_sel:[0,0,1] op_sel_hi:[0,1,1]\n\t"
      "v_pk_fma_f32 %2, %20, %14, %20 op_sel:[0,0,1] op_sel_hi:[0,1,1]\n\t"
      "v_pk_fma_f32 %3, %20, %15, %20 op_sel:[0,0,1] op_sel_hi:[0,1,1]\n\t"
      "v_max_f32_e32 %4, 0, %16\n\t"
      "v_pk_fma_f32 %0, %0, %12, %21 op_sel_hi:[1,1,0]\n\t"
      "v_pk_fma_f32 %1, %1, %13, %21 op_sel_hi:[1,1,0]\n\t"
      "v_pk_fma_f32 %2, %2, %14, %21 op_sel_hi:[1,1,0]\n\t"
      "v_pk_fma_f32 %3, %3, %15, %21 op_sel_hi:[1,1,0]\n\t"
      "v_max_f32_e32 %5, 0, %17\n\t"
      "v_pk_fma_f32 %0, %0, %12, %21 op_sel:[0,0,1] op_sel_hi:[1,1,1]\n\t"
      "v_pk_fma_f32 %1, %1, %13, %21 op_sel:[0,0,1] op_sel_hi:[1,1,1]\n\t"
      "v_pk_fma_f32 %2, %2, %14, %21 op_sel:[0,0,1] op_sel_hi:[1,1,1]\n\t"
      "v_pk_fma_f32 %3, %3, %15, %21 op_sel:[0,0,1] op_sel_hi:[1,1,1]\n\t"
      "v_max_f32_e32 %6, 0, %18\n\t"
      "v_pk_fma_f32 %0, %0, %12, %22 op_sel_hi:[1,1,0]\n\t"
      "v_pk_fma_f32 %1, %1, %13, %22 op_sel_hi:[1,1,0]\n\t"
      "v_pk_fma_f32 %2, %2, %14, %22 op_sel_hi:[1,1,0]\n\t"
      "v_pk_fma_f32 %3, %3, %15, %22 op_sel_hi:[1,1,0]\n\t"
      "v_max_f32_e32 %7, 0, %19\n\t"
      "v_pk_fma_f32 %0, %0, %12, %22 op_sel:[0,0,1] op_sel_hi:[1,1,1]\n\t"
      "v_pk_fma_f32 %1, %1, %13, %22 op_sel:[0,0,1] op_sel_hi:[1,1,1]\n\t"
      "v_pk_fma_f32 %2, %2, %14, %22 op_sel:[0,0,1] op_sel_hi:[1,1,1]\n\t"
      "v_pk_fma_f32 %3, %3, %15, %22 op_sel:[0,0,1] op_sel_hi:[1,1,1]\n\t"
      "v_max_f32_e32 %8, 0, %23\n\t"
      "v_pk_fma_f32 %0, %0, %12, -1.0 op_sel_hi:[1,1,0]\n\t"
      "v_pk_fma_f32 %1, %1, %13, -1.0 op_sel_hi:[1,1,0]\n\t"
      "v_pk_fma_f32 %2, %2, %14, -1.0 op_sel_hi:[1,1,0]\n\t"
      "v_pk_fma_f32 %3, %3, %15, -1.0 op_sel_hi:[1,1,0]\n\t"
      "v_max_f32_e32 %9, 0, %24\n\t"
      "v_max_f32_e32 %10, 0, %25\n\t"
      "v_max_f32_e32 %11, 0, %26"
      : "=&v"(pa), "=&v"(pb), "=&v"(pc), "=&v"(pd), "=&v"(m0), "=&v"(m1), "=&v"(m2), "=&v"(m3), "=&v"(m4), "=&v"(m5),
        "=&v"(m6), "=&v"(m7)
      : "v"(ta), "v"(tb), "v"(tc), "v"(td), "v"(x0), "v"(x1), "v"(x2), "v"(x3), "s"(c01), "s"(c23), "s"(c45), "v"(x4),
        "v"(x5), "v"(x6), "v"(x7));
  // exponentials into fresh registers (tied in / out operands on halves of a 64-bit pair cost a v_mov each), four elements
  // per block (30-operand limit of an asm statement)
  float e0, e1, e2, e3, e4, e5, e6, e7;
#define DLWP_TAIL4(ea, eb, ec, ed, aa, ab, ac, ad, ma, mb, mc, md, xa, xb, xc, xd)                                     \
  asm volatile("v_exp_f32_e32 %0, %8\n\tv_exp_f32_e32 %1, %9\n\tv_exp_f32_e32 %2, %10\n\tv_exp_f32_e32 %3, %11\n\t"    \
               "v_fma_f32 %4, -|%12|, %0, %4\n\tv_fma_f32 %5, -|%13|, %1, %5\n\t"                                   \
               "v_fma_f32 %6, -|%14|, %2, %6\n\tv_fma_f32 %7, -|%15|, %3, %7"                                        \
               : "=&v"(ea), "=&v"(eb), "=&v"(ec), "=&v"(ed), "+v"(ma), "+v"(mb), "+v"(mc), "+v"(md)                   \
               : "v"(aa), "v"(ab), "v"(ac), "v"(ad), "v"(xa), "v"(xb), "v"(xc), "v"(xd))
  DLWP_TAIL4(e0, e1, e2, e3, pa.x, pa.y, pb.x, pb.y, m0, m1, m2, m3, x0, x1, x2, x3);
  DLWP_TAIL4(e4, e5, e6, e7, pc.x, pc.y, pd.x, pd.y, m4, m5, m6, m7, x4, x5, x6, x7);
#undef DLWP_TAIL4
  u = f32x4{m0, m1, m2, m3};
  v = f32x4{m4, m5, m6, m7};
}

// The same GELU on eight plain v_fma_f32 chains.  For kernels whose SIMD also issues bf16 MFMAs (its own or the
// partner wave's): an MFMA and a VALU instruction share the SIMD's issue port, and beside MFMAs a packed-fp32
// instruction costs much more than the two plain ones it replaces (MI355X_MICROARCH.md, constants table: one
// v_pk_fma_f32 = +22 cycles over two v_fma_f32) -- the token MLP went 516 -> see token_mlp.hip with this form.
__device__ __forceinline__ void gelu_erf8_fma_stmt(f32x4& u, f32x4& v) {
  const float x0 = u[0], x1 = u[1], x2 = u[2], x3 = u[3], x4 = v[0], x5 = v[1], x6 = v[2], x7 = v[3];
  const float umax = DLWP_GELU_UMAX;
  // first reads in plain C (MFMA -> VALU hazard, see gelu_erf8)
  const float t0 = fminf(fabsf(x0), umax), t1 = fminf(fabsf(x1), umax), t2 = fminf(fabsf(x2), umax),
              t3 = fminf(fabsf(x3), umax), t4 = fminf(fabsf(x4), umax), t5 = fminf(fabsf(x5), umax),
              t6 = fminf(fabsf(x6), umax), t7 = fminf(fabsf(x7), umax);
  float p0 = DLWP_GELU_QTOP, p1 = p0, p2 = p0, p3 = p0, p4 = p0, p5 = p0, p6 = p0, p7 = p0;
#define DLWP_FSTEP1(p, t, cf) asm volatile("v_fma_f32 %0, %1, %2, %3" : "=v"(p) : "v"(p), "v"(t), "s"(cf));
#define DLWP_FSTEP8(cf)                                                                        \
  {                                                                                            \
    const float cc = cf;                                                                       \
    DLWP_FSTEP1(p0, t0, cc) DLWP_FSTEP1(p1, t1, cc) DLWP_FSTEP1(p2, t2, cc) DLWP_FSTEP1(p3, t3, cc) \
    DLWP_FSTEP1(p4, t4, cc) DLWP_FSTEP1(p5, t5, cc) DLWP_FSTEP1(p6, t6, cc) DLWP_FSTEP1(p7, t7, cc) \
  }
  DLWP_GELU_COEFFS(DLWP_FSTEP8)
  DLWP_FSTEP8(-1.0f)   // exponent u Q(u) - 1
#undef DLWP_FSTEP8
#undef DLWP_FSTEP1
  float m0, m1, m2, m3, m4, m5, m6, m7, e0, e1, e2, e3, e4, e5, e6, e7;
#define DLWP_X(m, x) asm volatile("v_max_f32_e32 %0, 0, %1" : "=v"(m) : "v"(x));
#define DLWP_E(e, a) asm volatile("v_exp_f32_e32 %0, %1" : "=v"(e) : "v"(a));
  DLWP_E(e0, p0) DLWP_X(m0, x0) DLWP_E(e1, p1) DLWP_X(m1, x1) DLWP_E(e2, p2) DLWP_X(m2, x2) DLWP_E(e3, p3) DLWP_X(m3, x3)
  DLWP_E(e4, p4) DLWP_X(m4, x4) DLWP_E(e5, p5) DLWP_X(m5, x5) DLWP_E(e6, p6) DLWP_X(m6, x6) DLWP_E(e7, p7) DLWP_X(m7, x7)
#undef DLWP_E
#undef DLWP_X
  float r0, r1, r2, r3, r4, r5, r6, r7;
#define DLWP_F(r, x, h, m) asm volatile("v_fma_f32 %0, -|%1|, %2, %3" : "=v"(r) : "v"(x), "v"(h), "v"(m));
  DLWP_F(r0, x0, e0, m0) DLWP_F(r1, x1, e1, m1) DLWP_F(r2, x2, e2, m2) DLWP_F(r3, x3, e3, m3)
  DLWP_F(r4, x4, e4, m4) DLWP_F(r5, x5, e5, m5) DLWP_F(r6, x6, e6, m6) DLWP_F(r7, x7, e7, m7)
#undef DLWP_F
  u = f32x4{r0, r1, r2, r3};
  v = f32x4{r4, r5, r6, r7};
}

// gelu_erf8_fma (the form the token MLP and the Linear epilogue use; gelu_erf8_fma_stmt above is the statement-per-instruction
// form it replaced): plain v_fma_f32 chains like before, but four elements per asm block -- one v_med3 instead of
// v_max |x|,|x| + v_min per element, no compiler-inserted s_nop between the statements (17 per 16 elements in the token MLP).
__device__ __forceinline__ void gelu_erf8_fma(f32x4& u, f32x4& v) {
  float umax = DLWP_GELU_UMAX;
  asm volatile("" : "+s"(umax));
#define DLWP_CX(c) c,
  constexpr float kc[6] = {DLWP_GELU_COEFFS(DLWP_CX) 0.f};
#undef DLWP_CX
  const float c0 = kc[0], c1 = kc[1], c2 = kc[2], c3 = kc[3], c4 = kc[4], qtop = DLWP_GELU_QTOP;
  auto half = [&](f32x4& w) {
    const float x0 = w[0], x1 = w[1], x2 = w[2], x3 = w[3];
    // first reads in plain C (MFMA -> VALU hazard, see gelu_erf8)
    const float t0 = __builtin_amdgcn_fmed3f(__builtin_fabsf(x0), 0.f, umax), t1 = __builtin_amdgcn_fmed3f(__builtin_fabsf(x1), 0.f, umax),
                t2 = __builtin_amdgcn_fmed3f(__builtin_fabsf(x2), 0.f, umax), t3 = __builtin_amdgcn_fmed3f(__builtin_fabsf(x3), 0.f, umax);
    float p0, p1, p2, p3, m0, m1, m2, m3, q;
#define DLWP_STEP4(c) "v_fma_f32 %0, %0, %9, " c "\n\tv_fma_f32 %1, %1, %10, " c "\n\tv_fma_f32 %2, %2, %11, " c "\n\tv_fma_f32 %3, %3, %12, " c "\n\t"
    asm volatile(
        "v_mov_b32 %8, %17\n\t"
        "v_fma_f32 %0, %8, %9, %18\n\tv_fma_f32 %1, %8, %10, %18\n\tv_fma_f32 %2, %8, %11, %18\n\tv_fma_f32 %3, %8, %12, %18\n\t"
        DLWP_STEP4("%19") "v_max_f32_e32 %4, 0, %13\n\t"
        DLWP_STEP4("%20") "v_max_f32_e32 %5, 0, %14\n\t"
        DLWP_STEP4("%21") "v_max_f32_e32 %6, 0, %15\n\t"
        DLWP_STEP4("%22") "v_max_f32_e32 %7, 0, %16\n\t"
        "v_fma_f32 %0, %0, %9, -1.0\n\tv_fma_f32 %1, %1, %10, -1.0\n\tv_fma_f32 %2, %2, %11, -1.0\n\tv_fma_f32 %3, %3, %12, -1.0"
        : "=&v"(p0), "=&v"(p1), "=&v"(p2), "=&v"(p3), "=&v"(m0), "=&v"(m1), "=&v"(m2), "=&v"(m3), "=&v"(q)
        : "v"(t0), "v"(t1), "v"(t2), "v"(t3), "v"(x0), "v"(x1), "v"(x2), "v"(x3), "s"(qtop), "s"(c0), "s"(c1), "s"(c2), "s"(c3),
          "s"(c4));
#undef DLWP_STEP4
    float e0, e1, e2, e3;
    asm volatile("v_exp_f32_e32 %0, %8\n\tv_exp_f32_e32 %1, %9\n\tv_exp_f32_e32 %2, %10\n\tv_exp_f32_e32 %3, %11\n\t"
                 "v_fma_f32 %4, -|%12|, %0, %4\n\tv_fma_f32 %5, -|%13|, %1, %5\n\t"
                 "v_fma_f32 %6, -|%14|, %2, %6\n\tv_fma_f32 %7, -|%15|, %3, %7"
                 : "=&v"(e0), "=&v"(e1), "=&v"(e2), "=&v"(e3), "+v"(m0), "+v"(m1), "+v"(m2), "+v"(m3)
                 : "v"(p0), "v"(p1), "v"(p2), "v"(p3), "v"(x0), "v"(x1), "v"(x2), "v"(x3));
    w = f32x4{m0, m1, m2, m3};
  };
  half(u);
  half(v);
}

// ---------------------------------------------------------------------------------------------
// fp32 GEMM on the bf16 matrix pipe ("bf16x6")
//   x = h + m + l with h = bf16(x), m = bf16(x - h), l = bf16(x - h - m)  (exact to 2^-24 |x|)
//   a*b ~= al*bh + ah*bl + am*bm + am*bh + ah*bm + ah*bh   (dropped terms <= 2^-24 |a b|)
// accumulated in fp32 by v_mfma_f32_16x16x32_bf16.  Measured (tools) as accurate as a plain fp32 GEMM
// (rel. error 1.1e-7 vs 2.9e-7 at K = 256).  Why: on gfx950 the fp32 MFMA runs on the fp32 VALU lanes
// and cannot overlap VALU work (tools/ubench_fp32.hip), while the bf16 matrix pipe is separate and 16x
// faster per flop -- six bf16 MFMAs cost 6/16 of one fp32 MFMA's time AND leave the fp32 lanes to GELU.
// ---------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// v_mfma_f32_16x16x32_bf16: lane l supplies A[i = l&15][k = 8*(l>>4) + 0..7] and
// B[k = 8*(l>>4) + 0..7][j = l&15] (8 bf16 = 4 dwords, element 0 in the low half of dword 0);
// D register r of lane l is D[row = 4*(l>>4) + r][col = l&15].
__device__ __forceinline__ f32x4 mfma16x16x32_bf16(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

__device__ __forceinline__ unsigned cvt_pk_bf16(float a, float b) {  // RNE, a in the low half
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, bf16x2v));
}

// three-way bf16 split of a pair of floats: 9 VALU issue slots (3 cvt_pk, 4 unpack, 2 packed subtract)
__device__ __forceinline__ void split3_pair(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
  h = cvt_pk_bf16(x0, x1);
  const float r0 = x0 - __uint_as_float(h << 16), r1 = x1 - __uint_as_float(h & 0xffff0000u);
  m = cvt_pk_bf16(r0, r1);
  const float s0 = r0 - __uint_as_float(m << 16), s1 = r1 - __uint_as_float(m & 0xffff0000u);
  l = cvt_pk_bf16(s0, s1);
}

// the six products of bf16x6, smallest first: (A part, B part) = (l,h) (h,l) (m,m) (m,h) (h,m) (h,h), parts indexed h, m, l = 0, 1, 2
__device__ constexpr int kX6A[6] = {2, 0, 1, 1, 0, 0};
__device__ constexpr int kX6B[6] = {0, 2, 1, 0, 1, 0};

// D += A*B with A = (ah, am, al), B = (bh, bm, bl)
__device__ __forceinline__ f32x4 mfma_bf16x6(const u32x4 (&a)[3], const u32x4 (&b)[3], f32x4 c) {
#pragma unroll
  for (int term = 0; term < 6; ++term) c = mfma16x16x32_bf16(a[kX6A[term]], b[kX6B[term]], c);
  return c;
}

__device__ __forceinline__ unsigned short bf16_bits(float x) { return (unsigned short)(cvt_pk_bf16(x, 0.f) & 0xFFFFu); }
__device__ __forceinline__ float bf16_to_f32(unsigned short b) { return __uint_as_float((unsigned)b << 16); }
typedef short s16x4 __attribute__((ext_vector_type(4)));   // what ds_read_b64_tr_b16 returns (__builtin_amdgcn_ds_read_tr16_b64_v4i16)
constexpr float kLog2e = 1.4426950408889634f;   // scores live in the log2 domain: softmax exponentials are bare v_exp_f32

// ---------------------------------------------------------------------------------------------
// fp32 GEMM on the f16 matrix instructions ("f16x3", round 2; residual scaling completed in round 3): half the matrix
// instructions and less than half the split work of bf16x6, for products that are fp32-grade (1e-7 relative in a K = 256 GEMM,
// numpy emulation in tests/test_f16x3_emulation.py) for 2^-14 <= |x| < 65504 -- and degrade gracefully below (absolute 2^-36):
//   x = xh + xm,  xh = f16(x),        xm' = f16((x - xh) * 2^11)      (11 + 11 significant bits; 5 VALU slots per PAIR:
//   w = wh + wm,  wh = f16(w * 2^s),  wm' = f16((w * 2^s - wh) * 2^11)  v_cvt_pk_f16_f32, two v_fma_mix_f32, v_fma_mixlo/hi_f16)
//   2^(11+s) w x ~= wm' * xh + wh * xm' + (wh * 2^11) * xh            (dropped: wm xm <= 2^-22 |w x|)
// BOTH residuals are stored SCALED by 2^11, so neither is an f16 subnormal at any magnitude its leading part represents (round
// 2 left the activation residual unscaled: an absolute floor of 3e-8 per activation, i.e. 2e-5 relative for activations of
// 1e-3 -- VERDICT r02, tests/test_f16x3_lowend_gpu.py).  The three products then sit at one scale, 2^(11+s) times the true one,
// in ONE accumulator: the leading product takes whB = wh * 2^11 (exact; formed from wh by v_pk_mul_f16 where an operand is read,
// or stored as a third image where the table is small), and the consumer multiplies by 2^-(11+s) where it adds the bias (an FMA
// in place of an add).  s is chosen per weight matrix when it is packed so that max |w| 2^s is in [8, 16): whB <= 2^15, no
// overflow at any weight magnitude.  MFMA operands and the conversions keep f16 subnormals (hipcc's default
// float_denorm_mode_16_64 = 3).
// ---------------------------------------------------------------------------------------------
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2v __attribute__((ext_vector_type(2)));

constexpr float kF16ResidualScale = 2048.0f;          // 2^11
constexpr float kF16OutputScale = 1.0f / 2048.0f;     // what the accumulator of an f16x3 product chain is multiplied by (times 2^-s)

__device__ __forceinline__ f32x4 mfma16x16x32_f16(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// split of a pair of floats into the two f16x3 operands: h = (xh0, xh1), m = (xm0', xm1') with xm' = f16((x - xh) * 2^11)
__device__ __forceinline__ void split_f16_pair(float x0, float x1, unsigned& h, unsigned& m) {
  const f16x2v hh = __builtin_convertvector(f32x2{x0, x1}, f16x2v);   // the FIRST read of x0 / x1 is compiler-visible
  h = __builtin_bit_cast(unsigned, hh);
  float r0, r1;   // x - xh (exact in fp32) in one instruction each: f16 operand read straight from the packed pair
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r0) : "v"(h), "v"(x0));
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r1) : "v"(h), "v"(x1));
  // f16(r * 2^11) straight into the two halves of m (fp32 product, one rounding; the constant rides in an SGPR: VOP3P takes no literal)
  const float k = kF16ResidualScale;
  asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(m) : "v"(r0), "s"(k));
  asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(m) : "v"(r1), "s"(k));
}

// The round-2 form of the split, kept for operands whose SCALE is fixed by construction -- the output of a LayerNorm without its
// affine part (|x| <= sqrt(C), O(1) entries): h = (xh0, xh1), s = h * 2^-11, m = (xm0, xm1) UNSCALED, to go with weights packed
// with s = 0 as (wh, wm' = (w - wh) * 2^11):  w x ~= wm' * xs + wh * xm + wh * xh at the TRUE scale (no multiply behind the
// accumulator).  xs and xm are f16 subnormals for |x| < 0.125; the bits that drops are an ABSOLUTE 3e-8 per element, i.e.
// fp32-grade against a dot product over O(1) entries -- and wrong by 3e-8 / |x| for inputs that are small as a whole, which is
// why every other operand takes split_f16_pair above.
__device__ __forceinline__ void split_f16_pair_unit(float x0, float x1, unsigned& h, unsigned& s, unsigned& m) {
  const f16x2v hh = __builtin_convertvector(f32x2{x0, x1}, f16x2v);
  h = __builtin_bit_cast(unsigned, hh);
  float r0, r1;
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r0) : "v"(h), "v"(x0));
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r1) : "v"(h), "v"(x1));
  m = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{r0, r1}, f16x2v));
  s = __builtin_bit_cast(unsigned, hh * f16x2v{(_Float16)0.00048828125f, (_Float16)0.00048828125f});
}

// max |w| of n floats as the bits of a non-negative float (monotone as unsigned); *out must be zero before the launch.
// gamma (or null): the maximum of |w[i] * gamma[i % ld]| instead (a LayerNorm's scale folded into the matrix)
static __global__ __launch_bounds__(256) void absmax_bits_kernel(const float* __restrict__ w, long long n, unsigned* __restrict__ out,
                                                                 const float* __restrict__ gamma = nullptr, int ld = 1) {
  unsigned m = 0u;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float v = gamma ? w[i] * gamma[i % ld] : w[i];
    const unsigned b = __float_as_uint(v) & 0x7fffffffu;
    if (b <= 0x7f800000u && b > m) m = b;                      // NaNs do not take part
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned o = __shfl_xor(m, off);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

// 2^s with max |w| 2^s in [8, 16), from the bits absmax_bits_kernel left (1 for a zero, subnormal or infinite maximum);
// `oscale` = 2^-(11+s), what a consumer multiplies the accumulator of the three f16 products by
__device__ __forceinline__ float f16x3_weight_scale(unsigned maxbits, float& oscale) {
  const int e = (int)(maxbits >> 23);                          // biased exponent of the maximum
  if (e < 16 || e > 250) { oscale = kF16OutputScale; return 1.f; }
  oscale = __uint_as_float((unsigned)(e - 14) << 23);          // 2^(e - 127 - 3 - 11)
  return __uint_as_float((unsigned)(257 - e) << 23);           // 2^(3 - (e - 127))
}

// 1 / p for p a power of two (exact)
__device__ __forceinline__ float pow2_reciprocal(float p) { return __uint_as_float(0x7f000000u - __float_as_uint(p)); }

// whB = wh * 2^11 of an operand fragment (exact: a power of two, |wh| < 16 by the packers' choice of s)
__device__ __forceinline__ u32x4 f16x8_times_2048(u32x4 wh) {
  const _Float16 k1 = (_Float16)2048.0f;
  const f16x8 k = {k1, k1, k1, k1, k1, k1, k1, k1};
  return __builtin_bit_cast(u32x4, __builtin_bit_cast(f16x8, wh) * k);
}

// D += 2^(11+s) A*B with A = (wh, wm', whB), B = (xh, xm' [, unused]): the two residual products first
__device__ __forceinline__ f32x4 mfma_f16x3(const u32x4 (&a)[3], const u32x4 (&b)[3], f32x4 c) {
  c = mfma16x16x32_f16(a[1], b[0], c);
  c = mfma16x16x32_f16(a[0], b[1], c);
  c = mfma16x16x32_f16(a[2], b[0], c);
  return c;
}

// the two forms behind one name (F16 = f16x3, else bf16x6); part order of the operand: bf16x6 (h, m, l), f16x3 (xh, xm', 0)
template <bool F16>
__device__ __forceinline__ void split_pair_x(float x0, float x1, unsigned& p0, unsigned& p1, unsigned& p2) {
  if constexpr (F16) {
    split_f16_pair(x0, x1, p0, p1);
    p2 = 0u;
  } else {
    split3_pair(x0, x1, p0, p1, p2);
  }
}
template <bool F16>
__device__ __forceinline__ f32x4 mfma_x(const u32x4 (&a)[3], const u32x4 (&b)[3], f32x4 c) {
  if constexpr (F16) return mfma_f16x3(a, b, c);
  else return mfma_bf16x6(a, b, c);
}

// host: s with max |w| 2^s in [8, 16) (0 for an all-zero or non-finite maximum)
inline int f16x3_weight_shift(float wmax) {
  if (!(wmax > 0.f) || !std::isfinite(wmax)) return 0;
  int e;
  std::frexp(wmax, &e);          // wmax = f 2^e, f in [0.5, 1)
  return 4 - e;
}

// host: the two f16 parts of a weight already multiplied by 2^s (RNE; residual scaled by 2^11, see above)
inline void split2_host_f16(float x, uint16_t& h, uint16_t& m) {
  const _Float16 hh = (_Float16)x;
  const _Float16 mm = (_Float16)((x - (float)hh) * 2048.0f);
  std::memcpy(&h, &hh, 2);
  std::memcpy(&m, &mm, 2);
}

// host: whB = wh * 2^11 of a leading part produced by split2_host_f16
inline uint16_t f16_times_2048_host(uint16_t h) {
  _Float16 hh;
  std::memcpy(&hh, &h, 2);
  const _Float16 b = (_Float16)((float)hh * 2048.0f);
  uint16_t o;
  std::memcpy(&o, &b, 2);
  return o;
}

// host: round-to-nearest-even bf16 split of one float (matches v_cvt_pk_bf16_f32 for finite values)
inline void split3_host(float x, uint16_t& h, uint16_t& m, uint16_t& l) {
  auto to_bf16 = [](float v) -> uint16_t {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
  };
  auto from_bf16 = [](uint16_t b) -> float {
    uint32_t u = (uint32_t)b << 16;
    float v;
    std::memcpy(&v, &u, 4);
    return v;
  };
  h = to_bf16(x);
  const float r = x - from_bf16(h);
  m = to_bf16(r);
  const float s2 = r - from_bf16(m);
  l = to_bf16(s2);
}

}  // namespace dlwp
