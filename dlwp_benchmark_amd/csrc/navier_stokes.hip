// Trajectories of the 2-D incompressible Navier-Stokes equations in vorticity form on the unit torus, one workgroup per
// trajectory with the spectrum resident in LDS for the whole launch (the scheme: include/dlwp_hip.h at
// dlwp_ns2d_rollout_f32).  The reference tree holds no solver (PARITY UNPINNED): tests/ns_ref.py restates the scheme in float64.
//
// LDS (n = 64: 126 208 B, n = 32: 32 384 B):
//   Z   [2][n][n + 1] float2   the two complex work planes; a row is n + 1 long, so that the 32 lanes of a half-wave that walk
//                              rows (row passes) or columns (column passes) fall on 32 different bank pairs
//   W   [n][n / 2 + 1] float2  wh, the half-plane spectrum of the vorticity -- the state
//   C   [n][n / 2 + 1] float2  dt fh / (1 + dt nu lap / 2), the forcing's share of a sub-step
//   tw  [n] float2             exp(-2 pi i j / n) from the host's float64 table (a kernel argument)
//   ca, cb, cq [n][n / 2 + 1]  (1 - dt nu lap / 2) / (1 + dt nu lap / 2),  mask dt / (1 + dt nu lap / 2),  2 pi / (lapi n^2):
//                              made in float64 at the head of the kernel, rounded once
//
// A 2-D transform is four passes of the radix butterflies of fft_radix.hpp over a plane in LDS (rows: pass 1, pass 2; columns:
// pass 1, pass 2) with a barrier behind each; pass 2 stores in place, so index k of either axis ends at pos<A, B>(k) and the
// reader of the result undoes that: no plane is ever copied.  Real fields travel in pairs: with real p, q the plane P + i Q
// (P, Q their Hermitian spectra) is the spectrum of p + i q, so
//   Z[0] = (ka + i kb) 2 pi wh / lapi     -> u + i v          Z[1] = (-kb + i ka) 2 pi wh    -> wa + i wb
// are two complex inverses, run as one batch of 2 n rows / 2 n columns, and the product u wa + v wb goes forward as one complex
// plane with a zero imaginary part: two inverses and one forward per sub-step.  The half-plane state reaches the other half of
// a plane as Z[-k] = m(-k) conj(wh[k]) (m odd for the derivatives, even for the frame output).
//
// Every sum runs in a fixed order in one thread: no atomics, no inline assembly, no traffic between workgroups.
#include "common.hpp"
#include "fft_radix.hpp"

namespace dlwp {
namespace ns2d {

constexpr int kThreads = 512;
// frames * substeps of one launch.  Measured on MI355X (profiles/navier_stokes_mi355x.json): a sub-step of a resident
// trajectory takes 9.8 us at n = 64 (3.8 us at n = 32), so the longest launch the cap admits runs 1.0 s per 256 trajectories
// (one per compute unit), 3.9 s at a batch of 1024.
constexpr long long kMaxSteps = 100000;

struct Twiddles {
  float2 w[64];               // exp(-2 pi i j / n), j < n
};

template <int N>
struct Split;
template <>
struct Split<32> { static constexpr int A = 4, B = 8; };
template <>
struct Split<64> { static constexpr int A = 8, B = 8; };

template <int N>
constexpr size_t lds_bytes() {
  return (size_t)2 * N * (N + 1) * 8 + (size_t)2 * N * (N / 2 + 1) * 8 + (size_t)N * 8 + (size_t)3 * N * (N / 2 + 1) * 4;
}

// pass 1 of one transform whose element n lives at p[n * es]: radix-A butterflies over n2 of x[n1 + B n2], twiddled, in place
template <int A, int B, int SIGN>
__device__ __forceinline__ void pass1(float2* p, int es, int n1, const float2* tw) {
  float2 v[A];
#pragma unroll
  for (int n2 = 0; n2 < A; ++n2) v[n2] = p[(n1 + B * n2) * es];
  afft::Dft<A, SIGN>::run(v);
#pragma unroll
  for (int k2 = 0; k2 < A; ++k2) {
    float2 w = tw[n1 * k2];
    if (SIGN > 0) w.y = -w.y;
    p[(n1 + B * k2) * es] = k2 == 0 ? v[0] : afft::cmul(v[k2], w);
  }
}
// pass 2: radix-B over the B values at B k2 + n1, stored where they were read: X[k] ends at pos<A, B>(k)
template <int A, int B, int SIGN>
__device__ __forceinline__ void pass2(float2* p, int es, int k2) {
  float2 v[B];
#pragma unroll
  for (int n1 = 0; n1 < B; ++n1) v[n1] = p[(B * k2 + n1) * es];
  afft::Dft<B, SIGN>::run(v);
#pragma unroll
  for (int k1 = 0; k1 < B; ++k1) p[(B * k2 + k1) * es] = v[k1];
}

// the 2-D transform of the first `planes` planes of Z, in place; on return (a barrier included) element (k0, k1) of a plane is at
// [pos(k0)][pos(k1)].  The caller has put a barrier behind its writes of Z.
template <int N, int SIGN>
__device__ __forceinline__ void fft2d(float2* Z, int planes, const float2* tw, int tid) {
  constexpr int A = Split<N>::A, B = Split<N>::B, S = N + 1;
  const int rows = planes * N;
  for (int it = tid; it < rows * B; it += kThreads) pass1<A, B, SIGN>(Z + (it % rows) * S, 1, it / rows, tw);
  __syncthreads();
  for (int it = tid; it < rows * A; it += kThreads) pass2<A, B, SIGN>(Z + (it % rows) * S, 1, it / rows);
  __syncthreads();
  for (int it = tid; it < rows * B; it += kThreads) {       // rows = planes * N columns as well
    const int c = it % N, q = it / N, z = q % planes;
    pass1<A, B, SIGN>(Z + z * N * S + c, S, q / planes, tw);
  }
  __syncthreads();
  for (int it = tid; it < rows * A; it += kThreads) {
    const int c = it % N, q = it / N, z = q % planes;
    pass2<A, B, SIGN>(Z + z * N * S + c, S, q / planes);
  }
  __syncthreads();
}

// what a half-plane mode (row i, column j) does when the planes are filled
enum ModeKind {
  kModeZero = 0,              // |ka| = N / 2 or kb = N / 2: the state is zero there, the planes get zeros (mirror included)
  kModeSelf = 1,              // k = 0: its own mirror
  kModePair = 2,              // writes [i][j] and the mirror [(N - i) % N][(N - j) % N]
  kModeSkip = 3               // column 0, ka < 0: written by its partner (i' = N - i), the state there is never read
};
template <int N>
__device__ __forceinline__ int mode_kind(int i, int j) {
  if (2 * i == N || 2 * j == N) return kModeZero;
  if (j == 0) return i == 0 ? kModeSelf : (2 * i < N ? kModePair : kModeSkip);
  return kModePair;
}
// whether the mode fills its mirror too: the column kb = N / 2 mirrors onto itself, a mode of its own fills that entry
template <int N>
__device__ __forceinline__ bool has_mirror(int kind, int j) { return kind == kModePair || (kind == kModeZero && 2 * j != N); }

template <int N>
__global__ __launch_bounds__(kThreads) void rollout_kernel(const float* w0, const float* __restrict__ filter,
                                                           const float* __restrict__ forcing, float* out, int frames,
                                                           int substeps, double dt, double nu, Twiddles twiddles) {
  constexpr int A = Split<N>::A, B = Split<N>::B, S = N + 1, H = N / 2 + 1, NH = N * H, NN = N * N;
  constexpr int kPoints = NN / kThreads;                    // grid points a thread multiplies
  static_assert(NN % kThreads == 0 && A * B == N, "the point loop has no tail");
  extern __shared__ __align__(16) unsigned char smem[];
  float2* Z = reinterpret_cast<float2*>(smem);
  float2* W = Z + 2 * N * S;
  float2* C = W + NH;
  float2* tw = C + NH;
  float* ca = reinterpret_cast<float*>(tw + N);
  float* cb = ca + NH;
  float* cq = cb + NH;
  const int tid = threadIdx.x;
  const size_t traj = blockIdx.x;
  const float* w0b = w0 + traj * NN;
  float* outb = out + traj * (size_t)frames * NN;
  constexpr float kInvNN = 1.0f / (float)NN;                // a power of two
  constexpr float kTwoPiNN = (float)(6.283185307179586476925 / (double)NN);

  // ---- tables, and the transforms of w0 (plane 1) and of the forcing (plane 0) as one batch ----
  for (int t = tid; t < N; t += kThreads) tw[t] = twiddles.w[t];
  for (int e = tid; e < NH; e += kThreads) {
    const int i = e / H, j = e - i * H, ka = 2 * i < N ? i : i - N;
    const double k2 = (double)(ka * ka + j * j), lap = 39.47841760435743447534 * k2;         // 4 pi^2 |k|^2
    const double half = 0.5 * dt * nu * lap, den = 1.0 + half;
    const bool keep = 3 * abs(ka) <= N && 3 * j <= N;        // the 2/3 rule
    ca[e] = (float)((1.0 - half) / den);
    cb[e] = keep ? (float)(dt / den) : 0.f;
    cq[e] = (float)(6.283185307179586476925 / ((e == 0 ? 1.0 : lap) * (double)NN));
  }
  for (int e = tid; e < NN; e += kThreads) {
    const int r = e / N, c = e - r * N;
    Z[r * S + c] = float2{forcing ? forcing[e] : 0.f, 0.f};
    Z[(N + r) * S + c] = float2{w0b[e], 0.f};
  }
  __syncthreads();
  fft2d<N, -1>(Z, 2, tw, tid);
  for (int e = tid; e < NH; e += kThreads) {
    const int i = e / H, j = e - i * H;
    const int kind = mode_kind<N>(i, j);
    const int at = afft::pos<A, B>(i) * S + afft::pos<A, B>(j);
    float2 fh = Z[at], wh = Z[N * S + at];
    if (filter) {
      const float f = filter[e];
      wh = float2{wh.x * f, wh.y * f};
    }
    if (kind == kModeZero || kind == kModeSkip) fh = wh = float2{0.f, 0.f};
    if (kind == kModeSelf) fh.y = wh.y = 0.f;                // the mean of a real field
    const int ka = 2 * i < N ? i : i - N;
    const double lap = 39.47841760435743447534 * (double)(ka * ka + j * j);
    const float g = (float)(dt / (1.0 + 0.5 * dt * nu * lap));
    C[e] = float2{fh.x * g, fh.y * g};
    W[e] = wh;
  }
  __syncthreads();            // the planes have been read

  for (int frame = 0;; ++frame) {
    // ---- frame output: irfft2(wh) through plane 0 ----
    for (int e = tid; e < NH; e += kThreads) {
      const int i = e / H, j = e - i * H;
      const int kind = mode_kind<N>(i, j);
      if (kind == kModeSkip) continue;
      const float2 w = W[e];
      const float2 z = kind == kModeZero ? float2{0.f, 0.f} : float2{w.x * kInvNN, w.y * kInvNN};
      Z[i * S + j] = z;
      if (has_mirror<N>(kind, j)) Z[((N - i) % N) * S + (N - j) % N] = float2{z.x, -z.y};
    }
    __syncthreads();
    fft2d<N, +1>(Z, 1, tw, tid);
    float* dst = outb + (size_t)frame * NN;
    for (int e = tid; e < NN; e += kThreads) {
      const int r = e / N, c = e - r * N;
      dst[e] = Z[afft::pos<A, B>(r) * S + afft::pos<A, B>(c)].x;
    }
    if (frame == frames - 1) break;
    __syncthreads();          // plane 0 has been read

    for (int step = 0; step < substeps; ++step) {
      // ---- the two packed planes from the state ----
      for (int e = tid; e < NH; e += kThreads) {
        const int i = e / H, j = e - i * H;
        const int kind = mode_kind<N>(i, j);
        if (kind == kModeSkip) continue;
        const float fa = (float)(2 * i < N ? i : i - N), fb = (float)j;
        const float2 w = kind == kModeZero ? float2{0.f, 0.f} : W[e];
        const float q = cq[e];
        // (ka + i kb) w and (-kb + i ka) w, then the same of conj(w) with the sign of m(-k) = -m(k)
        const float2 z1 = float2{q * (fa * w.x - fb * w.y), q * (fa * w.y + fb * w.x)};
        const float2 z2 = float2{kTwoPiNN * (-fb * w.x - fa * w.y), kTwoPiNN * (fa * w.x - fb * w.y)};
        Z[i * S + j] = z1;
        Z[(N + i) * S + j] = z2;
        if (has_mirror<N>(kind, j)) {
          const int mi = (N - i) % N, mj = (N - j) % N;
          Z[mi * S + mj] = float2{-(q * (fa * w.x + fb * w.y)), -(q * (fb * w.x - fa * w.y))};
          Z[(N + mi) * S + mj] = float2{-(kTwoPiNN * (fa * w.y - fb * w.x)), -(kTwoPiNN * (fa * w.x + fb * w.y))};
        }
      }
      __syncthreads();
      fft2d<N, +1>(Z, 2, tw, tid);
      // ---- u wa + v wb at every grid point: read where the transform left it, written in natural order behind a barrier ----
      float g[kPoints];
#pragma unroll
      for (int r = 0; r < kPoints; ++r) {
        const int e = tid + r * kThreads, pr = e / N, pc = e - pr * N;
        const float2 uv = Z[pr * S + pc], wab = Z[(N + pr) * S + pc];
        g[r] = uv.x * wab.x + uv.y * wab.y;
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < kPoints; ++r) {
        const int e = tid + r * kThreads, pr = e / N, pc = e - pr * N;
        // the index whose pos<A, B> is p: p = B k2 + k1 holds k2 + A k1
        const int n0 = pr / B + A * (pr % B), n1 = pc / B + A * (pc % B);
        Z[n0 * S + n1] = float2{g[r], 0.f};
      }
      __syncthreads();
      fft2d<N, -1>(Z, 1, tw, tid);
      // ---- Crank-Nicolson update of the state ----
      for (int e = tid; e < NH; e += kThreads) {
        const int i = e / H, j = e - i * H;
        const int kind = mode_kind<N>(i, j);
        if (kind == kModeZero || kind == kModeSkip) continue;
        const float2 F = Z[afft::pos<A, B>(i) * S + afft::pos<A, B>(j)], w = W[e], c = C[e];
        const float a = ca[e], b = cb[e];
        float2 nw = float2{a * w.x - b * F.x + c.x, a * w.y - b * F.y + c.y};
        if (kind == kModeSelf) nw.y = 0.f;
        W[e] = nw;
      }
      __syncthreads();        // plane 0 has been read; the state is whole
    }
  }
}

}  // namespace ns2d
}  // namespace dlwp

using namespace dlwp;

template <int N>
static int32_t ns2d_launch(const float* w0, const float* filter, const float* forcing, float* out, int32_t batch, int32_t frames,
                           int32_t substeps, double dt, double nu, hipStream_t stream) {
  ns2d::Twiddles tw;
  for (int j = 0; j < 64; ++j) {
    const double phi = -2.0 * 3.14159265358979323846 * (double)(j % N) / (double)N;
    tw.w[j] = float2{(float)std::cos(phi), (float)std::sin(phi)};
  }
  constexpr size_t lds = ns2d::lds_bytes<N>();
  static_assert(lds <= 160 * 1024, "one workgroup's LDS");
  auto kernel = ns2d::rollout_kernel<N>;
  if (lds > 48 * 1024)
    DLWP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, dim3((unsigned)batch), dim3(ns2d::kThreads), lds, stream, w0, filter, forcing, out, (int)frames,
                     (int)substeps, dt, nu, tw);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" int32_t dlwp_ns2d_rollout_f32(const float* w0_dev, const float* filter_dev, const float* forcing_dev, float* out_dev,
                                         int32_t batch, int32_t n, int32_t frames, int32_t substeps, double dt, double nu,
                                         void* stream) {
  DLWP_REQUIRE(w0_dev && out_dev, DLWP_ERR_INVALID_ARGUMENT, "ns2d: null argument");
  DLWP_REQUIRE(batch >= 1 && frames >= 1 && substeps >= 1, DLWP_ERR_INVALID_ARGUMENT,
               "ns2d: batch %d, frames %d and substeps %d must be at least 1", batch, frames, substeps);
  DLWP_REQUIRE(std::isfinite(dt) && dt > 0.0 && std::isfinite(nu) && nu >= 0.0, DLWP_ERR_INVALID_ARGUMENT,
               "ns2d: dt = %g must be positive and nu = %g non-negative, both finite", dt, nu);
  DLWP_REQUIRE(n == 32 || n == 64, DLWP_ERR_UNSUPPORTED,
               "ns2d: n = %d; the resident kernel runs 32 x 32 and 64 x 64 (the work planes of 128 x 128 exceed 160 KiB of LDS)", n);
  DLWP_REQUIRE((long long)frames * substeps <= ns2d::kMaxSteps, DLWP_ERR_UNSUPPORTED,
               "ns2d: frames * substeps = %lld exceeds the %lld of one launch; split the trajectory", (long long)frames * substeps,
               ns2d::kMaxSteps);
  DLWP_REQUIRE(frames == 1 || out_dev != w0_dev, DLWP_ERR_INVALID_ARGUMENT, "ns2d: out may be w0 itself only with frames == 1");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return n == 32 ? ns2d_launch<32>(w0_dev, filter_dev, forcing_dev, out_dev, batch, frames, substeps, dt, nu, s)
                 : ns2d_launch<64>(w0_dev, filter_dev, forcing_dev, out_dev, batch, frames, substeps, dt, nu, s);
}
