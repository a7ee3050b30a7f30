// Zonal energy spectrum sums of a rollout and its targets (reference scripts/losses.py:16-152: `ZonalSpectrum.compute` +
// `MELRCalculator.apply`), reduced on the device.  For every row f[n] (n over the W longitudes) of out / target
// [B, K, C, H, W]:
//   F[m] = (1/W) sum_n f[n] exp(-2 pi i m n / W),  m = 0 .. W/2           (np.fft.rfft(norm='forward'), losses.py:39)
//   P[m] = |F[m]|^2 * (m == 0 ? 1 : 2)                                     (the Nyquist bin doubled too, :40-43)
//   sums[q][k][c][m] = sum_{b,h} circ_h P_q[b, k, c, h, m],  q = 0: out, 1: target   (circ_h: losses.py:20-23,69-71)
// E = sums / (B H) is the reference's sample- and latitude-mean (:107-108); the log ratio and MELR (:117-121) are taken
// from E by the caller (metrics.ZonalSpectrumMetrics).
//
// Decomposition: the rows of one (k, c) plane -- B H of them, b-major -- are cut into S segments of whole row chunks;
// one workgroup per (segment, k c, q).  A workgroup walks its segment RCH rows at a time (RCH W / 2 = 4096 complex
// values in LDS): the real length-W row FFT is the complex length-W/2 FFT of the (even, odd) pairs (the two register
// passes of fft_radix.hpp), then the split post-pass forms F[k] and F[W/2 - k] of one item and overwrites their two
// slots with the powers (no second buffer); the next chunk's global loads are in flight in registers meanwhile.  Every
// thread owns one spectrum slot p and one row group g (rows g, g + G, ... of the chunk), and adds circ_h P in double in
// row order.  At the end the G row groups are added in order and the workgroup writes its [W/2 + 1] double partial to
// the workspace; a second kernel adds the S partials of every (q, k, c, m) in segment order.  No atomics: the sums are
// bitwise reproducible.  Powers are fp32 (fp32 transform), weights and every sum across rows fp64.
#include "common.hpp"
#include "fft_radix.hpp"

namespace dlwp {
namespace zspec {

using namespace afft;

constexpr int NT = 256;

// row FFT of W/2 = A * B; RCH rows per chunk: RCH * W/2 = 4096 complex values (32 KiB of LDS) for every width
template <int W>
struct Cfg;
template <> struct Cfg<32> { static constexpr int A = 4, B = 4; };
template <> struct Cfg<64> { static constexpr int A = 4, B = 8; };
template <> struct Cfg<128> { static constexpr int A = 8, B = 8; };
template <> struct Cfg<256> { static constexpr int A = 8, B = 16; };
template <> struct Cfg<512> { static constexpr int A = 16, B = 16; };

template <int W>
constexpr int rows_per_chunk() { return 8192 / W; }

template <int W>
__global__ __launch_bounds__(NT) void zonal_power_partials_kernel(const float* __restrict__ out, const float* __restrict__ tar,
                                                                  const double* __restrict__ circ,   // [H]
                                                                  double* __restrict__ part,         // [2][KC][S][NR + 1]
                                                                  int H, long long rows, long long seg_rows, int KC) {
  constexpr int NR = W / 2, A = Cfg<W>::A, B = Cfg<W>::B, RCH = rows_per_chunk<W>();
  constexpr int RS = NR + 1;                    // odd LDS stride (float2), as afno_fft.hip
  constexpr int F4R = W / 4;                    // float4 per row
  constexpr int PF = RCH * F4R / NT;            // float4 per thread and chunk (exact: 8)
  constexpr int NH = NR / 2 + 1;                // post-pass items per row: bins k and NR - k together
  constexpr int G = NT / NR;                    // row groups of the reduction
  static_assert(A * B == NR && PF * NT == RCH * F4R && G * NR == NT && RCH <= NT, "decomposition");
  __shared__ float2 rb[RCH * RS];
  __shared__ float2 s_twr[NR];                  // exp(-2 pi i j / NR)
  __shared__ float2 s_tww[NH];                  // exp(-2 pi i k / W), k <= NR / 2
  __shared__ double s_circ[RCH];
  const int tid = threadIdx.x;
  const int seg = blockIdx.x, kc = blockIdx.y, q = blockIdx.z;
  const float* __restrict__ x = q ? tar : out;
  for (int j = tid; j < NR; j += NT) {
    double sn, cs;
    sincospi(2.0 * j / NR, &sn, &cs);
    s_twr[j] = float2{(float)cs, (float)-sn};
  }
  for (int k = tid; k < NH; k += NT) {
    double sn, cs;
    sincospi(2.0 * k / W, &sn, &cs);
    s_tww[k] = float2{(float)cs, (float)-sn};
  }
  const long long lo = seg * seg_rows, hi = lo + seg_rows < rows ? lo + seg_rows : rows;
  // rows of the plane are (b, h), b-major: row j lives at ((b KC + kc) H + h) W
  float4 pre[PF];
  auto prefetch = [&](long long row0) {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int i = tid + u * NT;
      const long long j = row0 + i / F4R;
      if (j < hi) {
        const long long b = j / H, h = j - b * H;
        pre[u] = reinterpret_cast<const float4*>(x + ((b * KC + kc) * H + h) * W)[i % F4R];
      } else {
        pre[u] = float4{0.f, 0.f, 0.f, 0.f};
      }
    }
  };
  const int p = tid % NR, g = tid / NR;         // the spectrum slot and row group this thread reduces
  double acc = 0.0, acc_nyq = 0.0;
  constexpr float inv = 1.0f / ((float)W * (float)W);   // norm='forward' squared (a power of two: exact)
  prefetch(lo);
  for (long long row0 = lo; row0 < hi; row0 += RCH) {
    // (a) the chunk's rows into LDS: a float4 is two complex values z[n] = x[2n] + i x[2n+1]
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int i = tid + u * NT;
      const int r = i / F4R, m = i % F4R;
      rb[r * RS + 2 * m] = float2{pre[u].x, pre[u].y};
      rb[r * RS + 2 * m + 1] = float2{pre[u].z, pre[u].w};
    }
    if (tid < RCH) s_circ[tid] = row0 + tid < hi ? circ[(row0 + tid) % H] : 0.0;
    if (row0 + RCH < hi) prefetch(row0 + RCH);
    __syncthreads();
    fft_pass1<A, B, -1, NT>(rb, RS, RCH, s_twr, tid);
    __syncthreads();
    fft_pass2_inplace<A, B, -1, NT>(rb, RS, RCH, tid);      // Z[k] now sits at pos<A, B>(k)
    __syncthreads();
    // (b) split post-pass, in place: the item (r, k) reads Z[k] and Z[NR - k] and leaves in their slots
    //     P[k] and P[NR - k] (k = 0: P[0] in .x and the Nyquist bin P[NR] in .y of slot pos(0))
    //     F[k] = s/2 - (i/2) t,  F[NR - k] = conj(s/2 + (i/2) t),  s = Z[k] + conj Z[NR-k],  t = w_W^k (Z[k] - conj Z[NR-k])
    for (int it = tid; it < RCH * NH; it += NT) {
      const int k = it % NH, r = it / NH;
      float2* row = rb + r * RS;
      const int pk = pos<A, B>(k), pc = pos<A, B>((NR - k) % NR);
      const float2 zk = row[pk], zc = cconj(row[pc]);
      const float2 s = cadd(zk, zc), dd = csub(zk, zc);
      const float2 t = cmul(s_tww[k], dd);
      const float fx = 0.5f * (s.x + t.y), fy = 0.5f * (s.y - t.x);
      const float gx = 0.5f * (s.x - t.y), gy = 0.5f * (s.y + t.x);
      const float p_k = (fx * fx + fy * fy) * (k == 0 ? inv : 2.f * inv);
      const float p_c = (gx * gx + gy * gy) * (2.f * inv);
      if (k == 0) {
        row[pk] = float2{p_k, p_c};
      } else {
        row[pk] = float2{p_k, 0.f};
        if (2 * k != NR) row[pc] = float2{p_c, 0.f};
      }
    }
    __syncthreads();
    // (c) fixed-order weighted sum over the chunk's rows of this thread's group
    const int nr = hi - row0 < RCH ? (int)(hi - row0) : RCH;
    for (int r = g; r < nr; r += G) {
      const float2 v = rb[r * RS + p];
      acc += s_circ[r] * (double)v.x;
      if (p == 0) acc_nyq += s_circ[r] * (double)v.y;
    }
    __syncthreads();   // rb and s_circ are rewritten by the next chunk
  }
  // row groups in order; slot p holds bin a + A b' (p = B a + b')
  double* red = reinterpret_cast<double*>(rb);   // [G][NR] | nyq [G]
  red[g * NR + p] = acc;
  if (p == 0) red[G * NR + g] = acc_nyq;
  __syncthreads();
  double* dst = part + (((long long)q * KC + kc) * gridDim.x + seg) * (NR + 1);
  if (tid < NR) {
    double tot = 0.0;
    for (int gg = 0; gg < G; ++gg) tot += red[gg * NR + tid];
    dst[tid / B + A * (tid % B)] = tot;
  }
  if (tid == NT - 1) {
    // the Nyquist bin (for W = 512 this thread also wrote a slot above)
    double tot = 0.0;
    for (int gg = 0; gg < G; ++gg) tot += red[G * NR + gg];
    dst[NR] = tot;
  }
}

// sums[i] (+)= sum over the S segments of part[i / NB][s][i % NB], in segment order
__global__ __launch_bounds__(256) void zonal_power_combine_kernel(const double* __restrict__ part, double* __restrict__ sums,
                                                                  int n, int S, int NB, int accumulate) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* src = part + (long long)(i / NB) * S * NB + i % NB;
  double tot = 0.0;
  for (int s = 0; s < S; ++s) tot += src[(long long)s * NB];
  sums[i] = accumulate ? sums[i] + tot : tot;
}

}  // namespace zspec
}  // namespace dlwp

using namespace dlwp;

namespace {
bool width_supported(int32_t w) { return w == 32 || w == 64 || w == 128 || w == 256 || w == 512; }

// rows per segment (a multiple of the chunk) and segments per (k, c) plane: about 1024 workgroups in all, a function of the
// shape alone, so the workspace size and the summation order do not depend on the device
struct Split {
  long long rows = 0, seg_rows = 0, segs = 0;
};
Split split_of(int32_t batch, int32_t steps, int32_t channels, int32_t height, int32_t width) {
  Split sp;
  const long long kc = (long long)steps * channels, rch = 8192 / width;
  sp.rows = (long long)batch * height;
  long long want = (1024 + 2 * kc - 1) / (2 * kc);
  const long long max_segs = (sp.rows + rch - 1) / rch;
  if (want < 1) want = 1;
  if (want > max_segs) want = max_segs;
  sp.seg_rows = (sp.rows + want - 1) / want;
  sp.seg_rows = (sp.seg_rows + rch - 1) / rch * rch;
  sp.segs = (sp.rows + sp.seg_rows - 1) / sp.seg_rows;
  return sp;
}

bool shape_ok(int32_t batch, int32_t steps, int32_t channels, int32_t height, int32_t width) {
  return batch > 0 && steps > 0 && channels > 0 && height > 0 && width_supported(width);
}

template <int W>
void launch(const float* out, const float* tar, const double* circ, double* part, int H, const Split& sp, int KC, hipStream_t s) {
  hipLaunchKernelGGL(zspec::zonal_power_partials_kernel<W>, dim3((unsigned)sp.segs, KC, 2), dim3(zspec::NT), 0, s, out, tar,
                     circ, part, H, sp.rows, sp.seg_rows, KC);
}

int32_t zonal_sums(const float* out, const float* target, const double* circ, double* sums, int32_t batch, int32_t steps,
                   int32_t channels, int32_t height, int32_t width, void* workspace, size_t workspace_bytes, void* stream,
                   bool accumulate) {
  DLWP_REQUIRE(out && target && circ && sums && workspace, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(batch > 0 && steps > 0 && channels > 0 && height > 0 && width > 0, DLWP_ERR_INVALID_ARGUMENT, "bad shape");
  DLWP_REQUIRE(width_supported(width), DLWP_ERR_UNSUPPORTED,
               "zonal spectrum: width %d is not supported (a power of two from 32 to 512)", width);
  DLWP_REQUIRE((long long)steps * channels <= 65535, DLWP_ERR_UNSUPPORTED, "zonal spectrum: steps * channels above 65535");
  DLWP_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0 && (reinterpret_cast<uintptr_t>(target) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
               DLWP_ERR_INVALID_ARGUMENT, "out / target must be 16-byte and the workspace 8-byte aligned");
  const size_t need = dlwp_zonal_power_workspace_bytes(batch, steps, channels, height, width);
  DLWP_REQUIRE(workspace_bytes >= need, DLWP_ERR_WORKSPACE, "zonal spectrum workspace: %zu bytes given, %zu needed",
               workspace_bytes, need);
  const Split sp = split_of(batch, steps, channels, height, width);
  const int KC = steps * channels, NB = width / 2 + 1;
  DLWP_REQUIRE(sp.segs <= 0x7fffffffLL, DLWP_ERR_UNSUPPORTED, "zonal spectrum: too many rows");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  double* part = reinterpret_cast<double*>(workspace);
  switch (width) {
    case 32: launch<32>(out, target, circ, part, height, sp, KC, s); break;
    case 64: launch<64>(out, target, circ, part, height, sp, KC, s); break;
    case 128: launch<128>(out, target, circ, part, height, sp, KC, s); break;
    case 256: launch<256>(out, target, circ, part, height, sp, KC, s); break;
    default: launch<512>(out, target, circ, part, height, sp, KC, s); break;
  }
  DLWP_HIP_CHECK(hipGetLastError());
  const int n = 2 * KC * NB;
  hipLaunchKernelGGL(zspec::zonal_power_combine_kernel, dim3((n + 255) / 256), dim3(256), 0, s, part, sums, n, (int)sp.segs, NB,
                     accumulate ? 1 : 0);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}
}  // namespace

extern "C" size_t dlwp_zonal_power_workspace_bytes(int32_t batch, int32_t steps, int32_t channels, int32_t height, int32_t width) {
  if (!shape_ok(batch, steps, channels, height, width)) return 0;
  const Split sp = split_of(batch, steps, channels, height, width);
  return sizeof(double) * 2 * (size_t)steps * channels * (size_t)sp.segs * (width / 2 + 1);
}

extern "C" int32_t dlwp_zonal_power_sums_f32(const float* out_dev, const float* target_dev, const double* circumference_dev,
                                             double* sums_dev, int32_t batch, int32_t steps, int32_t channels, int32_t height,
                                             int32_t width, void* workspace_dev, size_t workspace_bytes, void* stream) {
  return zonal_sums(out_dev, target_dev, circumference_dev, sums_dev, batch, steps, channels, height, width, workspace_dev,
                    workspace_bytes, stream, false);
}

// the same sums ADDED to what sums_dev holds (the running sums of an evaluation over many batches)
extern "C" int32_t dlwp_zonal_power_sums_acc_f32(const float* out_dev, const float* target_dev, const double* circumference_dev,
                                                 double* sums_dev, int32_t batch, int32_t steps, int32_t channels,
                                                 int32_t height, int32_t width, void* workspace_dev, size_t workspace_bytes,
                                                 void* stream) {
  return zonal_sums(out_dev, target_dev, circumference_dev, sums_dev, batch, steps, channels, height, width, workspace_dev,
                    workspace_bytes, stream, true);
}
