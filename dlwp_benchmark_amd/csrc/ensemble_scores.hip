// Ensemble scores of the diffusion backbones' forecasts, reduced on the device.  The reference holds only a commented sketch
// of an ensemble evaluation (scripts/train.py:352-371: the ensemble mean and a standard deviation per lead day); the scores
// here are the usual ensemble-verification forms (Fortin et al. 2014 for the spread / skill pair, Ferro et al. 2008 for the
// fair CRPS, Hamill 2001 for the rank histogram) and are pinned by the float64 restatement tests/ensemble_ref.py.
//
// ens is M planes [B, K, C, H, W], member_stride elements apart; target is [B, K, C, H, W].  With x_(0) <= ... <= x_(M-1) the
// members at a grid point, y the target, w the latitude weight of the row, s the variable's scale (1 when null):
//   sums[0][k][c] += sum_{b,h,w} w (s (mean_m x_m - y))^2                        ensemble-mean squared error
//   sums[1][k][c] += sum w s^2 1/(M-1) sum_m (x_m - mean)^2                     ensemble variance (two-pass, about the mean)
//   sums[2][k][c] += sum w s 1/M sum_m |x_m - y|                                first CRPS term
//   sums[3][k][c] += sum w s sum_{i<j} |x_i - x_j| = sum w s sum_i (2i - M + 1) x_(i)      second CRPS term, unnormalised
//   ranks[k][c][r] += 1 with r = #{m : x_m < y}, strict and unweighted          rank histogram
// for the steps k = step_begin .. step_begin + K - 1 of sums [4][steps_total][C] and ranks [steps_total][C][M + 1].  NaNs are
// not treated: a NaN member or target poisons the sums of its (k, c) and lands in an unspecified rank bin.
//
// Decomposition: one thread per grid point, one workgroup per slice of PTS points of one (b, k, c) plane; the M loads of a
// point are M coalesced rows across the wave, each member value is read from HBM once and nothing but the partials is
// written.  A thread keeps the members in registers (MP = M padded to the next power of two, six instantiations), takes
// rank, mean and |x - y| from them, replaces them by the deviations d_m = x_m - mean (padding: +inf), takes the variance,
// sorts the deviations with a bitonic network of MP (log2 MP)(log2 MP + 1) / 4 compare-exchanges (v_min + v_max each) and
// takes sum_i (2i - M + 1) d_(i), which equals the sum over x_(i) because the coefficients add up to zero -- without the
// cancellation a field with a large mean (temperature in K) would bring.  All of that is fp32.  Across points everything is
// fp64 and in a fixed order: thread (its points in order), wave (xor tree), workgroup (waves in order), then a second kernel
// adds the workgroups' partials of a (k, c) in workgroup order onto the running sums.  No floating-point atomics: two runs
// give the same bits.  The rank counts are integers: an LDS histogram per workgroup, then one atomicAdd per bin.
#include "common.hpp"

namespace dlwp {
namespace ens {

constexpr int NT = 256;
constexpr int PTS = 1024;      // points of a workgroup: four per thread

template <int N>
__device__ __forceinline__ void bitonic_sort(float (&v)[N]) {
#pragma unroll
  for (int k = 2; k <= N; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const int l = i ^ j;
        if (l > i) {
          const float lo = fminf(v[i], v[l]), hi = fmaxf(v[i], v[l]);
          const bool up = (i & k) == 0;
          v[i] = up ? lo : hi;
          v[l] = up ? hi : lo;
        }
      }
    }
  }
}

// sum of term(0) .. term(N - 1) on four interleaved chains: at most N / 4 + 1 roundings on any path.  The terms are formed
// where they are added, so no second array of N registers lives beside the members.
template <int N, class Term>
__device__ __forceinline__ float sum4(Term term) {
  if constexpr (N < 4) {
    return term(0) + term(1);
  } else {
    float a0 = term(0), a1 = term(1), a2 = term(2), a3 = term(3);
#pragma unroll
    for (int i = 4; i < N; i += 4) {
      a0 += term(i);
      a1 += term(i + 1);
      a2 += term(i + 2);
      a3 += term(i + 3);
    }
    return (a0 + a1) + (a2 + a3);
  }
}

template <int MP>
__global__ __launch_bounds__(NT) void ensemble_partials_kernel(const float* __restrict__ ens, const float* __restrict__ tar,
                                                               const float* __restrict__ latw,    // [H]
                                                               const float* __restrict__ scale,   // [C] or null
                                                               double* __restrict__ part,         // [4][K C][B chunks]
                                                               unsigned long long* __restrict__ ranks,   // [steps_total][C][M + 1]
                                                               int M, long long member_stride, int K, int C, int H, int W,
                                                               int step_begin) {
  // grid: (chunks, K C, B)
  __shared__ int hist[65];
  __shared__ double red[4][NT / 64];
  const int tid = threadIdx.x;
  const int kc = blockIdx.y, b = blockIdx.z;
  const int k = kc / C, c = kc - k * C;
  const long long HW = (long long)H * W;
  const long long plane = ((long long)b * K * C + kc) * HW;
  const long long lo = (long long)blockIdx.x * PTS, hi = lo + PTS < HW ? lo + PTS : HW;
  const float s = scale ? scale[c] : 1.f;
  const float inv_m = 1.f / (float)M, inv_m1 = 1.f / (float)(M - 1);
  const float inf = __builtin_inff();
  if (tid < 65) hist[tid] = 0;
  __syncthreads();
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (long long i = lo + tid; i < hi; i += NT) {
    const float* __restrict__ p = ens + plane + i;
    float v[MP];
#pragma unroll
    for (int m = 0; m < MP; ++m) v[m] = m < M ? p[(long long)m * member_stride] : 0.f;
    const float y = tar[plane + i];
    const float w = latw[i / W];
    int rank = 0;
#pragma unroll
    for (int m = 0; m < MP; ++m) rank += (m < M && v[m] < y) ? 1 : 0;
    const float mean = sum4<MP>([&](int m) { return v[m]; }) * inv_m;      // the padding is 0 here
    const float abs_err = sum4<MP>([&](int m) { return m < M ? fabsf(v[m] - y) : 0.f; }) * inv_m;
#pragma unroll
    for (int m = 0; m < MP; ++m) v[m] = m < M ? v[m] - mean : inf;
    const float var = sum4<MP>([&](int m) { return m < M ? v[m] * v[m] : 0.f; }) * inv_m1;
    bitonic_sort<MP>(v);
    // sum_i (2i - M + 1) d_(i): the padding sits at i >= M and is skipped
    const float pairs = sum4<MP>([&](int m) { return m < M ? (float)(2 * m - M + 1) * v[m] : 0.f; });
    const float e = s * (mean - y);
    acc[0] += (double)(w * (e * e));
    acc[1] += (double)(w * ((s * s) * var));
    acc[2] += (double)(w * (s * abs_err));
    acc[3] += (double)(w * (s * pairs));
    atomicAdd(&hist[rank], 1);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc[q] += __shfl_xor(acc[q], o, 64);
    if ((tid & 63) == 0) red[q][tid >> 6] = acc[q];
  }
  __syncthreads();
  const int blocks_per_kc = gridDim.z * gridDim.x;
  if (tid < 4) {
    const double tot = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
    part[((long long)tid * gridDim.y + kc) * blocks_per_kc + (long long)b * gridDim.x + blockIdx.x] = tot;
  }
  if (tid <= M && hist[tid])
    atomicAdd(&ranks[((long long)(step_begin + k) * C + c) * (M + 1) + tid], (unsigned long long)hist[tid]);
}

// sums[q][step_begin + k][c] += the S partials of (q, k, c), in workgroup order
__global__ __launch_bounds__(256) void ensemble_combine_kernel(const double* __restrict__ part, double* __restrict__ sums, int KC,
                                                               int C, int S, int steps_total, int step_begin) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * KC) return;
  const int q = i / KC, kc = i - q * KC;
  const double* src = part + (long long)i * S;
  double tot = 0.0;
  for (int j = 0; j < S; ++j) tot += src[j];
  sums[((long long)q * steps_total + step_begin) * C + kc] += tot;
}

}  // namespace ens
}  // namespace dlwp

using namespace dlwp;

namespace {
long long chunks_of(int32_t height, int32_t width) { return ((long long)height * width + ens::PTS - 1) / ens::PTS; }

template <int MP>
void launch(const float* e, const float* t, const float* latw, const float* scale, double* part, unsigned long long* ranks, int M,
            long long member_stride, int B, int K, int C, int H, int W, int step_begin, hipStream_t s) {
  hipLaunchKernelGGL(ens::ensemble_partials_kernel<MP>, dim3((unsigned)chunks_of(H, W), K * C, B), dim3(ens::NT), 0, s, e, t, latw,
                     scale, part, ranks, M, member_stride, K, C, H, W, step_begin);
}
}  // namespace

extern "C" size_t dlwp_ensemble_sums_workspace_bytes(int32_t batch, int32_t steps, int32_t channels, int32_t height,
                                                     int32_t width) {
  if (batch <= 0 || steps <= 0 || channels <= 0 || height <= 0 || width <= 0) return 0;
  return sizeof(double) * 4 * (size_t)steps * channels * (size_t)batch * (size_t)chunks_of(height, width);
}

extern "C" int32_t dlwp_ensemble_sums_acc_f32(const float* ens_dev, const float* target_dev, const float* lat_weights_dev,
                                              const float* scale_or_null_dev, double* sums_dev, int64_t* ranks_dev,
                                              int32_t members, int64_t member_stride, int32_t batch, int32_t steps,
                                              int32_t channels, int32_t height, int32_t width, int32_t steps_total,
                                              int32_t step_begin, void* workspace_dev, size_t workspace_bytes, void* stream) {
  DLWP_REQUIRE(ens_dev && target_dev && lat_weights_dev && sums_dev && ranks_dev && workspace_dev, DLWP_ERR_INVALID_ARGUMENT,
               "null argument");
  DLWP_REQUIRE(batch > 0 && steps > 0 && channels > 0 && height > 0 && width > 0, DLWP_ERR_INVALID_ARGUMENT, "bad shape");
  DLWP_REQUIRE(members >= 2 && members <= 64, DLWP_ERR_UNSUPPORTED, "ensemble scores: %d members (2 to 64 are supported)",
               members);
  DLWP_REQUIRE(step_begin >= 0 && steps_total > 0 && (long long)step_begin + steps <= steps_total, DLWP_ERR_INVALID_ARGUMENT,
               "steps [%d, %lld) outside the %d steps of the sums", step_begin, (long long)step_begin + steps, steps_total);
  DLWP_REQUIRE((long long)steps * channels <= 65535 && batch <= 65535, DLWP_ERR_UNSUPPORTED, "grid too large");
  const long long hw = (long long)height * width;
  DLWP_REQUIRE(hw <= INT64_MAX / 64 / channels / steps / batch, DLWP_ERR_INVALID_ARGUMENT, "bad shape");
  const long long plane = hw * channels * steps * batch;
  DLWP_REQUIRE(member_stride >= plane && member_stride <= INT64_MAX / 64, DLWP_ERR_INVALID_ARGUMENT,
               "the member stride is smaller than one member [batch, steps, channels, height, width]");
  const long long chunks = chunks_of(height, width);
  DLWP_REQUIRE(chunks <= 0x7fffffffLL && chunks * batch <= 0x7fffffffLL, DLWP_ERR_UNSUPPORTED, "ensemble scores: plane too large");
  DLWP_REQUIRE((reinterpret_cast<uintptr_t>(workspace_dev) & 7) == 0, DLWP_ERR_INVALID_ARGUMENT,
               "the workspace must be 8-byte aligned");
  const size_t need = dlwp_ensemble_sums_workspace_bytes(batch, steps, channels, height, width);
  DLWP_REQUIRE(workspace_bytes >= need, DLWP_ERR_WORKSPACE, "ensemble scores workspace: %zu bytes given, %zu needed",
               workspace_bytes, need);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  double* part = reinterpret_cast<double*>(workspace_dev);
  unsigned long long* ranks = reinterpret_cast<unsigned long long*>(ranks_dev);
#define DLWP_ENS_LAUNCH(MP)                                                                                                  \
  launch<MP>(ens_dev, target_dev, lat_weights_dev, scale_or_null_dev, part, ranks, members, member_stride, batch, steps, channels, \
             height, width, step_begin, s)
  if (members <= 2) DLWP_ENS_LAUNCH(2);
  else if (members <= 4) DLWP_ENS_LAUNCH(4);
  else if (members <= 8) DLWP_ENS_LAUNCH(8);
  else if (members <= 16) DLWP_ENS_LAUNCH(16);
  else if (members <= 32) DLWP_ENS_LAUNCH(32);
  else DLWP_ENS_LAUNCH(64);
#undef DLWP_ENS_LAUNCH
  DLWP_HIP_CHECK(hipGetLastError());
  const int KC = steps * channels;
  hipLaunchKernelGGL(ens::ensemble_combine_kernel, dim3((4 * KC + 255) / 256), dim3(256), 0, s, part, sums_dev, KC, channels,
                     (int)(chunks * batch), steps_total, step_begin);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}
