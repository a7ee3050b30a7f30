// The PDE-Refiner noise scheduler on the device (reference models/diffusion_models/modern_unet/modern_unet.py:184,201 and
// scripts/train.py:228-255): the start noise of a forecast step, the DDPM ancestral step with its variance noise, and the
// training pair (residual, add_noise, v-target).  Each is ONE elementwise pass; the noise is a counter-based stream
// (philox_normal.hpp) evaluated where it is consumed, so nothing is drawn on the host or uploaded.
//
// Work split (the conventions of optim.hip): 256 threads per workgroup, one thread per block of 4 consecutive elements -- the
// 4 normals of one Philox block -- so a workgroup covers SPAN = 1024 elements per sweep; the grid is capped at MAX_BLOCKS
// and strided above the cap.  A block of 4 is loaded and stored as one 16-byte vector where every pointer of the call is
// 16-byte aligned (and, for the pair, where the 4 elements are contiguous in the inputs), element by element for an
// unaligned view and for the ragged tail.  One writer per element, no atomics, nothing read back on the host, no
// allocation and no synchronisation in a launch function.
//
// The kernels are VALU-bound by construction (ten Philox rounds plus log, sqrt and sincos per two normals) on tensors of a
// few hundred thousand elements: the gain is in launches, host RNG and uploads removed, not in bandwidth.
#include "philox_normal.hpp"

namespace dlwp {
namespace refiner {

constexpr int THREADS = 256;
constexpr int SPAN = 4 * THREADS;      // elements of a workgroup per sweep
constexpr int MAX_BLOCKS = 1024;       // four workgroups per compute unit

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static unsigned grid_for(long long n) {
  const long long b = (n + SPAN - 1) / SPAN;
  return (unsigned)(b < MAX_BLOCKS ? b : MAX_BLOCKS);
}

__device__ __forceinline__ f32x4 load4(const float* p, long long i, int live, bool vec) {
  if (vec && live == 4) return *reinterpret_cast<const f32x4*>(p + i);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < live; ++k) v[k] = p[i + k];
  return v;
}

__device__ __forceinline__ void store4(float* p, long long i, int live, bool vec, f32x4 v) {
  if (vec && live == 4) {
    *reinterpret_cast<f32x4*>(p + i) = v;
  } else {
    for (int k = 0; k < live; ++k) p[i + k] = v[k];
  }
}

// ---- (a) out[e] = normal(seed, offset + e) ------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void philox_normal_kernel(float* __restrict__ out, long long n, uint64_t seed,
                                                                uint64_t q0) {
  const bool vec = aligned16(out);
  const long long nblk = (n + 3) >> 2;
  for (long long b = (long long)blockIdx.x * THREADS + threadIdx.x; b < nblk; b += (long long)gridDim.x * THREADS) {
    const long long i = 4 * b;
    const int live = n - i < 4 ? (int)(n - i) : 4;
    store4(out, i, live, vec, philox::normal4(seed, q0 + (uint64_t)b));
  }
}

// ---- (b) the ancestral step (modern_unet.py:201, DDPMScheduler.step with v-prediction, "fixed_small" variance) -----------
//   prev = c0 (sa sample - sb model_output) + c1 sample + sigma z  =  A sample + B model_output + sigma z
// NOISE 0: sigma = 0 (t = 0), nothing is drawn or read; 1: z read from `noise`; 2: z drawn at the element's own index.
// Every element is read before it is written by the one thread that owns it: out may alias sample.
template <int NOISE>
__global__ __launch_bounds__(THREADS) void ddpm_step_kernel(const float* sample, const float* __restrict__ model_output,
                                                            const float* __restrict__ noise, float* out, long long n, float A,
                                                            float B, float sigma, uint64_t seed, uint64_t q0) {
  const bool vec = aligned16(sample) && aligned16(model_output) && aligned16(out) && (NOISE != 1 || aligned16(noise));
  const long long nblk = (n + 3) >> 2;
  for (long long b = (long long)blockIdx.x * THREADS + threadIdx.x; b < nblk; b += (long long)gridDim.x * THREADS) {
    const long long i = 4 * b;
    const int live = n - i < 4 ? (int)(n - i) : 4;
    const f32x4 s = load4(sample, i, live, vec), v = load4(model_output, i, live, vec);
    f32x4 r = A * s + B * v;
    if (NOISE == 1) r = r + sigma * load4(noise, i, live, vec);
    if (NOISE == 2) r = r + sigma * philox::normal4(seed, q0 + (uint64_t)b);
    store4(out, i, live, vec, r);
  }
}

// ---- (a', b') the member-major forms: [members][npm] flat, n = members * npm ------------------------------------------------
// Element (m, e) takes normal(seed, first_member + m, offset + e) (philox_normal.hpp).  The threads still own blocks of 4
// consecutive FLAT elements, so the accesses are the ones of (a) and (b); only the noise knows about members.  The step with
// sigma = 0 or with explicit noise has nothing to know: the launch function sends it to ddpm_step_kernel<0 / 1> over n.
__global__ __launch_bounds__(THREADS) void philox_normal_members_kernel(float* __restrict__ out, long long n, long long npm,
                                                                        uint32_t first_member, uint64_t seed, uint64_t q0) {
  const bool vec = aligned16(out);
  const long long nblk = (n + 3) >> 2;
  for (long long b = (long long)blockIdx.x * THREADS + threadIdx.x; b < nblk; b += (long long)gridDim.x * THREADS) {
    const long long i = 4 * b;
    const int live = n - i < 4 ? (int)(n - i) : 4;
    store4(out, i, live, vec, philox::member_normal4(seed, first_member, npm, q0, i, live));
  }
}

__global__ __launch_bounds__(THREADS) void ddpm_step_members_kernel(const float* sample, const float* __restrict__ model_output,
                                                                    float* out, long long n, long long npm,
                                                                    uint32_t first_member, float A, float B, float sigma,
                                                                    uint64_t seed, uint64_t q0) {
  const bool vec = aligned16(sample) && aligned16(model_output) && aligned16(out);
  const long long nblk = (n + 3) >> 2;
  for (long long b = (long long)blockIdx.x * THREADS + threadIdx.x; b < nblk; b += (long long)gridDim.x * THREADS) {
    const long long i = 4 * b;
    const int live = n - i < 4 ? (int)(n - i) : 4;
    const f32x4 s = load4(sample, i, live, vec), v = load4(model_output, i, live, vec);
    const f32x4 r = A * s + B * v + sigma * philox::member_normal4(seed, first_member, npm, q0, i, live);
    store4(out, i, live, vec, r);
  }
}

// ---- (c) the training pair (train.py:228-255) -------------------------------------------------------------------------
//   res = target - prog_last;  y_noised = sa res + sb eps;  v_target = sa eps - sb res
// Outputs are [(batch faces), 1, channels, plane] contiguous; output element o = ((b faces + f) channels + c) plane + p reads
// input element b batch_stride + (c faces + f) plane + p: the "b t c f h w -> (b f) t c h w" of train.py:232-233 by index
// arithmetic (faces = 1: lat-lon, the identity).  eps is indexed by o.
struct PairDims {
  long long n, plane, per_face, t_bs, p_bs;      // per_face = channels * plane
  int faces;
};

__device__ __forceinline__ void pair_index(const PairDims& d, long long o, long long& it, long long& ip) {
  const long long bf = o / d.per_face, rem = o - bf * d.per_face;
  const long long b = bf / d.faces, f = bf - b * d.faces;
  const long long c = rem / d.plane, p = rem - c * d.plane;
  const long long inner = (c * d.faces + f) * d.plane + p;
  it = b * d.t_bs + inner;
  ip = b * d.p_bs + inner;
}

template <int NOISE>      // 1: eps read from `noise`, 2: drawn at the output index
__global__ __launch_bounds__(THREADS) void refiner_pair_kernel(const float* __restrict__ target, const float* __restrict__ prog,
                                                               const float* __restrict__ noise, float* __restrict__ y_noised,
                                                               float* __restrict__ v_target, PairDims d, float sa, float sb,
                                                               uint64_t seed, uint64_t q0) {
  // a block of 4 outputs is 4 consecutive, 16-byte aligned inputs when it cannot straddle a plane and every base and batch
  // stride keeps the alignment
  const bool vec = (d.plane & 3) == 0 && (d.t_bs & 3) == 0 && (d.p_bs & 3) == 0 && aligned16(target) && aligned16(prog) &&
                   aligned16(y_noised) && aligned16(v_target) && (NOISE != 1 || aligned16(noise));
  const long long nblk = (d.n + 3) >> 2;
  for (long long b = (long long)blockIdx.x * THREADS + threadIdx.x; b < nblk; b += (long long)gridDim.x * THREADS) {
    const long long o = 4 * b;
    const int live = d.n - o < 4 ? (int)(d.n - o) : 4;
    f32x4 t = {0.f, 0.f, 0.f, 0.f}, g = t;
    long long it, ip;
    if (vec && live == 4) {
      pair_index(d, o, it, ip);
      t = *reinterpret_cast<const f32x4*>(target + it);
      g = *reinterpret_cast<const f32x4*>(prog + ip);
    } else {
      for (int k = 0; k < live; ++k) {
        pair_index(d, o + k, it, ip);
        t[k] = target[it];
        g[k] = prog[ip];
      }
    }
    const f32x4 eps = NOISE == 1 ? load4(noise, o, live, vec) : philox::normal4(seed, q0 + (uint64_t)b);
    const f32x4 res = t - g;
    store4(y_noised, o, live, vec, sa * res + sb * eps);
    store4(v_target, o, live, vec, sa * eps - sb * res);
  }
}

}  // namespace refiner
}  // namespace dlwp

using namespace dlwp;

extern "C" int64_t dlwp_refiner_grid_span(void) { return (int64_t)refiner::MAX_BLOCKS * refiner::SPAN; }

extern "C" int32_t dlwp_philox_normal_f32(float* out, int64_t n, int64_t seed, int64_t offset, void* stream) {
  DLWP_REQUIRE(out, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(n > 0, DLWP_ERR_INVALID_ARGUMENT, "bad size");
  DLWP_REQUIRE(offset >= 0 && (offset & 3) == 0, DLWP_ERR_INVALID_ARGUMENT, "the offset must be a non-negative multiple of 4");
  hipLaunchKernelGGL(refiner::philox_normal_kernel, dim3(refiner::grid_for(n)), dim3(refiner::THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), out, (long long)n, (uint64_t)seed, (uint64_t)offset >> 2);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" int32_t dlwp_ddpm_step_f32(const float* sample, const float* model_output, const float* noise_or_null, float* out,
                                      int64_t n, const double coef[4], int64_t seed, int64_t offset, void* stream) {
  DLWP_REQUIRE(sample && model_output && out && coef, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(n > 0, DLWP_ERR_INVALID_ARGUMENT, "bad size");
  DLWP_REQUIRE(offset >= 0 && (offset & 3) == 0, DLWP_ERR_INVALID_ARGUMENT, "the offset must be a non-negative multiple of 4");
  // coef = { c0 sa, c0 sb, c1, sigma } in double; folded here, rounded once to fp32
  const float A = (float)(coef[0] + coef[2]), B = (float)(-coef[1]), sigma = (float)coef[3];
  const dim3 grid(refiner::grid_for(n)), block(refiner::THREADS);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint64_t q0 = (uint64_t)offset >> 2;
  if (coef[3] == 0.0)
    hipLaunchKernelGGL(refiner::ddpm_step_kernel<0>, grid, block, 0, s, sample, model_output, noise_or_null, out, (long long)n, A, B,
                       sigma, (uint64_t)seed, q0);
  else if (noise_or_null)
    hipLaunchKernelGGL(refiner::ddpm_step_kernel<1>, grid, block, 0, s, sample, model_output, noise_or_null, out, (long long)n, A, B,
                       sigma, (uint64_t)seed, q0);
  else
    hipLaunchKernelGGL(refiner::ddpm_step_kernel<2>, grid, block, 0, s, sample, model_output, noise_or_null, out, (long long)n, A, B,
                       sigma, (uint64_t)seed, q0);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

// what the two member-major entry points share: the shape and the member range (a member is a uint32 counter word; the C ABI
// carries first_member and the count as int32, so the last member is 2^31 - 1)
static int32_t check_members(int64_t n_per_member, int32_t members, int32_t first_member, int64_t offset) {
  DLWP_REQUIRE(n_per_member > 0 && members > 0, DLWP_ERR_INVALID_ARGUMENT, "bad size");
  DLWP_REQUIRE(first_member >= 0 && (int64_t)first_member + members <= (int64_t)1 << 31, DLWP_ERR_INVALID_ARGUMENT,
               "members [%d, %lld) outside [0, 2^31)", first_member, (long long)first_member + members);
  DLWP_REQUIRE(n_per_member <= INT64_MAX / 2 / members, DLWP_ERR_INVALID_ARGUMENT, "bad size");
  DLWP_REQUIRE(offset >= 0 && (offset & 3) == 0, DLWP_ERR_INVALID_ARGUMENT, "the offset must be a non-negative multiple of 4");
  return DLWP_OK;
}

extern "C" int32_t dlwp_philox_normal_members_f32(float* out, int64_t n_per_member, int32_t members, int32_t first_member,
                                                  int64_t seed, int64_t offset, void* stream) {
  DLWP_REQUIRE(out, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  if (const int32_t rc = check_members(n_per_member, members, first_member, offset)) return rc;
  const long long n = (long long)n_per_member * members;
  hipLaunchKernelGGL(refiner::philox_normal_members_kernel, dim3(refiner::grid_for(n)), dim3(refiner::THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), out, n, (long long)n_per_member, (uint32_t)first_member, (uint64_t)seed,
                     (uint64_t)offset >> 2);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" int32_t dlwp_ddpm_step_members_f32(const float* sample, const float* model_output, const float* noise_or_null,
                                              float* out, int64_t n_per_member, int32_t members, int32_t first_member,
                                              const double coef[4], int64_t seed, int64_t offset, void* stream) {
  DLWP_REQUIRE(sample && model_output && out && coef, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  if (const int32_t rc = check_members(n_per_member, members, first_member, offset)) return rc;
  const long long n = (long long)n_per_member * members;
  const float A = (float)(coef[0] + coef[2]), B = (float)(-coef[1]), sigma = (float)coef[3];      // as dlwp_ddpm_step_f32
  const dim3 grid(refiner::grid_for(n)), block(refiner::THREADS);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint64_t q0 = (uint64_t)offset >> 2;
  if (coef[3] == 0.0)
    hipLaunchKernelGGL(refiner::ddpm_step_kernel<0>, grid, block, 0, s, sample, model_output, noise_or_null, out, n, A, B, sigma,
                       (uint64_t)seed, q0);
  else if (noise_or_null)
    hipLaunchKernelGGL(refiner::ddpm_step_kernel<1>, grid, block, 0, s, sample, model_output, noise_or_null, out, n, A, B, sigma,
                       (uint64_t)seed, q0);
  else
    hipLaunchKernelGGL(refiner::ddpm_step_members_kernel, grid, block, 0, s, sample, model_output, out, n, (long long)n_per_member,
                       (uint32_t)first_member, A, B, sigma, (uint64_t)seed, q0);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" int32_t dlwp_refiner_pair_f32(const float* target, const float* prog_last, const float* noise_or_null, float* y_noised,
                                         float* v_target, int32_t batch, int32_t faces, int32_t channels, int64_t plane,
                                         int64_t target_batch_stride, int64_t prog_batch_stride, float sqrt_abar,
                                         float sqrt_1m_abar, int64_t seed, int64_t offset, void* stream) {
  DLWP_REQUIRE(target && prog_last && y_noised && v_target, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(batch > 0 && faces > 0 && channels > 0 && plane > 0, DLWP_ERR_INVALID_ARGUMENT, "bad shape");
  DLWP_REQUIRE(plane <= INT64_MAX / channels / faces / batch, DLWP_ERR_INVALID_ARGUMENT, "bad shape");
  const long long row = (long long)channels * faces * plane;      // elements of one batch entry of the inputs
  DLWP_REQUIRE(target_batch_stride >= row && prog_batch_stride >= row, DLWP_ERR_INVALID_ARGUMENT,
               "a batch stride is smaller than one batch entry");
  DLWP_REQUIRE(offset >= 0 && (offset & 3) == 0, DLWP_ERR_INVALID_ARGUMENT, "the offset must be a non-negative multiple of 4");
  refiner::PairDims d;
  d.n = row * batch;
  d.faces = faces;
  // lat-lon: channel and plane are one contiguous run, so a block of 4 may cross a channel boundary
  d.plane = faces == 1 ? (long long)channels * plane : (long long)plane;
  d.per_face = (long long)channels * plane;
  d.t_bs = target_batch_stride;
  d.p_bs = prog_batch_stride;
  const dim3 grid(refiner::grid_for(d.n)), block(refiner::THREADS);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint64_t q0 = (uint64_t)offset >> 2;
  if (noise_or_null)
    hipLaunchKernelGGL(refiner::refiner_pair_kernel<1>, grid, block, 0, s, target, prog_last, noise_or_null, y_noised, v_target, d,
                       sqrt_abar, sqrt_1m_abar, (uint64_t)seed, q0);
  else
    hipLaunchKernelGGL(refiner::refiner_pair_kernel<2>, grid, block, 0, s, target, prog_last, noise_or_null, y_noised, v_target, d,
                       sqrt_abar, sqrt_1m_abar, (uint64_t)seed, q0);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}
