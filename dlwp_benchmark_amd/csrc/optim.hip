// The tail of a training step (reference scripts/train.py:186-312): the loss (scripts/losses.py:155-188 CustomMSELoss), the
// gradient-norm clip (train.py:299-305, torch/nn/utils/clip_grad.py:165-169), AdamW (train.py:59,309, torch 2.10's
// torch/optim/adam.py:347-547), EMA (train.py:312) and zero_grad (train.py:186).  Each is pure HBM streaming; each is ONE
// pass here.
//
// Multi-tensor addressing.  A model has hundreds of parameter tensors; one launch covers all of them through a device table
// in struct-of-arrays form (built once by optim.py, passed as plain pointers):
//   per tensor  p_ptrs[t], g_ptrs[t] (addresses as int64; g 0 = no gradient this step), numel[t], state_off[t] (element
//               offset into the optimizer's flat exp_avg / exp_avg_sq / shadow arenas, a multiple of 4), group[t], step[t],
//               derived[t][8] (the per-tensor floats of this step, see adamw_header_kernel)
//   per group   hyper[g][5] doubles: lr, beta1, beta2, eps, weight_decay
//   per chunk   chunk_tensor[c], chunk_first[c]: CHUNK consecutive elements of one tensor (fewer at its end)
// A workgroup takes whole chunks, chunk blockIdx.x first and then every gridDim.x-th: the grid is capped at MAX_BLOCKS (2048,
// eight workgroups per compute unit) and strided above it.  Inside a chunk: 16-byte loads and stores where every pointer of
// the tensor that the kernel touches is 16-byte aligned (a chunk starts a multiple of CHUNK elements into its tensor and the
// arenas are aligned, so the tensor's alignment is the chunk's), scalar ones for a tensor that is not (a view at an odd
// element offset) and for the ragged tail of every tensor.
//
// Determinism.  One writer per element, no float atomics.  The two reductions (sum of squared gradients, loss) leave one
// partial per chunk / per workgroup -- each thread adds its elements in ascending order, the 256 threads meet in a fixed
// LDS tree -- and a single-workgroup finish adds the partials in double in a fixed order (thread i takes partials i, i + 256,
// ...; then the same tree).  The partial of a chunk does not depend on the grid.  A rerun is bitwise identical.
//
// Nothing here reads a device value on the host: the clip coefficient, the step counts and the step-dependent AdamW factors
// live in device memory, so a recorded (hipGraph) step replays correctly.
#include "common.hpp"

namespace dlwp {
namespace optim {

constexpr int CHUNK = 4096;              // elements of a chunk: 256 threads x 4 vectors of 4
constexpr int THREADS = 256;
constexpr int MAX_BLOCKS = 2048;         // the grid cap of every multi-tensor kernel and of the loss
constexpr int LOSS_SWEEP = 4096;         // elements a loss workgroup takes per sweep
constexpr int DERIVED = 8;               // floats per tensor in derived[]
constexpr int HYPER = 5;                 // doubles per group in hyper[]

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the fixed-order sum of one value per thread; the result is valid in thread 0.  Ends with a barrier: s is free again.
template <class T>
__device__ __forceinline__ T block_sum(T v, T* s) {
  const int tid = threadIdx.x;
  s[tid] = v;
  __syncthreads();
#pragma unroll
  for (int o = THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) s[tid] += s[tid + o];
    __syncthreads();
  }
  const T r = s[0];
  __syncthreads();
  return r;
}

// elements of chunk c of its tensor
__device__ __forceinline__ int chunk_len(const int64_t* numel, int t, long long first) {
  const long long rem = numel[t] - first;
  return rem < CHUNK ? (int)rem : CHUNK;
}

// ---- gradient norm and clip (torch/nn/utils/clip_grad.py, norm_type 2) -------------------------------------------------
__global__ __launch_bounds__(THREADS) void mt_sumsq_kernel(const int64_t* __restrict__ g_ptrs, const int64_t* __restrict__ numel,
                                                           const int32_t* __restrict__ chunk_tensor,
                                                           const int64_t* __restrict__ chunk_first, int n_chunks,
                                                           float* __restrict__ partials) {
  __shared__ float s[THREADS];
  const int tid = threadIdx.x;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int t = chunk_tensor[c];
    const long long first = chunk_first[c];
    const float* g = reinterpret_cast<const float*>(g_ptrs[t]);
    float acc = 0.f;
    if (g) {
      const int n = chunk_len(numel, t, first);
      g += first;
      const int nvec = aligned16(g) ? n >> 2 : 0;
      for (int i = tid; i < nvec; i += THREADS) {
        const f32x4 v = reinterpret_cast<const f32x4*>(g)[i];
        acc += v[0] * v[0];
        acc += v[1] * v[1];
        acc += v[2] * v[2];
        acc += v[3] * v[3];
      }
      for (int i = 4 * nvec + tid; i < n; i += THREADS) acc += g[i] * g[i];
    }
    const float sum = block_sum(acc, s);
    if (tid == 0) partials[c] = sum;
  }
}

// total_norm = sqrt(sum of the partials), clip_coef = min(1, max_norm / (total_norm + 1e-6)) in fp32 as torch computes them;
// a NaN coefficient stays NaN (torch.clamp keeps it).  One workgroup.
__global__ __launch_bounds__(THREADS) void mt_norm_finish_kernel(const float* __restrict__ partials, int n_chunks, float max_norm,
                                                                 float* __restrict__ scal) {
  __shared__ double s[THREADS];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_chunks; i += THREADS) acc += (double)partials[i];
  const double sum = block_sum(acc, s);
  if (threadIdx.x == 0) {
    const float total = (float)sqrt(sum);
    float coef = max_norm / (total + 1e-6f);
    coef = coef > 1.0f ? 1.0f : coef;
    scal[0] = total;
    scal[1] = coef;
  }
}

__global__ __launch_bounds__(THREADS) void mt_scale_kernel(const int64_t* __restrict__ g_ptrs, const int64_t* __restrict__ numel,
                                                           const int32_t* __restrict__ chunk_tensor,
                                                           const int64_t* __restrict__ chunk_first, int n_chunks,
                                                           const float* __restrict__ scal) {
  const int tid = threadIdx.x;
  const float coef = scal[1];
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int t = chunk_tensor[c];
    const long long first = chunk_first[c];
    float* g = reinterpret_cast<float*>(g_ptrs[t]);
    if (!g) continue;
    const int n = chunk_len(numel, t, first);
    g += first;
    const int nvec = aligned16(g) ? n >> 2 : 0;
    for (int i = tid; i < nvec; i += THREADS) {
      f32x4 v = reinterpret_cast<f32x4*>(g)[i];
      v *= coef;
      reinterpret_cast<f32x4*>(g)[i] = v;
    }
    for (int i = 4 * nvec + tid; i < n; i += THREADS) g[i] *= coef;
  }
}

__global__ __launch_bounds__(THREADS) void mt_zero_kernel(const int64_t* __restrict__ g_ptrs, const int64_t* __restrict__ numel,
                                                          const int32_t* __restrict__ chunk_tensor,
                                                          const int64_t* __restrict__ chunk_first, int n_chunks) {
  const int tid = threadIdx.x;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int t = chunk_tensor[c];
    const long long first = chunk_first[c];
    float* g = reinterpret_cast<float*>(g_ptrs[t]);
    if (!g) continue;
    const int n = chunk_len(numel, t, first);
    g += first;
    const int nvec = aligned16(g) ? n >> 2 : 0;
    for (int i = tid; i < nvec; i += THREADS) reinterpret_cast<f32x4*>(g)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int i = 4 * nvec + tid; i < n; i += THREADS) g[i] = 0.f;
  }
}

// ---- AdamW (torch 2.10 torch/optim/adam.py:347-547, _single_tensor_adam with decoupled weight decay) ----------------------
// One thread per tensor: the step of a tensor that has a gradient advances, and the factors that depend on it are derived in
// double (as torch derives them in Python floats) and left as floats for the main kernel:
//   derived[t] = { 1 - lr wd,  1 - beta1,  beta2,  1 - beta2,  -lr / bc1,  1 / sqrt(bc2),  eps,  - }
// with bc1 = 1 - beta1^step, bc2 = 1 - beta2^step.  A tensor without a gradient keeps its step and is skipped below.
__global__ void adamw_header_kernel(const int64_t* __restrict__ g_ptrs, const int32_t* __restrict__ group,
                                    const double* __restrict__ hyper, int32_t* __restrict__ step, float* __restrict__ derived,
                                    int n_tensors) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tensors || !g_ptrs[t]) return;
  const int s = step[t] + 1;
  step[t] = s;
  const double* h = hyper + HYPER * group[t];
  const double lr = h[0], b1 = h[1], b2 = h[2], eps = h[3], wd = h[4];
  const double bc1 = 1.0 - pow(b1, (double)s), bc2 = 1.0 - pow(b2, (double)s);
  float* d = derived + DERIVED * t;
  d[0] = (float)(1.0 - lr * wd);
  d[1] = (float)(1.0 - b1);
  d[2] = (float)b2;
  d[3] = (float)(1.0 - b2);
  d[4] = (float)(-(lr / bc1));
  d[5] = (float)(1.0 / sqrt(bc2));
  d[6] = (float)eps;
  d[7] = 0.f;
}

struct AdamwFactors {
  float decay, w1, beta2, w2, neg_step, inv_sqrt_bc2, eps, coef;
};

// p *= 1 - lr wd;  m = lerp(m, g, 1 - beta1);  v = beta2 v + (1 - beta2) g g;  p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
__device__ __forceinline__ void adamw_element(float& p, float g, float& m, float& v, const AdamwFactors& f, bool clip) {
  if (clip) g *= f.coef;                      // the product mt_scale_kernel would have stored
  p *= f.decay;
  m = m + f.w1 * (g - m);
  v = v * f.beta2 + (f.w2 * g) * g;
  const float denom = sqrtf(v) * f.inv_sqrt_bc2 + f.eps;
  p = p + (f.neg_step * m) / denom;
}

__global__ __launch_bounds__(THREADS) void mt_adamw_kernel(const int64_t* __restrict__ p_ptrs, const int64_t* __restrict__ g_ptrs,
                                                           const int64_t* __restrict__ numel,
                                                           const int64_t* __restrict__ state_off,
                                                           const float* __restrict__ derived,
                                                           const int32_t* __restrict__ chunk_tensor,
                                                           const int64_t* __restrict__ chunk_first, int n_chunks,
                                                           float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                                                           const float* __restrict__ scal) {
  const int tid = threadIdx.x;
  const bool clip = scal != nullptr;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int t = chunk_tensor[c];
    const long long first = chunk_first[c];
    const float* g = reinterpret_cast<const float*>(g_ptrs[t]);
    if (!g) continue;
    float* p = reinterpret_cast<float*>(p_ptrs[t]) + first;
    g += first;
    float* m = exp_avg + state_off[t] + first;
    float* v = exp_avg_sq + state_off[t] + first;
    const float* d = derived + DERIVED * t;
    const AdamwFactors f{d[0], d[1], d[2], d[3], d[4], d[5], d[6], clip ? scal[1] : 1.0f};
    const int n = chunk_len(numel, t, first);
    const int nvec = (aligned16(p) && aligned16(g)) ? n >> 2 : 0;      // m and v: aligned by construction of the arenas
    for (int i = tid; i < nvec; i += THREADS) {
      f32x4 pv = reinterpret_cast<f32x4*>(p)[i], mv = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i];
      const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float pk = pv[k], mk = mv[k], vk = vv[k];
        adamw_element(pk, gv[k], mk, vk, f, clip);
        pv[k] = pk;
        mv[k] = mk;
        vv[k] = vk;
      }
      reinterpret_cast<f32x4*>(p)[i] = pv;
      reinterpret_cast<f32x4*>(m)[i] = mv;
      reinterpret_cast<f32x4*>(v)[i] = vv;
    }
    for (int i = 4 * nvec + tid; i < n; i += THREADS) adamw_element(p[i], g[i], m[i], v[i], f, clip);
  }
}

// ---- EMA: shadow = decay shadow + (1 - decay) p (train.py:312) -----------------------------------------------------------
__global__ __launch_bounds__(THREADS) void mt_ema_kernel(const int64_t* __restrict__ p_ptrs, const int64_t* __restrict__ numel,
                                                         const int64_t* __restrict__ state_off,
                                                         const int32_t* __restrict__ chunk_tensor,
                                                         const int64_t* __restrict__ chunk_first, int n_chunks,
                                                         float* __restrict__ shadow, float decay, float one_minus) {
  const int tid = threadIdx.x;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int t = chunk_tensor[c];
    const long long first = chunk_first[c];
    const float* p = reinterpret_cast<const float*>(p_ptrs[t]);
    if (!p) continue;
    p += first;
    float* sh = shadow + state_off[t] + first;
    const int n = chunk_len(numel, t, first);
    const int nvec = aligned16(p) ? n >> 2 : 0;
    for (int i = tid; i < nvec; i += THREADS) {
      const f32x4 pv = reinterpret_cast<const f32x4*>(p)[i];
      f32x4 sv = reinterpret_cast<f32x4*>(sh)[i];
      sv = one_minus * pv + decay * sv;
      reinterpret_cast<f32x4*>(sh)[i] = sv;
    }
    for (int i = 4 * nvec + tid; i < n; i += THREADS) sh[i] = one_minus * p[i] + decay * sh[i];
  }
}

// ---- the loss: mean((t - x)^2 w) over x, t [outer][inner], w [inner] (losses.py:175-188) ---------------------------------
// The per-element arithmetic is double (x - t is then exact, and a float64 weight is used as float64, as the reference's
// promotion does): term = (x - t)^2 w into the sum, 2 (x - t) w / N rounded once into the gradient.  8 bytes read and 4
// written per element; the double operations stay far below the HBM time.
template <int WMODE>     // 0: no weight, 1: float weight, 2: double weight
__device__ __forceinline__ double weight_at(const void* w, long long j) {
  if (WMODE == 1) return (double)static_cast<const float*>(w)[j];
  if (WMODE == 2) return static_cast<const double*>(w)[j];
  return 1.0;
}

template <int WMODE>
__global__ __launch_bounds__(THREADS) void mse_loss_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                           const void* __restrict__ w, float* __restrict__ grad,
                                                           double* __restrict__ partials, long long n, long long inner,
                                                           double two_over_n) {
  __shared__ double s[THREADS];
  const int tid = threadIdx.x;
  const bool vec = aligned16(x) && aligned16(t) && aligned16(grad);
  double acc = 0.0;
  for (long long base = (long long)blockIdx.x * LOSS_SWEEP; base < n; base += (long long)gridDim.x * LOSS_SWEEP) {
#pragma unroll
    for (int j = 0; j < LOSS_SWEEP / (4 * THREADS); ++j) {
      const long long i = base + 4ll * (tid + THREADS * j);
      if (i >= n) break;
      const int live = n - i < 4 ? (int)(n - i) : 4;
      float xv[4] = {0.f, 0.f, 0.f, 0.f}, tv[4] = {0.f, 0.f, 0.f, 0.f}, gv[4];
      if (vec && live == 4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(x + i), b = *reinterpret_cast<const f32x4*>(t + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          xv[k] = a[k];
          tv[k] = b[k];
        }
      } else {
        for (int k = 0; k < live; ++k) {
          xv[k] = x[i + k];
          tv[k] = t[i + k];
        }
      }
      long long wi = WMODE ? i % inner : 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < live) {
          const double d = (double)xv[k] - (double)tv[k];
          const double wk = weight_at<WMODE>(w, wi);
          acc += d * d * wk;
          gv[k] = (float)(d * wk * two_over_n);
          if (WMODE && ++wi == inner) wi = 0;
        }
      }
      if (grad) {
        if (vec && live == 4) {
          *reinterpret_cast<f32x4*>(grad + i) = f32x4{gv[0], gv[1], gv[2], gv[3]};
        } else {
          for (int k = 0; k < live; ++k) grad[i + k] = gv[k];
        }
      }
    }
  }
  const double sum = block_sum(acc, s);
  if (tid == 0) partials[blockIdx.x] = sum;
}

// out[0] (double) = sum of the partials / n, and the same value as a float in the third float of the 16-byte block
__global__ __launch_bounds__(THREADS) void mse_loss_finish_kernel(const double* __restrict__ partials, int n_partials, double n,
                                                                  double* __restrict__ out) {
  __shared__ double s[THREADS];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_partials; i += THREADS) acc += partials[i];
  const double sum = block_sum(acc, s);
  if (threadIdx.x == 0) {
    const double mean = sum / n;
    out[0] = mean;
    reinterpret_cast<float*>(out)[2] = (float)mean;
  }
}

// grad *= upstream, the scalar read on the device; nothing is read or written when it is exactly 1
template <class S>
__global__ __launch_bounds__(THREADS) void scale_by_scalar_kernel(float* __restrict__ g, const S* __restrict__ upstream,
                                                                  long long n) {
  const float u = (float)upstream[0];
  if (u == 1.0f) return;
  const long long stride = (long long)gridDim.x * THREADS;
  const long long nvec = aligned16(g) ? n >> 2 : 0;
  for (long long i = (long long)blockIdx.x * THREADS + threadIdx.x; i < nvec; i += stride) {
    f32x4 v = reinterpret_cast<f32x4*>(g)[i];
    v *= u;
    reinterpret_cast<f32x4*>(g)[i] = v;
  }
  for (long long i = 4 * nvec + (long long)blockIdx.x * THREADS + threadIdx.x; i < n; i += stride) g[i] *= u;
}

static int loss_partials(int64_t n) {
  if (n <= 0) return 0;
  const int64_t p = (n + LOSS_SWEEP - 1) / LOSS_SWEEP;
  return (int)(p < MAX_BLOCKS ? p : MAX_BLOCKS);
}

static unsigned grid_for(int n_chunks) { return (unsigned)(n_chunks < MAX_BLOCKS ? n_chunks : MAX_BLOCKS); }

}  // namespace optim
}  // namespace dlwp

using namespace dlwp;

extern "C" int32_t dlwp_mt_chunk_elems(void) { return optim::CHUNK; }

extern "C" int32_t dlwp_mse_loss_partials(int64_t n) { return optim::loss_partials(n); }

extern "C" int32_t dlwp_mse_loss_f32(const float* x, const float* t, const void* w, int32_t w_is_f64, float* grad,
                                     double* partials, double* out, int64_t outer, int64_t inner, void* stream) {
  DLWP_REQUIRE(x && t && partials && out, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(outer > 0 && inner > 0 && outer <= INT64_MAX / inner, DLWP_ERR_INVALID_ARGUMENT, "bad shape");
  const long long n = (long long)outer * inner;
  const int P = optim::loss_partials(n);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const double two_over_n = 2.0 / (double)n;
  if (!w)
    hipLaunchKernelGGL(optim::mse_loss_kernel<0>, dim3(P), dim3(optim::THREADS), 0, s, x, t, w, grad, partials, n,
                       (long long)inner, two_over_n);
  else if (!w_is_f64)
    hipLaunchKernelGGL(optim::mse_loss_kernel<1>, dim3(P), dim3(optim::THREADS), 0, s, x, t, w, grad, partials, n,
                       (long long)inner, two_over_n);
  else
    hipLaunchKernelGGL(optim::mse_loss_kernel<2>, dim3(P), dim3(optim::THREADS), 0, s, x, t, w, grad, partials, n,
                       (long long)inner, two_over_n);
  hipLaunchKernelGGL(optim::mse_loss_finish_kernel, dim3(1), dim3(optim::THREADS), 0, s, (const double*)partials, P,
                     (double)n, out);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" int32_t dlwp_mse_loss_scale_grad_f32(float* grad, const void* upstream, int32_t upstream_is_f64, int64_t n,
                                                void* stream) {
  DLWP_REQUIRE(grad && upstream, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(n > 0, DLWP_ERR_INVALID_ARGUMENT, "bad size");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const long long per_block = 4ll * optim::THREADS * 4;
  long long blocks = ((long long)n + per_block - 1) / per_block;
  if (blocks > optim::MAX_BLOCKS) blocks = optim::MAX_BLOCKS;
  if (upstream_is_f64)
    hipLaunchKernelGGL(optim::scale_by_scalar_kernel<double>, dim3((unsigned)blocks), dim3(optim::THREADS), 0, s, grad,
                       static_cast<const double*>(upstream), (long long)n);
  else
    hipLaunchKernelGGL(optim::scale_by_scalar_kernel<float>, dim3((unsigned)blocks), dim3(optim::THREADS), 0, s, grad,
                       static_cast<const float*>(upstream), (long long)n);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" int32_t dlwp_mt_grad_norm_f32(const int64_t* g_ptrs, const int64_t* numel, const int32_t* chunk_tensor,
                                         const int64_t* chunk_first, int32_t n_chunks, float* partials, float max_norm,
                                         float* scal, void* stream) {
  DLWP_REQUIRE(g_ptrs && numel && chunk_tensor && chunk_first && partials && scal, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(n_chunks >= 0, DLWP_ERR_INVALID_ARGUMENT, "bad chunk count");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (n_chunks > 0)
    hipLaunchKernelGGL(optim::mt_sumsq_kernel, dim3(optim::grid_for(n_chunks)), dim3(optim::THREADS), 0, s, g_ptrs, numel,
                       chunk_tensor, chunk_first, n_chunks, partials);
  hipLaunchKernelGGL(optim::mt_norm_finish_kernel, dim3(1), dim3(optim::THREADS), 0, s, (const float*)partials, n_chunks,
                     max_norm, scal);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" int32_t dlwp_mt_scale_f32(const int64_t* g_ptrs, const int64_t* numel, const int32_t* chunk_tensor,
                                     const int64_t* chunk_first, int32_t n_chunks, const float* scal, void* stream) {
  DLWP_REQUIRE(g_ptrs && numel && chunk_tensor && chunk_first && scal, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(n_chunks >= 0, DLWP_ERR_INVALID_ARGUMENT, "bad chunk count");
  if (n_chunks == 0) return DLWP_OK;
  hipLaunchKernelGGL(optim::mt_scale_kernel, dim3(optim::grid_for(n_chunks)), dim3(optim::THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), g_ptrs, numel, chunk_tensor, chunk_first, n_chunks, scal);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" int32_t dlwp_mt_zero_f32(const int64_t* g_ptrs, const int64_t* numel, const int32_t* chunk_tensor,
                                    const int64_t* chunk_first, int32_t n_chunks, void* stream) {
  DLWP_REQUIRE(g_ptrs && numel && chunk_tensor && chunk_first, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(n_chunks >= 0, DLWP_ERR_INVALID_ARGUMENT, "bad chunk count");
  if (n_chunks == 0) return DLWP_OK;
  hipLaunchKernelGGL(optim::mt_zero_kernel, dim3(optim::grid_for(n_chunks)), dim3(optim::THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), g_ptrs, numel, chunk_tensor, chunk_first, n_chunks);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" int32_t dlwp_mt_adamw_f32(const int64_t* p_ptrs, const int64_t* g_ptrs, const int64_t* numel, const int64_t* state_off,
                                     const int32_t* group, int32_t* step, float* derived, const double* hyper, int32_t n_tensors,
                                     const int32_t* chunk_tensor, const int64_t* chunk_first, int32_t n_chunks, float* exp_avg,
                                     float* exp_avg_sq, const float* scal, void* stream) {
  DLWP_REQUIRE(p_ptrs && g_ptrs && numel && state_off && group && step && derived && hyper && chunk_tensor && chunk_first &&
                   exp_avg && exp_avg_sq,
               DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(n_tensors >= 0 && n_chunks >= 0, DLWP_ERR_INVALID_ARGUMENT, "bad table size");
  DLWP_REQUIRE((reinterpret_cast<uintptr_t>(exp_avg) & 15) == 0 && (reinterpret_cast<uintptr_t>(exp_avg_sq) & 15) == 0,
               DLWP_ERR_INVALID_ARGUMENT, "the state arenas must be 16-byte aligned");
  if (n_tensors == 0 || n_chunks == 0) return DLWP_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(optim::adamw_header_kernel, dim3((unsigned)((n_tensors + 255) / 256)), dim3(256), 0, s, g_ptrs, group, hyper,
                     step, derived, n_tensors);
  hipLaunchKernelGGL(optim::mt_adamw_kernel, dim3(optim::grid_for(n_chunks)), dim3(optim::THREADS), 0, s, p_ptrs, g_ptrs, numel,
                     state_off, (const float*)derived, chunk_tensor, chunk_first, n_chunks, exp_avg, exp_avg_sq, scal);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" int32_t dlwp_mt_ema_f32(const int64_t* p_ptrs, const int64_t* numel, const int64_t* state_off,
                                   const int32_t* chunk_tensor, const int64_t* chunk_first, int32_t n_chunks, float* shadow,
                                   float decay, float one_minus_decay, void* stream) {
  DLWP_REQUIRE(p_ptrs && numel && state_off && chunk_tensor && chunk_first && shadow, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(n_chunks >= 0, DLWP_ERR_INVALID_ARGUMENT, "bad chunk count");
  DLWP_REQUIRE((reinterpret_cast<uintptr_t>(shadow) & 15) == 0, DLWP_ERR_INVALID_ARGUMENT,
               "the shadow arena must be 16-byte aligned");
  if (n_chunks == 0) return DLWP_OK;
  hipLaunchKernelGGL(optim::mt_ema_kernel, dim3(optim::grid_for(n_chunks)), dim3(optim::THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), p_ptrs, numel, state_off, chunk_tensor, chunk_first, n_chunks, shadow,
                     decay, one_minus_decay);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}
