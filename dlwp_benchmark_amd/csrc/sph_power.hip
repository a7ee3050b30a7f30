// Spherical power spectra of a rollout and its targets, reduced on the device (the reference has no
// spherical spectrum -- PARITY UNPINNED, the definitions are pinned by mathematics as those of sht.hip are).  For a unit
// (b, k, c) of out / target [B, K, C, nlat, nlon] the three planes out, target and out - target (the difference formed in the
// field domain, in fp32) go through the two stages of the forward transform (sht_stages.hpp, shared with sht_kernel); with
// c = sht(.) and f_m = 1 for the self-conjugate columns m = 0 and 2 m = nlon (whose imaginary parts are dropped), 2 otherwise:
//   sums[0][k][c][l] = sum_b sum_{m <= min(l, mmax - 1)} f_m |c_out[l][m]|^2          1: the same of target
//   sums[2][k][c][l] = the same of out - target           sums[3][k][c][l] = sum_b sum_m f_m Re(c_out[l][m] conj c_target[l][m])
// No coefficient is written to memory.  Two launches:
//
//   sph_power_kernel    a workgroup takes kUnits units and a tile of mt zonal wavenumbers, exactly as sht_kernel takes planes:
//                       rows go through LDS in chunks (the difference is formed as they are staged), the DFT stage leaves X in
//                       LDS, then a thread owns (l, m), contracts over latitude for its 3 kUnits planes -- every twiddle and
//                       table load is shared by them -- and forms the four f_m-weighted terms in fp64 (zero for l < m).  Degrees
//                       are taken `lp` at a time: the terms of a pass go to LDS (the row staging area, free by then), and one
//                       thread per (degree, unit, quantity) adds them over the tile's m in ascending order in fp64 and stores
//                       ONE partial per (unit, m tile, quantity, l) in the workspace.
//   sph_power_combine_kernel   one thread per (quantity, k, c, l) adds the partials in one fp64 chain, b ascending and m tiles
//                       ascending inside a b, starting from zero or (the _acc entry point) from what the sums hold: a batch cut
//                       anywhere and fed through _acc gives the bits of the one-shot call.
//
// The tiling (kUnits, mt, rt, lp) is a function of (nlat, nlon, lmax, mmax) alone and a unit's arithmetic does not look at its
// neighbours, so a unit's partials do not depend on the batch or on which units share its workgroup.  No atomics, no
// transcendental.
#include <algorithm>

#include "sht_stages.hpp"

namespace dlwp {
namespace sphp {

using sht::kThreads;

// LDS: tw [nlon] float2 | X [3 kUnits][nlat][mt] float2 | xs [3 kUnits][rt][nlon] float, later terms [lp][4 kUnits][mt + 1] double
template <int kUnits>
__global__ __launch_bounds__(kThreads) void sph_power_kernel(const float* __restrict__ out, const float* __restrict__ tar,
                                                             const float* __restrict__ wleg, const float2* __restrict__ tw,
                                                             double* __restrict__ part,      // [units][mtiles][4][lmax]
                                                             long long units, int nlat, int nlon, int lmax, int mmax, int mt, int rt,
                                                             int mtiles, int lp, sht::TableStrides ts, sht::ColumnFactor cf) {
  constexpr int kPlanes = 3 * kUnits, kQ = 4 * kUnits;
  extern __shared__ __align__(16) unsigned char smem[];
  float2* tws = reinterpret_cast<float2*>(smem);
  float2* Xs = tws + nlon;
  float* xs = reinterpret_cast<float*>(Xs + (size_t)kPlanes * nlat * mt);
  double* terms = reinterpret_cast<double*>(xs);      // 8-byte aligned: everything before it is float2
  const int tid = threadIdx.x;
  const int mtile = (int)(blockIdx.x % mtiles), m0 = mtile * mt;
  const long long u0 = (long long)(blockIdx.x / mtiles) * kUnits;
  const int mn = min(mt, mmax - m0);
  const int nu = (int)min((long long)kUnits, units - u0);
  for (int t = tid; t < nlon; t += kThreads) tws[t] = tw[t];
  for (int k0 = 0; k0 < nlat; k0 += rt) {
    const int rn = min(rt, nlat - k0);
    __syncthreads();          // the chunk before has been read (first pass: nothing to wait for)
#pragma unroll
    for (int u = 0; u < kUnits; ++u) {
      const long long at = ((u0 + u) * nlat + k0) * (long long)nlon;      // only dereferenced for u < nu
      float* dst = xs + 3 * u * rt * nlon;
      for (int e = tid; e < rn * nlon; e += kThreads) {
        const float a = u < nu ? out[at + e] : 0.f, b = u < nu ? tar[at + e] : 0.f;
        dst[e] = a;
        dst[rt * nlon + e] = b;
        dst[2 * rt * nlon + e] = a - b;
      }
    }
    __syncthreads();
    sht::dft_rows<kPlanes>(xs, tws, Xs, tid, k0, rn, m0, mn, nlat, nlon, mt, rt, cf);
  }
  __syncthreads();            // X is complete, and xs has been read for the last time: its space now holds the terms
  const int col = mt + 1, stride = kQ * col;          // [degree][unit, quantity][m]: a wave writes consecutive m; the threads of the
                                                      // m sum, mt + 1 doubles apart, read different banks where mt is a power of two
  for (int l0 = 0; l0 < lmax; l0 += lp) {
    const int ln = min(lp, lmax - l0);
    for (int it = tid; it < ln * mn; it += kThreads) {
      const int ll = it / mn, mm = it - ll * mn, m = m0 + mm;
      float ar[kPlanes], ai[kPlanes];
      sht::legendre_column<kPlanes>(Xs, wleg, ts, l0 + ll, m, mm, nlat, mt, ar, ai);
      const double f = (m == 0 || 2 * m == nlon) ? 1.0 : 2.0;
      double* t = terms + (size_t)ll * stride + mm;
#pragma unroll
      for (int u = 0; u < kUnits; ++u) {
        const double xr = ar[3 * u], xi = ai[3 * u], yr = ar[3 * u + 1], yi = ai[3 * u + 1], dr = ar[3 * u + 2], di = ai[3 * u + 2];
        t[(4 * u) * col] = f * (xr * xr + xi * xi);
        t[(4 * u + 1) * col] = f * (yr * yr + yi * yi);
        t[(4 * u + 2) * col] = f * (dr * dr + di * di);
        t[(4 * u + 3) * col] = f * (xr * yr + xi * yi);
      }
    }
    __syncthreads();
    for (int e = tid; e < ln * kQ; e += kThreads) {
      const int ll = e / kQ, qu = e - ll * kQ, u = qu >> 2, q = qu & 3;
      if (u < nu) {
        const double* t = terms + (size_t)ll * stride + qu * col;
        double s = 0.0;
        for (int mm = 0; mm < mn; ++mm) s += t[mm];
        part[(((u0 + u) * mtiles + mtile) * 4 + q) * lmax + l0 + ll] = s;
      }
    }
    __syncthreads();          // the terms are rewritten by the next pass
  }
}

// sums[q][kc][l] (+)= sum_b sum_t part[b kc_n + kc][t][q][l], one chain per thread
__global__ __launch_bounds__(256) void sph_power_combine_kernel(const double* __restrict__ part, double* __restrict__ sums,
                                                                long long n, int batch, long long kc_n, int lmax, int mtiles,
                                                                int accumulate) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int l = (int)(i % lmax);
  const long long r = i / lmax, kc = r % kc_n, q = r / kc_n;
  double tot = accumulate ? sums[i] : 0.0;
  for (int b = 0; b < batch; ++b)
    for (int t = 0; t < mtiles; ++t) tot += part[(((b * kc_n + kc) * mtiles + t) * 4 + q) * lmax + l];
  sums[i] = tot;
}

// The tiling of a shape: units per workgroup, the two tile extents of fit_tiles, degrees per pass, LDS bytes.
struct Plan {
  int units = 0, mt = 0, rt = 0, lp = 0;
  size_t bytes = 0;
};

// `units` units per workgroup: sht_kernel's plan for 3 `units` planes, then as many degrees per pass as give every thread an
// item and whose terms fit the staging area; where even one degree's terms do not (few rows, many m), the tile of m is halved.
static bool plan_for(int units, int nlat, int nlon, int lmax, int mmax, Plan& p) {
  const size_t planes = 3 * (size_t)units, fixed = (size_t)nlon * 8;
  p.units = units;
  p.mt = mmax, p.rt = nlat;
  if (!sht::fit_tiles(fixed, planes * nlat * 8, p.mt, planes * nlon * 4, p.rt, p.bytes)) return false;
  for (;;) {
    const size_t xs_bytes = planes * p.rt * nlon * 4, row_bytes = (size_t)4 * units * (p.mt + 1) * 8;
    p.lp = std::min(std::max(1, sht::kThreads / p.mt), lmax);
    p.lp = (int)std::max<size_t>(1, std::min<size_t>(p.lp, xs_bytes / row_bytes));
    p.bytes = fixed + planes * nlat * 8 * p.mt + std::max(xs_bytes, row_bytes * p.lp);
    if (p.bytes <= sht::kLdsBudget) return true;
    if (p.mt == 1) return false;
    p.mt = (p.mt + 1) / 2;
  }
}

// Two units per workgroup where that costs no further tile of m (a tile more reads out and target once more) and still gives
// every thread an item of the DFT stage; one otherwise.  A function of the four extents alone.
static bool plan_of(int nlat, int nlon, int lmax, int mmax, Plan& p) {
  Plan one, two;
  if (!plan_for(1, nlat, nlon, lmax, mmax, one)) return false;
  p = one;
  if (plan_for(2, nlat, nlon, lmax, mmax, two) && two.mt == one.mt &&
      ((long long)two.mt * two.rt >= sht::kThreads || (two.mt == mmax && two.rt == nlat)))
    p = two;
  return true;
}

static bool shape_ok(int32_t b, int32_t k, int32_t c, int32_t nlat, int32_t nlon, int32_t lmax, int32_t mmax) {
  return b >= 1 && k >= 1 && c >= 1 && nlat >= 2 && nlat <= 256 && nlon >= 2 && nlon <= 512 && nlon % 2 == 0 && lmax >= 1 &&
         lmax <= nlat && mmax >= 1 && mmax <= nlon / 2 + 1;
}

}  // namespace sphp
}  // namespace dlwp

using namespace dlwp;

extern "C" size_t dlwp_sph_power_workspace_bytes(int32_t b, int32_t k, int32_t c, int32_t nlat, int32_t nlon, int32_t lmax,
                                                 int32_t mmax) {
  sphp::Plan p;
  if (!sphp::shape_ok(b, k, c, nlat, nlon, lmax, mmax) || !sphp::plan_of(nlat, nlon, lmax, mmax, p)) return 0;
  const size_t mtiles = ((size_t)mmax + p.mt - 1) / p.mt;
  return sizeof(double) * 4 * (size_t)b * k * c * mtiles * lmax;
}

static int32_t sph_power_sums(const float* out, const float* target, const float* wleg, const float* tw, double* sums, int32_t b,
                              int32_t k, int32_t c, int32_t nlat, int32_t nlon, int32_t lmax, int32_t mmax, void* workspace,
                              size_t workspace_bytes, void* stream, bool accumulate) {
  DLWP_REQUIRE(out && target && sums && workspace, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(b >= 1 && k >= 1 && c >= 1, DLWP_ERR_INVALID_ARGUMENT, "b, k and c must be at least 1");
  const long long units = (long long)b * k * c;
  if (int32_t rc = sht::check_transform(out, wleg, tw, sums, units, nlat, nlon, lmax, mmax)) return rc;
  DLWP_REQUIRE((reinterpret_cast<uintptr_t>(tw) | reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(workspace)) % 8 == 0,
               DLWP_ERR_INVALID_ARGUMENT, "tw_dev, sums_dev and workspace_dev must be 8-byte aligned");
  sphp::Plan p;
  DLWP_REQUIRE(sphp::plan_of(nlat, nlon, lmax, mmax, p), DLWP_ERR_UNSUPPORTED, "no tiling of %d x %d fits the LDS budget", nlat, nlon);
  const long long mtiles = (mmax + p.mt - 1) / p.mt, groups = (units + p.units - 1) / p.units;
  const long long n = 4LL * k * c * lmax;
  DLWP_REQUIRE(groups <= 0x7fffffffLL / mtiles && n <= 0x7fffffffLL * 256, DLWP_ERR_UNSUPPORTED, "grid too large: %lld units",
               units);
  const size_t need = dlwp_sph_power_workspace_bytes(b, k, c, nlat, nlon, lmax, mmax);
  DLWP_REQUIRE(workspace_bytes >= need, DLWP_ERR_WORKSPACE, "spherical spectrum workspace: %zu bytes given, %zu needed",
               workspace_bytes, need);
  const float scale = (float)(2.0 * 3.14159265358979323846 / (double)nlon);
  const sht::TableStrides ts{(size_t)lmax * mmax, (size_t)mmax};        // wleg [k][l][m]
  const sht::ColumnFactor cf{scale, scale, true};                       // the imaginary parts of m = 0 and 2 m = nlon are dropped
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  double* part = reinterpret_cast<double*>(workspace);
  auto kernel = p.units == 2 ? sphp::sph_power_kernel<2> : sphp::sph_power_kernel<1>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(groups * mtiles)), dim3(sht::kThreads), p.bytes, s, out, target, wleg,
                     reinterpret_cast<const float2*>(tw), part, units, nlat, nlon, lmax, mmax, p.mt, p.rt, (int)mtiles, p.lp, ts, cf);
  DLWP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(sphp::sph_power_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, sums, n, b,
                     (long long)k * c, lmax, (int)mtiles, accumulate ? 1 : 0);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" int32_t dlwp_sph_power_sums_f32(const float* out_dev, const float* target_dev, const float* wleg_dev, const float* tw_dev,
                                           double* sums_dev, int32_t b, int32_t k, int32_t c, int32_t nlat, int32_t nlon,
                                           int32_t lmax, int32_t mmax, void* workspace_dev, size_t workspace_bytes, void* stream) {
  return sph_power_sums(out_dev, target_dev, wleg_dev, tw_dev, sums_dev, b, k, c, nlat, nlon, lmax, mmax, workspace_dev,
                        workspace_bytes, stream, false);
}

// the same sums ADDED to what sums_dev holds (the running sums of an evaluation over many batches)
extern "C" int32_t dlwp_sph_power_sums_acc_f32(const float* out_dev, const float* target_dev, const float* wleg_dev,
                                               const float* tw_dev, double* sums_dev, int32_t b, int32_t k, int32_t c, int32_t nlat,
                                               int32_t nlon, int32_t lmax, int32_t mmax, void* workspace_dev, size_t workspace_bytes,
                                               void* stream) {
  return sph_power_sums(out_dev, target_dev, wleg_dev, tw_dev, sums_dev, b, k, c, nlat, nlon, lmax, mmax, workspace_dev,
                        workspace_bytes, stream, true);
}
