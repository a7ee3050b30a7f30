// The two stages of the forward spherical harmonic transform as device code, shared by sht_kernel (sht.hip: the coefficients
// are the result) and sph_power_kernel (sph_power.hip: the coefficients stay in registers and only their power per degree
// leaves the workgroup), with the LDS layout, the tile planner and the envelope check both launches use.
//
// LDS of a workgroup of kPlanes planes and a tile of mt zonal wavenumbers, rows staged rt at a time:
//   tw [nlon] float2 | X [kPlanes][nlat][mt] float2 | xs [kPlanes][rt][nlon] float
#pragma once

#include "common.hpp"

namespace dlwp {
namespace sht {

constexpr int kThreads = 256;
constexpr size_t kLdsBudget = 52 * 1024;     // three workgroups per compute unit (160 KB)

// Each transform's backward is the OTHER kernel over the table its forward reads (both are linear: the adjoint of "DFT, then
// contract over latitude" is "contract over degree, then DFT back").  What differs between a kernel's two uses is carried by
// two small arguments, not by a second copy of the kernel:
//   TableStrides  where the Legendre table keeps (row k, degree l) for column m: wleg is [k][l][m], leg is [l][k][m].  m is the
//                 fastest index of both, so the lanes of a wave (consecutive m) read consecutive floats either way.
//   ColumnFactor  what multiplies column m between the two stages: the quadrature's 2 pi / nlon (forward sht and the adjoint of
//                 sht), or irfft's Hermitian weights -- 1 for the self-conjugate columns m = 0 and 2 m = nlon, whose imaginary
//                 parts are dropped, 2 for the others (isht and the adjoint of isht).
struct TableStrides {
  size_t row, degree;
};
struct ColumnFactor {
  float self_conjugate, other;
  bool drop_imag;             // zero the imaginary part of the self-conjugate columns
};

// DFT stage of one row chunk: rows [k0, k0 + rn) of kPlanes planes lie in xs; a thread owns (row k, m) and forms
// X[k][m] = f_m sum_j x[k][j] tw[(j m) mod nlon] for its planes from the twiddle table in LDS, and leaves it in Xs.
template <int kPlanes>
__device__ __forceinline__ void dft_rows(const float* __restrict__ xs, const float2* __restrict__ tws, float2* __restrict__ Xs,
                                         int tid, int k0, int rn, int m0, int mn, int nlat, int nlon, int mt, int rt,
                                         ColumnFactor cf) {
  for (int it = tid; it < rn * mn; it += kThreads) {
    const int kk = it / mn, mm = it - kk * mn, m = m0 + mm;
    float ar[kPlanes], ai[kPlanes];
#pragma unroll
    for (int p = 0; p < kPlanes; ++p) ar[p] = ai[p] = 0.f;
    const float* row = xs + kk * nlon;
    int idx = 0;            // (j m) mod nlon; m < nlon, so one subtraction wraps it
#pragma unroll 4
    for (int j = 0; j < nlon; ++j) {
      const float2 w = tws[idx];
      idx += m;
      if (idx >= nlon) idx -= nlon;
#pragma unroll
      for (int p = 0; p < kPlanes; ++p) {
        const float v = row[p * rt * nlon + j];
        ar[p] = fmaf(v, w.x, ar[p]);
        ai[p] = fmaf(v, w.y, ai[p]);
      }
    }
    const bool self_conjugate = m == 0 || 2 * m == nlon;      // only the adjoint of isht and the power sums tell them apart
    const float f = self_conjugate ? cf.self_conjugate : cf.other;
#pragma unroll
    for (int p = 0; p < kPlanes; ++p)
      Xs[(p * nlat + k0 + kk) * mt + mm] = float2{ar[p] * f, self_conjugate && cf.drop_imag ? 0.f : ai[p] * f};
  }
}

// Legendre contraction of one (l, m = m0 + mm): c[p] = sum_k table[k][l][m] X[p][k][mm], k ascending; zero for l < m, which
// costs no loop.  One table load feeds kPlanes complex FMAs; the lanes of a wave read consecutive m.
template <int kPlanes>
__device__ __forceinline__ void legendre_column(const float2* __restrict__ Xs, const float* __restrict__ wleg, TableStrides ts,
                                                int l, int m, int mm, int nlat, int mt, float (&ar)[kPlanes],
                                                float (&ai)[kPlanes]) {
#pragma unroll
  for (int p = 0; p < kPlanes; ++p) ar[p] = ai[p] = 0.f;
  if (l >= m) {
    const float* wp = wleg + l * ts.degree + m;
#pragma unroll 4
    for (int k = 0; k < nlat; ++k) {
      const float w = wp[k * ts.row];
#pragma unroll
      for (int p = 0; p < kPlanes; ++p) {
        const float2 v = Xs[(p * nlat + k) * mt + mm];
        ar[p] = fmaf(w, v.x, ar[p]);
        ai[p] = fmaf(w, v.y, ai[p]);
      }
    }
  }
}

// the two tile extents of a transform kernel: start from "everything in one tile" and halve the larger LDS array until the
// workgroup fits the budget.  a_unit / b_unit: bytes of the two arrays per unit of their extent.
inline bool fit_tiles(size_t fixed, size_t a_unit, int& a, size_t b_unit, int& b, size_t& bytes) {
  for (;;) {
    bytes = fixed + a_unit * a + b_unit * b;
    if (bytes <= kLdsBudget) return true;
    if (a_unit * a >= b_unit * b && a > 1) a = (a + 1) / 2;
    else if (b > 1) b = (b + 1) / 2;
    else if (a > 1) a = (a + 1) / 2;
    else return false;
  }
}

inline int32_t check_transform(const void* a, const void* b, const void* c, const void* d, int64_t planes, int32_t nlat,
                               int32_t nlon, int32_t lmax, int32_t mmax) {
  DLWP_REQUIRE(a && b && c && d, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(planes >= 1, DLWP_ERR_INVALID_ARGUMENT, "planes must be at least 1");
  DLWP_REQUIRE(nlat >= 2 && nlat <= 256 && nlon >= 2 && nlon <= 512 && nlon % 2 == 0 && lmax >= 1 && lmax <= nlat && mmax >= 1 &&
                   mmax <= nlon / 2 + 1,
               DLWP_ERR_UNSUPPORTED, "spherical transform outside the envelope: nlat %d (2..256), nlon %d (even, 2..512), lmax %d "
               "(1..nlat), mmax %d (1..nlon / 2 + 1)", nlat, nlon, lmax, mmax);
  return DLWP_OK;
}

}  // namespace sht
}  // namespace dlwp
