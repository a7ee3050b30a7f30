// Top-of-atmosphere insolation (the prescribed variable `tisr` of the reference configs) generated on the device: reference
// data/datasets/add_insolation.py:9-73 restated as a separable product.
//   sol[t, p] = S (sin lat_p sin dec_t - cos lat_p cos dec_t cos h[t, p]) rho_t^-2,   h = 2 pi (day_t + lon_p / 360)      (:62-69)
// The caller (ops.insolation) tabulates in float64, per date, sin dec, cos dec, rho^-2 and cos / sin of 2 pi frac(day), and per
// point sin lat, cos lat and cos / sin of 2 pi lon / 360; the kernel forms cos h = cos a cos b - sin a sin b and the product
// in fp64 FMAs and rounds once to fp32.  No transcendental runs on the device and no angle is ever held in fp32 (h reaches
// 2300 rad at the end of a year, where an fp32 angle is good to 2e-4).  Values below zero are clipped (:70-71) and the
// dataset's normalisation (x - mean) / std (data/datasets/datasets.py:371) is applied to the rounded value in the same pass.
//
// A thread owns one point: it reads the point's four doubles once and walks TD dates (the date table is read through the
// scalar cache), so a wave's stores are 256 consecutive bytes of one date's field.  One writer per element.
#include "common.hpp"

namespace dlwp {
namespace insol {

constexpr int NT = 256;
constexpr int TD = 8;   // dates per thread

__global__ __launch_bounds__(NT) void insolation_kernel(const double* __restrict__ date_tab,    // [T][5]
                                                        const double* __restrict__ point_tab,   // [N][4]
                                                        float* __restrict__ y, int T, long long N, double S, int clip_zero,
                                                        int normalise, float mean, float scale) {
  const long long p = (long long)blockIdx.x * NT + threadIdx.x;
  if (p >= N) return;
  const double slat = point_tab[4 * p], clat = point_tab[4 * p + 1], clon = point_tab[4 * p + 2], slon = point_tab[4 * p + 3];
  for (int t0 = blockIdx.y * TD; t0 < T; t0 += gridDim.y * TD) {
    const int t1 = t0 + TD < T ? t0 + TD : T;
    for (int t = t0; t < t1; ++t) {
      const double* __restrict__ d = date_tab + 5 * (long long)t;
      const double sdec = d[0], cdec = d[1], rm2 = d[2], cday = d[3], sday = d[4];
      const double cos_h = fma(cday, clon, -(sday * slon));
      const double v = S * fma(slat, sdec, -(clat * cdec * cos_h)) * rm2;
      float f = (float)v;
      if (clip_zero && f < 0.f) f = 0.f;
      if (normalise) f = (f - mean) / scale;
      y[(long long)t * N + p] = f;
    }
  }
}

}  // namespace insol
}  // namespace dlwp

using namespace dlwp;

extern "C" int32_t dlwp_insolation_f32(const double* date_table_dev, const double* point_table_dev, float* out_dev, int32_t dates,
                                       int64_t points, double solar_constant, int32_t clip_zero, int32_t normalise, float mean,
                                       float scale, void* stream) {
  DLWP_REQUIRE(date_table_dev && point_table_dev && out_dev, DLWP_ERR_INVALID_ARGUMENT, "insolation: null argument");
  DLWP_REQUIRE(dates > 0 && points > 0, DLWP_ERR_INVALID_ARGUMENT, "insolation: %d dates, %lld points", dates, (long long)points);
  DLWP_REQUIRE(!normalise || (scale != 0.f && scale == scale && mean == mean), DLWP_ERR_INVALID_ARGUMENT,
               "insolation: normalisation with a zero or NaN scale");
  DLWP_REQUIRE((reinterpret_cast<uintptr_t>(date_table_dev) & 7) == 0 && (reinterpret_cast<uintptr_t>(point_table_dev) & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(out_dev) & 3) == 0,
               DLWP_ERR_INVALID_ARGUMENT, "insolation: misaligned pointer");
  const long long bx = (points + insol::NT - 1) / insol::NT;
  DLWP_REQUIRE(bx <= 0x7fffffffLL, DLWP_ERR_UNSUPPORTED, "insolation: too many points");
  long long by = ((long long)dates + insol::TD - 1) / insol::TD;
  if (by > 65535) by = 65535;
  hipLaunchKernelGGL(insol::insolation_kernel, dim3((unsigned)bx, (unsigned)by), dim3(insol::NT), 0,
                     reinterpret_cast<hipStream_t>(stream), date_table_dev, point_table_dev, out_dev, dates, (long long)points,
                     solar_constant, clip_zero, normalise, mean, scale);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}
