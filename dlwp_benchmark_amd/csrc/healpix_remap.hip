// HEALPix -> lat-lon remap on the device.  The reference remaps every rollout before it scores it (scripts/evaluate.py:79-116,
// 298-303, scripts/train.py:430-441) with HEALPixRemap.hpx2ll (data/processing/healpix_mapping.py:372-404) on the host, one
// (sample, step, variable) plane per call: a Python loop over the pixels, then reproject's bilinear interpolation.  The map is
// linear and fixed, so the host evaluates it once into a table of four (cell, weight) taps per lat-lon cell
// (dlwp_benchmark_amd/healpix.py:latlon_table) and this kernel applies the table to every plane:
//
//   y[p][q] = ((w0 x[p][i0] + w1 x[p][i1]) + w2 x[p][i2]) + w3 x[p][i3]        fp32, this order, no FMA contraction
//
// The table is 32 B per output cell against 4 B written per plane, so a thread reads its cells' taps ONCE into registers and
// walks a block of planes with them.  Stores are coalesced along `cells` (consecutive lanes, consecutive q); the taps of
// neighbouring lat-lon cells are neighbouring HEALPix cells of a plane that is a few KB to a few hundred KB, so the gathers
// hit L1/L2 and HBM sees each plane once.  The workgroups of one plane block are consecutive in the (one-dimensional) grid:
// they run at the same time and share those planes in L2.  No zero-weight tap is skipped: a NaN tap makes NaN as it does in
// numpy.  Indices are checked against 12 nside^2 where the table is built, not here.
#include "common.hpp"

namespace dlwp {
namespace hpxremap {

constexpr int kThreads = 256;
constexpr int kPlanesPerBlock = 16;
// A workgroup covers kThreads * kCellsPerThread CONSECUTIVE cells, a thread kCellsPerThread of them kThreads apart (every store
// instruction of a wave is 256 contiguous bytes).  Why more than one: along a circle of latitude consecutive HEALPix cells sit
// one face row apart (n - 1 floats), so from nside 32 up every gather of a wave lands in a cache line of its own, and the
// lines a run of cells needs -- one per ring pixel it spans -- are the lines the next circles of latitude need too.  A
// workgroup that covers several circles (1024 cells = 2.8 rows of a 180 x 360 grid) fetches them from L2 once.  Measured
// against one cell per thread: 1.7x faster at nside 64, equal at nside 32, 3 % faster on the 32 x 64
// grid; eight are no better.
#ifndef DLWP_REMAP_CELLS_PER_THREAD
#define DLWP_REMAP_CELLS_PER_THREAD 4     /* A/B builds */
#endif
constexpr int kCellsPerThread = DLWP_REMAP_CELLS_PER_THREAD;

template <int R>
__global__ __launch_bounds__(kThreads) void to_latlon_kernel(const float* __restrict__ x, const int4* __restrict__ index,
                                                            const float4* __restrict__ weight, float* __restrict__ y,
                                                            long long planes, int npix, int cells, int tiles) {
  constexpr int U = R >= 8 ? 1 : (R >= 4 ? 2 : 4);       // planes whose gathers are in flight together (16 to 32 loads)
  const int tile = blockIdx.x % tiles;
  const long long p0 = (long long)(blockIdx.x / tiles) * kPlanesPerBlock;
  const long long q0 = (long long)tile * (kThreads * R) + threadIdx.x;
  int4 i[R];
  float4 w[R];
  bool ok[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {          // a cell past the end reads cell 0 of the plane and stores nothing
    const long long q = q0 + r * kThreads;
    ok[r] = q < cells;
    i[r] = ok[r] ? index[q] : int4{0, 0, 0, 0};
    w[r] = ok[r] ? weight[q] : float4{0.f, 0.f, 0.f, 0.f};
  }
  const long long left = planes - p0;
  const int np = left < kPlanesPerBlock ? (int)left : kPlanesPerBlock;
  const float* xp = x + p0 * npix;
  float* yp = y + p0 * cells + q0;
  int p = 0;
  for (; p + U <= np; p += U) {
    float v[U][R][4];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float* xu = xp + (long long)(p + u) * npix;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        v[u][r][0] = xu[i[r].x];
        v[u][r][1] = xu[i[r].y];
        v[u][r][2] = xu[i[r].z];
        v[u][r][3] = xu[i[r].w];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (ok[r])
          yp[(long long)(p + u) * cells + r * kThreads] =
              ((w[r].x * v[u][r][0] + w[r].y * v[u][r][1]) + w[r].z * v[u][r][2]) + w[r].w * v[u][r][3];
  }
  for (; p < np; ++p) {
    const float* xu = xp + (long long)p * npix;
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (ok[r])
        yp[(long long)p * cells + r * kThreads] =
            ((w[r].x * xu[i[r].x] + w[r].y * xu[i[r].y]) + w[r].z * xu[i[r].z]) + w[r].w * xu[i[r].w];
  }
}

}  // namespace hpxremap
}  // namespace dlwp

using namespace dlwp;

extern "C" int32_t dlwp_healpix_to_latlon_f32(const float* x_dev, const int32_t* index_dev, const float* weight_dev, float* y_dev,
                                              int64_t planes, int32_t nside, int32_t cells, void* stream) {
  DLWP_REQUIRE(x_dev && index_dev && weight_dev && y_dev, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(planes >= 1 && cells >= 1, DLWP_ERR_INVALID_ARGUMENT, "planes and cells must be at least 1");
  DLWP_REQUIRE(nside >= 1 && nside <= 8192, DLWP_ERR_INVALID_ARGUMENT, "nside %d outside 1..8192", nside);
  DLWP_REQUIRE((reinterpret_cast<uintptr_t>(index_dev) | reinterpret_cast<uintptr_t>(weight_dev)) % 16 == 0,
               DLWP_ERR_INVALID_ARGUMENT, "the table must be 16-byte aligned");
  const int npix = 12 * nside * nside;   // <= 805306368
  const long long per_block = (long long)hpxremap::kThreads * hpxremap::kCellsPerThread;
  const long long tiles = ((long long)cells + per_block - 1) / per_block;
  const long long plane_blocks = (planes + hpxremap::kPlanesPerBlock - 1) / hpxremap::kPlanesPerBlock;
  DLWP_REQUIRE(plane_blocks <= 0x7fffffffLL / tiles, DLWP_ERR_UNSUPPORTED, "grid too large: %lld planes of %d cells",
               (long long)planes, cells);
  hipLaunchKernelGGL(hpxremap::to_latlon_kernel<hpxremap::kCellsPerThread>, dim3((unsigned)(tiles * plane_blocks)), dim3(hpxremap::kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), x_dev, reinterpret_cast<const int4*>(index_dev),
                     reinterpret_cast<const float4*>(weight_dev), y_dev, (long long)planes, npix, cells, (int)tiles);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}
