// The device generator of csrc/refiner.hip: a counter-based stream of standard normals.  Every kernel that needs noise
// includes this header and evaluates the SAME function of (seed, global element index): a draw depends on neither the grid
// nor on how a range is split across launches.
//
//   generator   Philox4x32-10 (Salmon et al., SC 2011; Random123): multipliers 0xD2511F53 / 0xCD9E8D57, the key bumped by
//               the Weyl constants 0x9E3779B9 / 0xBB67AE85 between rounds; key = (seed low word, seed high word),
//               counter = (q low word, q high word, 0, 0)
//   indexing    element e of a draw with base `offset` (a multiple of 4) has the global index g = offset + e and is lane
//               g % 4 of block q = g / 4
//   uniforms    u = float(x) * 2^-32 + 2^-33 in fp32 (the product is exact, the sum is rounded once): never 0
//   normals     Box-Muller per word pair: r = sqrt(-2 ln u_a), theta = 6.2831855f * u_b (fp32); (x0, x1) give lanes 0 / 1 =
//               r cos theta / r sin theta, (x2, x3) lanes 2 / 3
// tests/philox_ref.py restates this in numpy (and checks the Random123 known-answer vectors).
#pragma once

#include "common.hpp"

namespace dlwp {
namespace philox {

struct u32x4s {
  uint32_t x, y, z, w;
};

__host__ __device__ __forceinline__ u32x4s philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                         uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return u32x4s{c0, c1, c2, c3};
}

__device__ __forceinline__ float uniform01(uint32_t x) { return (float)x * 2.3283064365386963e-10f + 1.1641532182693481e-10f; }

__device__ __forceinline__ void box_muller(uint32_t xa, uint32_t xb, float& n0, float& n1) {
  const float r = sqrtf(-2.0f * logf(uniform01(xa)));
  const float theta = 6.2831855f * uniform01(xb);
  float s, c;
  sincosf(theta, &s, &c);
  n0 = r * c;
  n1 = r * s;
}

// the four normals of block q
__device__ __forceinline__ f32x4 normal4(uint64_t seed, uint64_t q) {
  const u32x4s x = philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
  f32x4 z;
  float a, b;
  box_muller(x.x, x.y, a, b);
  z[0] = a;
  z[1] = b;
  box_muller(x.z, x.w, a, b);
  z[2] = a;
  z[3] = b;
  return z;
}

}  // namespace philox
}  // namespace dlwp
