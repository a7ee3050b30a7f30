// The device generator of csrc/refiner.hip: a counter-based stream of standard normals.  Every kernel that needs noise
// includes this header and evaluates the SAME function of (seed, global element index): a draw depends on neither the grid
// nor on how a range is split across launches.
//
//   generator   Philox4x32-10 (Salmon et al., SC 2011; Random123): multipliers 0xD2511F53 / 0xCD9E8D57, the key bumped by
//               the Weyl constants 0x9E3779B9 / 0xBB67AE85 between rounds; key = (seed low word, seed high word),
//               counter = (q low word, q high word, member, 0)
//   members     `member` (a uint32) selects one of 2^32 independent streams of a seed: the draws of ensemble member m of a
//               forecast.  Member 0 is the stream of every call that names no member.  Element (m, e) of a member-major
//               draw [members][n_per_member] with base `offset` is normal(seed, first_member + m, offset + e): a member's
//               values depend on neither how many members are drawn beside it nor where it sits in the call
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

// the four normals of block q of stream `member`
__device__ __forceinline__ f32x4 normal4(uint64_t seed, uint32_t member, uint64_t q) {
  const u32x4s x = philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), member, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
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

// the four normals of block q (member 0)
__device__ __forceinline__ f32x4 normal4(uint64_t seed, uint64_t q) { return normal4(seed, 0u, q); }

// A member-major draw [members][npm] (npm = n_per_member, any positive value): the normals of the flat elements i .. i + 3.
// Flat element t is element e = t % npm of member t / npm and has the stream index 4 q0 + e.  With npm a multiple of 4 the
// four are one Philox block; otherwise they may straddle blocks and members, and a block is evaluated whenever (member,
// block) changes along the four -- at most four times (npm = 1).  Elements at and past `live` are left 0.
__device__ __forceinline__ f32x4 member_normal4(uint64_t seed, uint32_t first_member, long long npm, uint64_t q0, long long i,
                                                int live) {
  long long m = i / npm, e = i - m * npm;
  if ((npm & 3) == 0) return normal4(seed, first_member + (uint32_t)m, q0 + (uint64_t)(e >> 2));
  f32x4 r = {0.f, 0.f, 0.f, 0.f}, z = r;
  long long have_m = -1, have_b = -1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < live) {
      if (m != have_m || (e >> 2) != have_b) {
        z = normal4(seed, first_member + (uint32_t)m, q0 + (uint64_t)(e >> 2));
        have_m = m;
        have_b = e >> 2;
      }
      const int lane = (int)(e & 3);
      r[k] = lane == 0 ? z[0] : lane == 1 ? z[1] : lane == 2 ? z[2] : z[3];
      if (++e == npm) {
        e = 0;
        ++m;
      }
    }
  }
  return r;
}

}  // namespace philox
}  // namespace dlwp
