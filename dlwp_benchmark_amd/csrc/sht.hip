// Real spherical harmonic transforms and the Driscoll-Healy channel mix of the SFNO backbone (models/sfno.py).  The reference
// reaches them through torch_harmonics (models/fno/fno.py:183-200: RealSHT / InverseRealSHT, norm "ortho", Condon-Shortley
// phase); that library is not part of the reference tree, so the conventions are restated in dlwp_benchmark_amd/sphere.py and
// pinned by mathematics.  Three kernels:
//
//   sht_kernel      x [planes, nlat, nlon] -> c [planes, lmax, mmax] complex.  A workgroup takes kPlanes planes and a tile of
//                   zonal wavenumbers m: rows of x go through LDS in chunks, a thread owns (row k, m) and forms the real DFT
//                   X[k][m] = (2 pi / nlon) sum_j x[k][j] tw[(j m) mod nlon] for its planes from the twiddle TABLE in LDS (any even
//                   nlon, no transcendental), X stays in LDS; then a thread owns (l, m) and contracts over latitude with the
//                   table wleg[k][l][m] -- one table load feeds kPlanes complex FMAs, the lanes of a wave read consecutive m.
//                   l < m is written as zero and costs no loop.  At 32 x 64 one m tile holds every m: x is read once, the
//                   spectrum written once, nothing else touches memory but the 128 KB table, which lives in L2.
//   isht_kernel     the two stages the other way round: a workgroup takes kPlanes planes and a tile of rows; per m tile the
//                   coefficients go to LDS (l >= m only: the other triangle is never read), a thread owns (k, m) and sums over
//                   l >= m; the Hermitian factor (1 for m = 0 and m = nlon / 2, whose imaginary parts are dropped, else 2) is
//                   applied where X is stored; then a thread owns (k, j) and sums over m -- irfft(n = nlon, norm = "forward").
//   sph_mix_kernel  c_out[b][o][l][m] = sum_i c_in[b][i][l][m] w[i][o][l]: per degree l a complex GEMM with rows (b, m <= l),
//                   written as a real GEMM of depth 2 cin on v_mfma_f32_16x16x4_f32 (exact fp32 products and sums, as
//                   afno.hip): a lane's (re, im) pair of c_in feeds two k-steps, against (wr, wi) for the imaginary and
//                   (wr, -wi) for the real output columns.  See the kernel for the tiling.
//
// and their backwards: each transform's adjoint is the OTHER transform's kernel over the same table
// (TableStrides / ColumnFactor below), the input gradient of the mix is sph_mix_kernel over the conjugate-transposed weight, and
//   sph_mix_wgrad_kernel  gw[i][o][l] = sum_b sum_{m <= l} conj(c_in[b][i][l][m]) g[b][o][l][m]: per degree a complex GEMM with
//                   M = cin, N = cout, K = batch * rows_l on the same matrix instruction.  See the kernel.
//
// Every sum runs in a fixed order in one thread (or one accumulator chain of the matrix pipe): no atomics, the same bits twice.
// The two stages of sht_kernel are device functions of sht_stages.hpp, which sph_power.hip (power spectra without the
// coefficients ever reaching memory) runs as well.
#include <algorithm>

#include "sht_stages.hpp"

namespace dlwp {
namespace sht {

constexpr int kMaxPlanes = 4;                // planes of a workgroup, which share every table load: 4, 2 or 1 (chosen per shape in dlwp_sht_f32)
// kThreads, kLdsBudget, TableStrides / ColumnFactor, the two stages of the forward transform, fit_tiles and check_transform:
// sht_stages.hpp (sph_power.hip runs the same two stages).

// ---- sht, and the adjoint of isht (x: the cotangent of the field, wleg: the table `leg`) ------------------------------------
// LDS: tw [nlon] float2 | X [kPlanes][nlat][mt] float2 | xs [kPlanes][rt][nlon] float
template <int kPlanes>
__global__ __launch_bounds__(kThreads) void sht_kernel(const float* __restrict__ x, const float* __restrict__ wleg,
                                                       const float2* __restrict__ tw, float2* __restrict__ coeffs,
                                                       long long planes, int nlat, int nlon, int lmax, int mmax, int mt, int rt,
                                                       int mtiles, TableStrides ts, ColumnFactor cf) {
  extern __shared__ __align__(16) unsigned char smem[];
  float2* tws = reinterpret_cast<float2*>(smem);
  float2* Xs = tws + nlon;
  float* xs = reinterpret_cast<float*>(Xs + (size_t)kPlanes * nlat * mt);
  const int tid = threadIdx.x;
  const int m0 = (int)(blockIdx.x % mtiles) * mt;
  const long long p0 = (long long)(blockIdx.x / mtiles) * kPlanes;
  const int mn = min(mt, mmax - m0);
  const int np = (int)min((long long)kPlanes, planes - p0);
  for (int t = tid; t < nlon; t += kThreads) tws[t] = tw[t];
  for (int k0 = 0; k0 < nlat; k0 += rt) {
    const int rn = min(rt, nlat - k0);
    __syncthreads();          // the chunk before has been read (first pass: nothing to wait for)
#pragma unroll
    for (int p = 0; p < kPlanes; ++p) {
      const float* src = x + ((p0 + p) * nlat + k0) * (long long)nlon;      // only dereferenced for p < np
      for (int e = tid; e < rn * nlon; e += kThreads) xs[p * rt * nlon + e] = p < np ? src[e] : 0.f;
    }
    __syncthreads();
    dft_rows<kPlanes>(xs, tws, Xs, tid, k0, rn, m0, mn, nlat, nlon, mt, rt, cf);
  }
  __syncthreads();
  for (int it = tid; it < lmax * mn; it += kThreads) {
    const int l = it / mn, mm = it - l * mn, m = m0 + mm;
    float ar[kPlanes], ai[kPlanes];
    legendre_column<kPlanes>(Xs, wleg, ts, l, m, mm, nlat, mt, ar, ai);
#pragma unroll
    for (int p = 0; p < kPlanes; ++p)
      if (p < np) coeffs[((p0 + p) * lmax + l) * (long long)mmax + m] = float2{ar[p], ai[p]};
  }
}

// ---- isht, and the adjoint of sht (coeffs: the cotangent of the spectrum, leg: the table `wleg`) ----------------------------
// LDS: tw [nlon] float2 | cs [kPlanes][lmax][mt] float2 | X [kPlanes][kt][mmax] float2
template <int kPlanes>
__global__ __launch_bounds__(kThreads) void isht_kernel(const float2* __restrict__ coeffs, const float* __restrict__ leg,
                                                        const float2* __restrict__ tw, float* __restrict__ y, long long planes,
                                                        int nlat, int nlon, int lmax, int mmax, int mt, int kt, int ktiles,
                                                        TableStrides ts, ColumnFactor cf) {
  extern __shared__ __align__(16) unsigned char smem[];
  float2* tws = reinterpret_cast<float2*>(smem);
  float2* cs = tws + nlon;
  float2* Xs = cs + (size_t)kPlanes * lmax * mt;
  const int tid = threadIdx.x;
  const int k0 = (int)(blockIdx.x % ktiles) * kt;
  const long long p0 = (long long)(blockIdx.x / ktiles) * kPlanes;
  const int kn = min(kt, nlat - k0);
  const int np = (int)min((long long)kPlanes, planes - p0);
  for (int t = tid; t < nlon; t += kThreads) tws[t] = tw[t];
  for (int m0 = 0; m0 < mmax; m0 += mt) {
    const int mn = min(mt, mmax - m0);
    __syncthreads();          // the tile before has been read
    for (int e = tid; e < kPlanes * lmax * mn; e += kThreads) {
      const int p = e / (lmax * mn), r = e - p * (lmax * mn), l = r / mn, mm = r - l * mn, m = m0 + mm;
      float2 v = float2{0.f, 0.f};
      if (p < np && l >= m) v = coeffs[((p0 + p) * lmax + l) * (long long)mmax + m];     // the l < m triangle is never read
      cs[(p * lmax + l) * mt + mm] = v;
    }
    __syncthreads();
    for (int it = tid; it < kn * mn; it += kThreads) {
      const int kk = it / mn, mm = it - kk * mn, m = m0 + mm;
      float ar[kPlanes], ai[kPlanes];
#pragma unroll
      for (int p = 0; p < kPlanes; ++p) ar[p] = ai[p] = 0.f;
      const float* lp = leg + (k0 + kk) * ts.row + m;
#pragma unroll 4
      for (int l = m; l < lmax; ++l) {
        const float w = lp[l * ts.degree];
#pragma unroll
        for (int p = 0; p < kPlanes; ++p) {
          const float2 v = cs[(p * lmax + l) * mt + mm];
          ar[p] = fmaf(w, v.x, ar[p]);
          ai[p] = fmaf(w, v.y, ai[p]);
        }
      }
      const bool self_conjugate = m == 0 || 2 * m == nlon;      // the columns irfft takes the real part of
      const float f = self_conjugate ? cf.self_conjugate : cf.other;
#pragma unroll
      for (int p = 0; p < kPlanes; ++p)
        Xs[(p * kt + kk) * mmax + m] = float2{f * ar[p], self_conjugate && cf.drop_imag ? 0.f : f * ai[p]};
    }
  }
  __syncthreads();
  for (int it = tid; it < kn * nlon; it += kThreads) {
    const int kk = it / nlon, j = it - kk * nlon;
    float acc[kPlanes];
#pragma unroll
    for (int p = 0; p < kPlanes; ++p) acc[p] = 0.f;
    const float2* xr = Xs + (size_t)kk * mmax;
    int idx = 0;              // (j m) mod nlon; j < nlon
#pragma unroll 4
    for (int m = 0; m < mmax; ++m) {
      const float2 w = tws[idx];
      idx += j;
      if (idx >= nlon) idx -= nlon;
#pragma unroll
      for (int p = 0; p < kPlanes; ++p) {
        const float2 v = xr[p * kt * mmax + m];
        acc[p] = fmaf(v.x, w.x, acc[p]);
        acc[p] = fmaf(v.y, w.y, acc[p]);
      }
    }
#pragma unroll
    for (int p = 0; p < kPlanes; ++p)
      if (p < np) y[((p0 + p) * nlat + k0 + kk) * (long long)nlon + j] = acc[p];
  }
}

// ---- channel mix -----------------------------------------------------------------------------------------------------------
// A workgroup takes one degree l, kMixOut output channels and kMixRows of the rows (b, m <= l), packed without gaps (row r is
// b = r / (l + 1), m = r % (l + 1): degree 0 has `batch` rows, not batch * 16), one 16-row tile per wave and four 16-column
// tiles of complex outputs per wave: eight accumulators.  The weights of kMixK input channels go through LDS (each is used by
// the four waves); a lane reads its c_in pair straight from global memory, where 16 consecutive m are 128 contiguous bytes.  Both
// are fetched one stage ahead into registers.
// The parameter layout [cin][cout][lmax] puts the lmax degrees of one (i, o) side by side, so a workgroup that reads it
// (kPacked false) uses 8 bytes of every 128-byte line it touches -- measured at 256 x 256 x 32, batch 16: 0.197 ms, slower than
// torch's batched GEMM.  The packed image [lmax][cin][cout] (sph_mix_pack_kernel; made once per weight version by ops.sph_mix)
// turns those into 512 contiguous bytes per wave and load.  The grid is ordered so that the workgroups that share weight lines
// run on one XCD at the same time and find them in its L2: blocks are dealt round-robin over the eight XCDs (a matter of speed
// only), so XCD x takes the units u = x, x + 8, ... of (output tile, degree group); with fewer than eight output tiles the
// degrees of one tile are split into groups (l = group, group + G, ...: the triangle's work stays balanced) so that all eight get
// work.
constexpr int kMixOut = 64;
constexpr int kMixK = 32;
constexpr int kMixRows = 64;
constexpr int kMixStride = 80;     // float2 per LDS row: k-groups 0 / 1 (and 2 / 3) of a ds_read_b64 fall on different bank halves

// The input gradient gc_in[b][i][l][m] = sum_o g[b][o][l][m] conj(w[i][o][l]) is the same GEMM over the conjugate-transposed
// weight: kWeight names where w[k][n] of degree l is found.
enum MixWeight {
  kMixParam = 0,              // the parameter [k][n][lmax]
  kMixPacked = 1,             // a degree-major image [lmax][k][n] (of the weight, or of its conjugate transpose)
  kMixParamAdjoint = 2        // the parameter [n][k][lmax], conjugated: the input gradient without a pack
};

template <int kWeight>
__global__ __launch_bounds__(kThreads) void sph_mix_kernel(const float2* __restrict__ cin, const float2* __restrict__ w,
                                                           float2* __restrict__ cout, int batch, int ci, int co, int lmax, int mmax,
                                                           int n_ot, int n_rb, int groups, int per_group) {
  __shared__ float2 Ws[kMixK * kMixStride];
  const int tid = threadIdx.x;
  int q = blockIdx.x >> 3;
  const int rb = q % n_rb;
  q /= n_rb;
  const int unit = (q / per_group) * 8 + (int)(blockIdx.x & 7);      // (output tile, degree group)
  const int ot = unit / groups;
  const int l = unit % groups + groups * (q % per_group);
  if (ot >= n_ot || l >= lmax) return;
  const int rows_l = min(l, mmax - 1) + 1;
  const int M = batch * rows_l;
  if (rb * kMixRows >= M) return;
  const int o0 = ot * kMixOut;
  const size_t plane = (size_t)lmax * mmax;
  if (rb == 0) {              // the entries above the diagonal of this degree and these outputs
    const int nz = mmax - rows_l, on = min(kMixOut, co - o0);
    for (int e = tid; e < batch * on * nz; e += kThreads) {
      const int mz = e % nz, t2 = e / nz, ol = t2 % on, b = t2 / on;
      cout[((size_t)b * co + o0 + ol) * plane + (size_t)l * mmax + rows_l + mz] = float2{0.f, 0.f};
    }
  }
  const int wave = tid >> 6, lane = tid & 63, g = lane >> 4, r16 = lane & 15;
  const int row = rb * kMixRows + wave * 16 + r16;
  const bool row_ok = row < M;
  const int rb_ = row_ok ? row / rows_l : 0, rm_ = row_ok ? row - rb_ * rows_l : 0;
  const float2* a_ptr = cin + (size_t)rb_ * ci * plane + (size_t)l * mmax + rm_;
  f32x4 accR[4], accI[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) accR[c] = accI[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int kWPer = kMixK * kMixOut / kThreads;     // 8 weights per thread and stage
  constexpr int kSteps = kMixK / 4;                     // 8 pairs of k-steps per stage
  float2 wreg[kWPer], areg[kSteps];
  auto fetch = [&](int i0) {
#pragma unroll
    for (int n = 0; n < kWPer; ++n) {
      const int e = tid + n * kThreads, i = i0 + (e >> 6), o = o0 + (e & 63);
      const size_t at = kWeight == kMixPacked ? ((size_t)l * ci + i) * co + o
                        : (kWeight == kMixParam ? ((size_t)i * co + o) * lmax + l : ((size_t)o * ci + i) * lmax + l);
      wreg[n] = (i < ci && o < co) ? w[at] : float2{0.f, 0.f};
      if (kWeight == kMixParamAdjoint) wreg[n].y = -wreg[n].y;
    }
#pragma unroll
    for (int t = 0; t < kSteps; ++t) {
      const int i = i0 + 4 * t + g;
      areg[t] = (row_ok && i < ci) ? a_ptr[(size_t)i * plane] : float2{0.f, 0.f};
    }
  };
  fetch(0);
  for (int i0 = 0; i0 < ci; i0 += kMixK) {
    __syncthreads();          // the stage before has been read
#pragma unroll
    for (int n = 0; n < kWPer; ++n) {
      const int e = tid + n * kThreads;
      Ws[(e >> 6) * kMixStride + (e & 63)] = wreg[n];
    }
    float2 a[kSteps];
#pragma unroll
    for (int t = 0; t < kSteps; ++t) a[t] = areg[t];
    __syncthreads();
    if (i0 + kMixK < ci) fetch(i0 + kMixK);
#pragma unroll
    for (int t = 0; t < kSteps; ++t) {
      const float are = a[t].x, aim = a[t].y, naim = -a[t].y;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float2 wv = Ws[(4 * t + g) * kMixStride + c * 16 + r16];
        accR[c] = mfma16x16x4(are, wv.x, accR[c]);
        accR[c] = mfma16x16x4(naim, wv.y, accR[c]);
        accI[c] = mfma16x16x4(are, wv.y, accI[c]);
        accI[c] = mfma16x16x4(aim, wv.x, accI[c]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int orow = rb * kMixRows + wave * 16 + 4 * g + r;
    if (orow >= M) continue;
    const int ob = orow / rows_l, om = orow - ob * rows_l;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int o = o0 + c * 16 + r16;
      if (o < co) cout[((size_t)ob * co + o) * plane + (size_t)l * mmax + om] = float2{accR[c][r], accI[c][r]};
    }
  }
}

// The 32 x 32 tile transpose behind every re-layout of a mix weight, through LDS so that both sides are coalesced:
//   in [rows][nmid][cols] -> out [cols][nmid][rows]  (complex; conj: conjugated on the way)
// weight [cin * cout][lmax] -> packed [lmax][cin * cout] is rows = cin * cout, nmid = 1, cols = lmax; its inverse (a transpose is
// its own inverse with the extents exchanged) rows = lmax, cols = cin * cout; the conjugate transpose [cin][cout][lmax] ->
// [lmax][cout][cin] of the input gradient rows = cin, nmid = cout, cols = lmax.
__global__ __launch_bounds__(kThreads) void sph_mix_pack_kernel(const float2* __restrict__ w, float2* __restrict__ packed, long long rows,
                                                                long long nmid, long long cols, long long rtiles, long long ctiles,
                                                                bool conj) {
  __shared__ float2 tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const long long c0 = (long long)(blockIdx.x % ctiles) * 32, q = blockIdx.x / ctiles;
  const long long r0 = (q % rtiles) * 32, mid = q / rtiles;
#pragma unroll
  for (int r = ty; r < 32; r += 8)
    if (r0 + r < rows && c0 + tx < cols) tile[r][tx] = w[((r0 + r) * nmid + mid) * cols + c0 + tx];
  __syncthreads();
#pragma unroll
  for (int r = ty; r < 32; r += 8)
    if (c0 + r < cols && r0 + tx < rows) {
      const float2 v = tile[tx][r];
      packed[((c0 + r) * nmid + mid) * rows + r0 + tx] = float2{v.x, conj ? -v.y : v.y};
    }
}

// ---- weight gradient of the channel mix ------------------------------------------------------------------------------------
// gw[i][o][l] = sum_b sum_{m < rows_l} conj(c_in[b][i][l][m]) g[b][o][l][m]: per degree a complex GEMM with M = cin, N = cout and
// K = batch * rows_l, on v_mfma_f32_16x16x4_f32 as the forward:
//   gw.re = sum c.re g.re + c.im g.im        gw.im = sum c.re g.im - c.im g.re
// A workgroup takes one degree and a kWgTile x kWgTile tile of (i, o); a wave 16 rows i and the four 16-column tiles of o, eight
// accumulators.  K runs over k = b * rows_l + m in ascending order in chunks of kWgK, every sum in one accumulator chain: no
// split-K, no atomics.  Both operands of one (b, channel, l) are a run of rows_l contiguous complex values: a chunk of them goes
// through LDS as [channel][k] (32 consecutive lanes load 32 consecutive k: whole runs, and contiguous 256 B of LDS), fetched one
// chunk ahead into registers.  Channels beyond cin / cout and k beyond K are ZERO in LDS, so the MFMA loop has no tail code;
// its trip count is the chunk's k-steps, uniform over the workgroup (degree 0 of batch 1 has K = 1: one step).
// LDS stride kWgStride = 34 float2: an MFMA operand read is ds_read_b64 at [16 r-lanes][k-group g], dword 68 r + 2 g, and the
// 32 lanes of a half-wave (g in {0, 1} or {2, 3}) fall on the 64 banks 4 r + 2 g (+ 1) once each; the staging writes are 16
// contiguous float2 per lane group.
// Degrees are dealt so that the round-robin of blocks over the eight XCDs stays balanced over the triangle: the tiles of one
// degree are consecutive blocks, and the degrees come in runs of sixteen, eight descending then the other eight ascending, so
// that with one tile per degree XCD x takes degrees 15 - x and x of a run.
// kDegreeMajor: gw is written [lmax][cin][cout] (16 lanes write 128 contiguous bytes; transposed back by sph_mix_pack_kernel);
// otherwise straight into the parameter layout [cin][cout][lmax], 8 bytes per 128-byte line.
constexpr int kWgTile = 64;
constexpr int kWgK = 32;
constexpr int kWgStride = 34;

template <bool kDegreeMajor>
__global__ __launch_bounds__(kThreads) void sph_mix_wgrad_kernel(const float2* __restrict__ cin, const float2* __restrict__ g,
                                                                 float2* __restrict__ gw, int batch, int ci, int co, int lmax,
                                                                 int mmax, int n_it, int n_ot) {
  __shared__ float2 As[kWgTile * kWgStride], Bs[kWgTile * kWgStride];
  const int tid = threadIdx.x;
  const int tiles = n_it * n_ot;
  const int pos = (int)(blockIdx.x / tiles), tile = (int)(blockIdx.x % tiles);
  const int run = pos >> 4, r = pos & 15;
  const int l = run * 16 + (r < 8 ? 15 - r : r - 8);
  if (l >= lmax) return;
  const int i0 = (tile / n_ot) * kWgTile, o0 = (tile % n_ot) * kWgTile;
  const int rows_l = min(l, mmax - 1) + 1;
  const int K = batch * rows_l;
  const size_t plane = (size_t)lmax * mmax;
  const int wave = tid >> 6, lane = tid & 63, grp = lane >> 4, r16 = lane & 15;
  constexpr int kPer = kWgTile * kWgK / kThreads;       // 8 values of each operand per thread and chunk
  const int kk = tid & (kWgK - 1), ch0 = tid >> 5;      // this thread's k of a chunk, and its first channel (then + 8, ...)
  f32x4 accR[4], accI[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) accR[c] = accI[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  float2 areg[kPer], breg[kPer];
  auto fetch = [&](int k0) {
    const int k = k0 + kk;
    const bool k_ok = k < K;
    const int b = k_ok ? k / rows_l : 0, m = k_ok ? k - b * rows_l : 0;
    const size_t at = (size_t)l * mmax + m;
#pragma unroll
    for (int n = 0; n < kPer; ++n) {
      const int i = i0 + ch0 + 8 * n, o = o0 + ch0 + 8 * n;
      areg[n] = (k_ok && i < ci) ? cin[((size_t)b * ci + i) * plane + at] : float2{0.f, 0.f};
      breg[n] = (k_ok && o < co) ? g[((size_t)b * co + o) * plane + at] : float2{0.f, 0.f};
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < K; k0 += kWgK) {
    __syncthreads();          // the chunk before has been read
#pragma unroll
    for (int n = 0; n < kPer; ++n) {
      As[(ch0 + 8 * n) * kWgStride + kk] = areg[n];
      Bs[(ch0 + 8 * n) * kWgStride + kk] = breg[n];
    }
    __syncthreads();
    if (k0 + kWgK < K) fetch(k0 + kWgK);
    const int steps = (min(kWgK, K - k0) + 3) >> 2;
    for (int t = 0; t < steps; ++t) {
      const float2 a = As[(wave * 16 + r16) * kWgStride + 4 * t + grp];
      const float nai = -a.y;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float2 bv = Bs[(c * 16 + r16) * kWgStride + 4 * t + grp];
        accR[c] = mfma16x16x4(a.x, bv.x, accR[c]);
        accR[c] = mfma16x16x4(a.y, bv.y, accR[c]);
        accI[c] = mfma16x16x4(a.x, bv.y, accI[c]);
        accI[c] = mfma16x16x4(nai, bv.x, accI[c]);
      }
    }
  }
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int i = i0 + wave * 16 + 4 * grp + rr;
    if (i >= ci) continue;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int o = o0 + c * 16 + r16;
      if (o < co) gw[kDegreeMajor ? ((size_t)l * ci + i) * co + o : ((size_t)i * co + o) * lmax + l] = float2{accR[c][rr], accI[c][rr]};
    }
  }
}

}  // namespace sht
}  // namespace dlwp

using namespace dlwp;

// sht_kernel: fields -> spectra.  adjoint false: dlwp_sht_f32 over wleg; true: the backward of isht over leg
static int32_t sht_launch(bool adjoint, const float* x_dev, const float* wleg_dev, const float* tw_dev, float* coeffs_dev,
                          int64_t planes, int32_t nlat, int32_t nlon, int32_t lmax, int32_t mmax, void* stream) {
  if (int32_t rc = sht::check_transform(x_dev, wleg_dev, tw_dev, coeffs_dev, planes, nlat, nlon, lmax, mmax)) return rc;
  DLWP_REQUIRE((reinterpret_cast<uintptr_t>(tw_dev) | reinterpret_cast<uintptr_t>(coeffs_dev)) % 8 == 0, DLWP_ERR_INVALID_ARGUMENT,
               "tw_dev and coeffs_dev must be 8-byte aligned");
  // the most planes per workgroup (4, 2, 1) whose tiles still give every thread an item of the DFT stage
  int np = sht::kMaxPlanes, mt = 0, rt = 0;
  size_t bytes = 0;
  for (;; np /= 2) {
    mt = mmax, rt = nlat;
    const bool fits = sht::fit_tiles((size_t)nlon * 8, (size_t)np * nlat * 8, mt, (size_t)np * nlon * 4, rt, bytes);
    if (fits && ((long long)mt * rt >= sht::kThreads || (mt == mmax && rt == nlat) || np == 1)) break;
    DLWP_REQUIRE(np > 1, DLWP_ERR_UNSUPPORTED, "no tiling of %d x %d fits the LDS budget", nlat, nlon);
  }
  const long long mtiles = (mmax + mt - 1) / mt, groups = (planes + np - 1) / np;
  DLWP_REQUIRE(groups <= 0x7fffffffLL / mtiles, DLWP_ERR_UNSUPPORTED, "grid too large: %lld planes", (long long)planes);
  const float scale = (float)(2.0 * 3.14159265358979323846 / (double)nlon);
  const sht::TableStrides ts = adjoint ? sht::TableStrides{(size_t)mmax, (size_t)nlat * mmax}
                                       : sht::TableStrides{(size_t)lmax * mmax, (size_t)mmax};
  const sht::ColumnFactor cf = adjoint ? sht::ColumnFactor{1.f, 2.f, true} : sht::ColumnFactor{scale, scale, false};
  auto kernel = np == 4 ? sht::sht_kernel<4> : (np == 2 ? sht::sht_kernel<2> : sht::sht_kernel<1>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)(groups * mtiles)), dim3(sht::kThreads), bytes,
                     reinterpret_cast<hipStream_t>(stream), x_dev, wleg_dev, reinterpret_cast<const float2*>(tw_dev),
                     reinterpret_cast<float2*>(coeffs_dev), (long long)planes, nlat, nlon, lmax, mmax, mt, rt, (int)mtiles, ts, cf);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

// isht_kernel: spectra -> fields.  adjoint false: dlwp_isht_f32 over leg; true: the backward of sht over wleg
static int32_t isht_launch(bool adjoint, const float* coeffs_dev, const float* leg_dev, const float* tw_dev, float* y_dev,
                           int64_t planes, int32_t nlat, int32_t nlon, int32_t lmax, int32_t mmax, void* stream) {
  if (int32_t rc = sht::check_transform(coeffs_dev, leg_dev, tw_dev, y_dev, planes, nlat, nlon, lmax, mmax)) return rc;
  DLWP_REQUIRE((reinterpret_cast<uintptr_t>(tw_dev) | reinterpret_cast<uintptr_t>(coeffs_dev)) % 8 == 0, DLWP_ERR_INVALID_ARGUMENT,
               "tw_dev and coeffs_dev must be 8-byte aligned");
  int np = sht::kMaxPlanes, mt = 0, kt = 0;
  size_t bytes = 0;
  for (;; np /= 2) {          // as in dlwp_sht_f32
    mt = mmax, kt = nlat;
    const bool fits = sht::fit_tiles((size_t)nlon * 8, (size_t)np * lmax * 8, mt, (size_t)np * mmax * 8, kt, bytes);
    if (fits && ((long long)mt * kt >= sht::kThreads || (mt == mmax && kt == nlat) || np == 1)) break;
    DLWP_REQUIRE(np > 1, DLWP_ERR_UNSUPPORTED, "no tiling of %d x %d fits the LDS budget", nlat, nlon);
  }
  const long long ktiles = (nlat + kt - 1) / kt, groups = (planes + np - 1) / np;
  DLWP_REQUIRE(groups <= 0x7fffffffLL / ktiles, DLWP_ERR_UNSUPPORTED, "grid too large: %lld planes", (long long)planes);
  const float scale = (float)(2.0 * 3.14159265358979323846 / (double)nlon);
  const sht::TableStrides ts = adjoint ? sht::TableStrides{(size_t)lmax * mmax, (size_t)mmax}
                                       : sht::TableStrides{(size_t)mmax, (size_t)nlat * mmax};
  const sht::ColumnFactor cf = adjoint ? sht::ColumnFactor{scale, scale, false} : sht::ColumnFactor{1.f, 2.f, true};
  auto kernel = np == 4 ? sht::isht_kernel<4> : (np == 2 ? sht::isht_kernel<2> : sht::isht_kernel<1>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)(groups * ktiles)), dim3(sht::kThreads), bytes,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const float2*>(coeffs_dev), leg_dev,
                     reinterpret_cast<const float2*>(tw_dev), y_dev, (long long)planes, nlat, nlon, lmax, mmax, mt, kt, (int)ktiles, ts, cf);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" int32_t dlwp_sht_f32(const float* x_dev, const float* wleg_dev, const float* tw_dev, float* coeffs_dev, int64_t planes,
                                int32_t nlat, int32_t nlon, int32_t lmax, int32_t mmax, void* stream) {
  return sht_launch(false, x_dev, wleg_dev, tw_dev, coeffs_dev, planes, nlat, nlon, lmax, mmax, stream);
}

extern "C" int32_t dlwp_isht_f32(const float* coeffs_dev, const float* leg_dev, const float* tw_dev, float* y_dev, int64_t planes,
                                 int32_t nlat, int32_t nlon, int32_t lmax, int32_t mmax, void* stream) {
  return isht_launch(false, coeffs_dev, leg_dev, tw_dev, y_dev, planes, nlat, nlon, lmax, mmax, stream);
}

extern "C" int32_t dlwp_sht_bwd_f32(const float* g_dev, const float* wleg_dev, const float* tw_dev, float* gx_dev, int64_t planes,
                                    int32_t nlat, int32_t nlon, int32_t lmax, int32_t mmax, void* stream) {
  return isht_launch(true, g_dev, wleg_dev, tw_dev, gx_dev, planes, nlat, nlon, lmax, mmax, stream);
}

extern "C" int32_t dlwp_isht_bwd_f32(const float* gy_dev, const float* leg_dev, const float* tw_dev, float* gc_dev, int64_t planes,
                                     int32_t nlat, int32_t nlon, int32_t lmax, int32_t mmax, void* stream) {
  return sht_launch(true, gy_dev, leg_dev, tw_dev, gc_dev, planes, nlat, nlon, lmax, mmax, stream);
}

static int32_t check_mix(const void* a, const void* b, const void* c, int32_t batch, int32_t cin, int32_t cout, int32_t lmax,
                         int32_t mmax) {
  DLWP_REQUIRE(a && b && c, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(batch >= 1 && cin >= 1 && cout >= 1, DLWP_ERR_INVALID_ARGUMENT, "batch, cin and cout must be at least 1");
  DLWP_REQUIRE(lmax >= 1 && lmax <= 1024 && mmax >= 1 && mmax <= 1024 && (long long)batch * mmax < (1LL << 24),
               DLWP_ERR_UNSUPPORTED, "sph_mix outside the envelope: lmax %d, mmax %d (1..1024), batch %d * mmax < 2^24", lmax, mmax,
               batch);
  DLWP_REQUIRE((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) % 8 == 0,
               DLWP_ERR_INVALID_ARGUMENT, "pointers must be 8-byte aligned");
  return DLWP_OK;
}

// c_out [batch][cout] = c_in [batch][cin] times the [cin][cout] matrix of each degree, found in weight_dev as `mode` says
static int32_t sph_mix_launch(sht::MixWeight mode, const float* c_in_dev, const float* weight_dev, float* c_out_dev, int32_t batch,
                              int32_t cin, int32_t cout, int32_t lmax, int32_t mmax, void* stream) {
  if (int32_t rc = check_mix(c_in_dev, weight_dev, c_out_dev, batch, cin, cout, lmax, mmax)) return rc;
  const long long n_ot = (cout + sht::kMixOut - 1) / sht::kMixOut;
  const long long n_rb = ((long long)batch * std::min(lmax, mmax) + sht::kMixRows - 1) / sht::kMixRows;
  const long long groups = n_ot >= 8 ? 1 : std::min<long long>((8 + n_ot - 1) / n_ot, lmax);     // degree groups per output tile
  const long long per_group = (lmax + groups - 1) / groups;
  const long long blocks = 8 * n_rb * per_group * ((n_ot * groups + 7) / 8);
  DLWP_REQUIRE(blocks <= 0x7fffffffLL && (long long)batch * cout * mmax < (1LL << 31), DLWP_ERR_UNSUPPORTED,
               "grid too large: batch %d, cout %d, lmax %d", batch, cout, lmax);
  auto kernel = mode == sht::kMixPacked ? sht::sph_mix_kernel<sht::kMixPacked>
                                        : (mode == sht::kMixParam ? sht::sph_mix_kernel<sht::kMixParam>
                                                                  : sht::sph_mix_kernel<sht::kMixParamAdjoint>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(sht::kThreads), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const float2*>(c_in_dev), reinterpret_cast<const float2*>(weight_dev),
                     reinterpret_cast<float2*>(c_out_dev), batch, cin, cout, lmax, mmax, (int)n_ot, (int)n_rb, (int)groups,
                     (int)per_group);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

// in [rows][nmid][cols] -> out [cols][nmid][rows] (complex), see sph_mix_pack_kernel
static int32_t sph_mix_transpose(const float* in_dev, float* out_dev, long long rows, long long nmid, long long cols, bool conj,
                                 int32_t cin, int32_t cout, int32_t lmax, void* stream) {
  DLWP_REQUIRE(in_dev && out_dev, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(cin >= 1 && cout >= 1 && lmax >= 1 && lmax <= 1024, DLWP_ERR_INVALID_ARGUMENT, "cin, cout >= 1 and 1 <= lmax <= 1024");
  DLWP_REQUIRE((reinterpret_cast<uintptr_t>(in_dev) | reinterpret_cast<uintptr_t>(out_dev)) % 8 == 0,
               DLWP_ERR_INVALID_ARGUMENT, "pointers must be 8-byte aligned");
  const long long rtiles = (rows + 31) / 32, ctiles = (cols + 31) / 32;
  DLWP_REQUIRE(rtiles <= 0x7fffffffLL / ctiles / nmid, DLWP_ERR_UNSUPPORTED, "grid too large: cin %d, cout %d", cin, cout);
  hipLaunchKernelGGL(sht::sph_mix_pack_kernel, dim3((unsigned)(rtiles * ctiles * nmid)), dim3(sht::kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const float2*>(in_dev),
                     reinterpret_cast<float2*>(out_dev), rows, nmid, cols, rtiles, ctiles, conj);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

static int32_t sph_mix_wgrad_launch(bool degree_major, const float* c_in_dev, const float* g_dev, float* gw_dev, int32_t batch,
                                    int32_t cin, int32_t cout, int32_t lmax, int32_t mmax, void* stream) {
  if (int32_t rc = check_mix(c_in_dev, g_dev, gw_dev, batch, cin, cout, lmax, mmax)) return rc;
  const long long n_it = (cin + sht::kWgTile - 1) / sht::kWgTile, n_ot = (cout + sht::kWgTile - 1) / sht::kWgTile;
  const long long runs = (lmax + 15) / 16;
  DLWP_REQUIRE(n_it * n_ot <= 0x7fffffffLL / (16 * runs) && (long long)batch * std::max(cin, cout) * mmax < (1LL << 31),
               DLWP_ERR_UNSUPPORTED, "grid too large: batch %d, cin %d, cout %d, lmax %d", batch, cin, cout, lmax);
  auto kernel = degree_major ? sht::sph_mix_wgrad_kernel<true> : sht::sph_mix_wgrad_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(16 * runs * n_it * n_ot)), dim3(sht::kThreads), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const float2*>(c_in_dev), reinterpret_cast<const float2*>(g_dev),
                     reinterpret_cast<float2*>(gw_dev), batch, cin, cout, lmax, mmax, (int)n_it, (int)n_ot);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}

extern "C" int32_t dlwp_sph_mix_f32(const float* c_in_dev, const float* weight_dev, float* c_out_dev, int32_t batch, int32_t cin,
                                    int32_t cout, int32_t lmax, int32_t mmax, void* stream) {
  return sph_mix_launch(sht::kMixParam, c_in_dev, weight_dev, c_out_dev, batch, cin, cout, lmax, mmax, stream);
}

extern "C" int32_t dlwp_sph_mix_packed_f32(const float* c_in_dev, const float* packed_dev, float* c_out_dev, int32_t batch,
                                           int32_t cin, int32_t cout, int32_t lmax, int32_t mmax, void* stream) {
  return sph_mix_launch(sht::kMixPacked, c_in_dev, packed_dev, c_out_dev, batch, cin, cout, lmax, mmax, stream);
}

extern "C" int32_t dlwp_sph_mix_pack_f32(const float* weight_dev, float* packed_dev, int32_t cin, int32_t cout, int32_t lmax,
                                         void* stream) {
  return sph_mix_transpose(weight_dev, packed_dev, (long long)cin * cout, 1, lmax, false, cin, cout, lmax, stream);
}

extern "C" int32_t dlwp_sph_mix_unpack_f32(const float* packed_dev, float* weight_dev, int32_t cin, int32_t cout, int32_t lmax,
                                           void* stream) {
  return sph_mix_transpose(packed_dev, weight_dev, lmax, 1, (long long)cin * cout, false, cin, cout, lmax, stream);
}

extern "C" int32_t dlwp_sph_mix_pack_adjoint_f32(const float* weight_dev, float* packed_dev, int32_t cin, int32_t cout, int32_t lmax,
                                                 void* stream) {
  return sph_mix_transpose(weight_dev, packed_dev, cin, cout, lmax, true, cin, cout, lmax, stream);
}

// the mix the other way: the kernel's input channels are the forward's outputs
extern "C" int32_t dlwp_sph_mix_dgrad_f32(const float* g_dev, const float* weight_dev, float* gc_in_dev, int32_t batch, int32_t cin,
                                          int32_t cout, int32_t lmax, int32_t mmax, void* stream) {
  return sph_mix_launch(sht::kMixParamAdjoint, g_dev, weight_dev, gc_in_dev, batch, cout, cin, lmax, mmax, stream);
}

extern "C" int32_t dlwp_sph_mix_wgrad_f32(const float* c_in_dev, const float* g_dev, float* gw_dev, int32_t batch, int32_t cin,
                                          int32_t cout, int32_t lmax, int32_t mmax, void* stream) {
  return sph_mix_wgrad_launch(false, c_in_dev, g_dev, gw_dev, batch, cin, cout, lmax, mmax, stream);
}

extern "C" int32_t dlwp_sph_mix_wgrad_packed_f32(const float* c_in_dev, const float* g_dev, float* gw_packed_dev, int32_t batch,
                                                 int32_t cin, int32_t cout, int32_t lmax, int32_t mmax, void* stream) {
  return sph_mix_wgrad_launch(true, c_in_dev, g_dev, gw_packed_dev, batch, cin, cout, lmax, mmax, stream);
}
