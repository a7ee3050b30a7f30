// Table of the one-input-channel lifting MLP of the fused FNO step kernel (lift_from_table, fno_device.hpp; DESIGN.md
// section 4.6): builder, host evaluation, guard.  Host code only -- the table's layout constants and lift_tab_locate are
// the device's own, taken from fno_device.hpp.
#include "fno_device.hpp"

using namespace dlwp;
using namespace dlwp::fno;

namespace {
constexpr double kLiftTabBound = 1.0 / 4194304.0;   // 2^-22: the operand precision the f16x3 form documents and accepts

struct LiftFn {   // lift(x) and its first two derivatives, fp64 (weights as given, fp32)
  const float *w1, *b1, *w2, *b2;
  int hid;
  mutable std::vector<double> g0, g1, g2;
  void operator()(double x, double* f, double* d1, double* d2) const {
    g0.resize(hid); g1.resize(hid); g2.resize(hid);
    for (int c = 0; c < hid; ++c) {
      const double w = w1[c], z = w * x + (double)b1[c];
      const double cdf = 0.5 * std::erfc(-z * 0.70710678118654752440);          // no cancellation in the lower tail
      const double pdf = 0.39894228040143267794 * std::exp(-0.5 * z * z);
      g0[c] = z * cdf;                           // gelu
      g1[c] = (cdf + z * pdf) * w;               // d/dx
      g2[c] = (2.0 - z * z) * pdf * w * w;       // d2/dx2
    }
    for (int o = 0; o < kC; ++o) {
      const float* wr = w2 + (size_t)o * hid;
      double s0 = 0.0, s1 = 0.0, s2 = 0.0;
      for (int c = 0; c < hid; ++c) {
        const double w = wr[c];
        s0 += w * g0[c];
        if (d1) { s1 += w * g1[c]; s2 += w * g2[c]; }
      }
      f[o] = (double)b2[o] + s0;
      if (d1) { d1[o] = s1; d2[o] = s2; }
    }
  }
};

// The table at x, with the device's arithmetic (lift_tab_locate + fp32 fmaf Horner); false outside the domain.
bool lift_table_eval1(const float* tab, int range, int log2_inv_h, float x, float* out, float* v_out, int* idx_out) {
  if (!(std::fabs(x) < (float)range)) return false;
  float v;
  const int idx = lift_tab_locate(x, range << log2_inv_h, (float)(1 << log2_inv_h), v);
  const float* c = tab + (size_t)idx * kLiftTabStride;
  for (int o = 0; o < kC; ++o) {
    float acc = c[(kLiftTabCoefs - 1) * kC + o];
    for (int k = kLiftTabCoefs - 2; k >= 0; --k) acc = std::fmaf(acc, v, c[k * kC + o]);
    out[o] = acc;
  }
  if (v_out) *v_out = v;
  if (idx_out) *idx_out = idx;
  return true;
}

// Fills tab [2 range 2^log2_inv_h][6][32] and returns the guard's figure: the largest ||p(x) - lift(x)||_2 / ||lift(x)||_2 over four
// interior points of every interval and, in the two intervals touching zero, v = 2^-k, k = 1..20 (points whose ||lift|| is
// below 1e-30 count with their absolute error over the largest ||lift|| seen).  NaN if anything is not finite.
double lift_table_fill(const LiftFn& fn, int range, int log2_inv_h, float* tab) {
  const int n_side = range << log2_inv_h, n = 2 * n_side;
  const double h = std::ldexp(1.0, -log2_inv_h);
  std::vector<double> F((size_t)(n + 1) * kC), D(F.size()), E(F.size());
  double fmax = 0.0;
  for (int k = 0; k <= n; ++k) {
    double* f = &F[(size_t)k * kC];
    fn((k - n_side) * h, f, &D[(size_t)k * kC], &E[(size_t)k * kC]);
    double nn = 0.0;
    for (int o = 0; o < kC; ++o) nn += f[o] * f[o];
    fmax = std::fmax(fmax, std::sqrt(nn));
  }
  for (int t = 0; t < n; ++t) {
    // anchor = the end nearer zero; v runs from it towards the far end, so odd derivatives change sign for x < 0
    const bool neg = t < n_side;
    const int a = neg ? t + 1 : t, b = neg ? t : t + 1;
    const double sg = neg ? -h : h;
    for (int o = 0; o < kC; ++o) {
      const double f0 = F[(size_t)a * kC + o], d0 = sg * D[(size_t)a * kC + o], e0 = h * h * E[(size_t)a * kC + o];
      const double f1 = F[(size_t)b * kC + o], d1 = sg * D[(size_t)b * kC + o], e1 = h * h * E[(size_t)b * kC + o];
      const double c0 = f0, c1 = d0, c2 = 0.5 * e0;
      const double ra = f1 - c0 - c1 - c2, rb = d1 - c1 - 2.0 * c2, rc = e1 - 2.0 * c2;
      const double co[kLiftTabCoefs] = {c0, c1, c2, 10.0 * ra - 4.0 * rb + 0.5 * rc, -15.0 * ra + 7.0 * rb - rc,
                                        6.0 * ra - 3.0 * rb + 0.5 * rc};
      for (int k = 0; k < kLiftTabCoefs; ++k) tab[((size_t)t * kLiftTabCoefs + k) * kC + o] = (float)co[k];
    }
  }
  double worst = 0.0;
  bool finite = std::isfinite(fmax);
  double want[kC];
  float got[kC];
  auto probe = [&](float x) {
    if (!lift_table_eval1(tab, range, log2_inv_h, x, got, nullptr, nullptr)) { finite = false; return; }
    fn((double)x, want, nullptr, nullptr);
    double en = 0.0, fnorm = 0.0;
    for (int o = 0; o < kC; ++o) {
      const double e = (double)got[o] - want[o];
      en += e * e;
      fnorm += want[o] * want[o];
    }
    en = std::sqrt(en); fnorm = std::sqrt(fnorm);
    const double rel = fnorm < 1e-30 ? (fmax > 0.0 ? en / fmax : en) : en / fnorm;
    if (!std::isfinite(rel)) finite = false;
    worst = std::fmax(worst, rel);
  };
  for (int t = 0; t < n; ++t) {
    const bool neg = t < n_side;
    const double anchor = ((neg ? t + 1 : t) - n_side) * h;
    for (int m = 0; m < 4; ++m) probe((float)(anchor + (neg ? -h : h) * (2 * m + 1) / 8.0));
  }
  for (int k = 1; k <= 20; ++k) {
    probe((float)std::ldexp(h, -k));
    probe((float)-std::ldexp(h, -k));
  }
  return finite ? worst : std::nan("");
}
}  // namespace

extern "C" int32_t dlwp_fno2d_lift_table_build(const float* lift_w1, const float* lift_b1, const float* lift_w2,
                                               const float* lift_b2, int32_t lifting, int32_t range, int32_t log2_inv_h,
                                               float* table, size_t table_floats, double* guard_err, int32_t* accepted) {
  DLWP_REQUIRE(lift_w1 && lift_b1 && lift_w2 && lift_b2 && table, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(lifting >= 1 && range >= 1 && range <= 1024 && log2_inv_h >= 0 && log2_inv_h <= 8, DLWP_ERR_INVALID_ARGUMENT,
               "need lifting >= 1, range in [1, 1024], log2_inv_h in [0, 8] (got %d, %d, %d)", lifting, range, log2_inv_h);
  const size_t need = (size_t)2 * ((size_t)range << log2_inv_h) * kLiftTabStride;
  DLWP_REQUIRE(table_floats >= need, DLWP_ERR_INVALID_ARGUMENT, "table holds %zu floats, %zu needed", table_floats, need);
  const LiftFn fn{lift_w1, lift_b1, lift_w2, lift_b2, lifting, {}, {}, {}};
  const double err = lift_table_fill(fn, range, log2_inv_h, table);
  if (guard_err) *guard_err = err;
  if (accepted) *accepted = err <= kLiftTabBound ? 1 : 0;   // NaN fails
  return DLWP_OK;
}

extern "C" int32_t dlwp_fno2d_lift_table_eval_host(const float* table, int32_t range, int32_t log2_inv_h, const float* x,
                                                   int64_t n, float* out, float* v_out, int32_t* interval_out) {
  DLWP_REQUIRE(table && x && out && n >= 0, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(range >= 1 && range <= 1024 && log2_inv_h >= 0 && log2_inv_h <= 8, DLWP_ERR_INVALID_ARGUMENT,
               "need range in [1, 1024], log2_inv_h in [0, 8] (got %d, %d)", range, log2_inv_h);
  for (int64_t i = 0; i < n; ++i) {
    float v = std::nanf("");
    int idx = -1;
    if (!lift_table_eval1(table, range, log2_inv_h, x[i], out + i * kC, &v, &idx))   // outside the domain: the kernel evaluates the MLP
      for (int o = 0; o < kC; ++o) out[i * kC + o] = std::nanf("");
    if (v_out) v_out[i] = v;
    if (interval_out) interval_out[i] = idx;
  }
  return DLWP_OK;
}
