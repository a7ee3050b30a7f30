// The padded, pre-activated, two-segment input load of the 3x3 convolution family: one element of
// P(act_pre(cat([x0, x1], 1))) at (sample b, channel c, row ih, column iw), ih in [-1, H], iw in [-1, W].  Shared by the direct
// forward (conv.hip: conv3x3_cyl_kernel) and the weight gradient (conv_wgrad.hip: PaddedLoad), so both read the same padded tensor.
//   P = CylinderPad(1) when p.hpx is null: longitude wraps, latitude pads zeros (utils/utils.py:11-26);
//   P = HEALPixPadding(1) through the ring table otherwise (utils/healpix.py:316-368).
// `Src` is any parameter block with the fields x0, c0, x1, c1, H, W, pre_act, hpx of conv::Params.
// The load comes in three steps, so that a kernel that reads many channels at one position can do the first once and keep
// the loads of the second in flight together: locate_padded (which cells of the unpadded tensor a padded position reads:
// channel-independent), fetch_padded (the raw values of one channel), finish_padded_act (pre-activation and corner mean).
// load_padded_act is the three in a row.
#pragma once

#include "act_common.hpp"

namespace dlwp {
namespace conv {

// the cells a padded position reads: n = 0 none (a padding zero), 1 one cell, 2 the mean of two (a synthesised HEALPix
// corner); a cell is (sample index sa, pixel pa inside the sample's [H][W] plane)
struct PadSource {
  int n, sa, pa, sb, pb;
};

template <class Src>
__device__ __forceinline__ PadSource locate_padded(const Src& p, int b, int ih, int iw) {
  PadSource s = {0, 0, 0, 0, 0};
  if (p.hpx) {
    if (ih >= -1 && ih <= p.H && iw >= -1 && iw <= p.W) {
      if (ih >= 0 && ih < p.H && iw >= 0 && iw < p.W) {
        s.n = 1; s.sa = b; s.pa = ih * p.W + iw;
      } else {
        const int HW = p.H * p.W;
        const int face = b % 12, s0 = b - face;
        const int2 e = p.hpx[(long long)face * (p.H + 2) * (p.W + 2) + (ih + 1) * (p.W + 2) + (iw + 1)];
        const int fa = e.x / HW;
        s.n = 1; s.sa = s0 + fa; s.pa = e.x - fa * HW;
        if (e.y >= 0) {
          const int fb = e.y / HW;
          s.n = 2; s.sb = s0 + fb; s.pb = e.y - fb * HW;
        }
      }
    }
  } else if (ih >= 0 && ih < p.H && iw >= -1 && iw <= p.W) {
    iw = iw < 0 ? iw + p.W : (iw >= p.W ? iw - p.W : iw);   // circular longitude
    s.n = 1; s.sa = b; s.pa = ih * p.W + iw;
  }
  return s;
}

// raw values of channel c at the located cells (0 where there is none, or c is past the last channel)
template <class Src>
__device__ __forceinline__ void fetch_padded(const Src& p, const PadSource& s, int c, float& v, float& v2) {
  v = 0.f;
  v2 = 0.f;
  if (s.n && c < p.c0 + p.c1) {
    const long long HW = (long long)p.H * p.W;
    const bool seg0 = c < p.c0;
    const float* base = seg0 ? p.x0 : p.x1;
    const int cs = seg0 ? p.c0 : p.c1, cl = seg0 ? c : c - p.c0;
    v = base[((long long)s.sa * cs + cl) * HW + s.pa];
    if (s.n == 2) v2 = base[((long long)s.sb * cs + cl) * HW + s.pb];
  }
}

template <class Src>
__device__ __forceinline__ float finish_padded_act(const Src& p, const PadSource& s, float v, float v2) {
  using actc::apply_act;
  if (s.n == 2) {
    // a synthesised corner is the mean of two cells of the ACTIVATED tensor (the reference pads after the activation,
    // unet.py:886-887): activate each source, then average
    if (p.pre_act) return 0.5f * apply_act(v, p.pre_act) + 0.5f * apply_act(v2, p.pre_act);
    return 0.5f * v + 0.5f * v2;
  }
  return p.pre_act ? apply_act(v, p.pre_act) : v;   // padding zeros stay zero (act(0) = 0)
}

template <class Src>
__device__ __forceinline__ float load_padded_act(const Src& p, int b, int c, int ih, int iw) {
  const PadSource s = locate_padded(p, b, ih, iw);
  float v, v2;
  fetch_padded(p, s, c, v, v2);
  return finish_padded_act(p, s, v, v2);
}

}  // namespace conv
}  // namespace dlwp
