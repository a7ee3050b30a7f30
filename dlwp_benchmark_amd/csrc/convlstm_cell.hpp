// The ConvLSTM cell update of one (sample, channel, pixel) element (reference models/convlstm/convlstm.py:96-109) and its
// derivative: the arithmetic convlstm_bwd.hip recomputes the forward with.  The expressions are those of
// convlstm_gates_kernel (conv.hip), operation for operation -- sigma as 1 / (1 + __expf(-x)), tanh as tanhf, the library
// builds with -ffp-contract=off -- so the recomputed c is the c the forward stored.
#pragma once

#include "common.hpp"

namespace dlwp {
namespace clstm {

__device__ __forceinline__ float sigmoid(float x) { return 1.f / (1.f + __expf(-x)); }

// what the forward evaluates on the way to (h, c): the three gate activations, tanh of the candidate, the new cell state
// and its tanh; h = so * tc
struct Cell {
  float si, sf, so, tn, c, tc;
};

__device__ __forceinline__ Cell cell_forward(float netin, float ig, float fg, float og, float c_prev) {
  Cell s;
  s.si = sigmoid(ig);
  s.sf = sigmoid(fg);
  s.so = sigmoid(og);
  s.tn = tanhf(netin);
  s.c = s.sf * c_prev + s.si * s.tn;
  s.tc = tanhf(s.c);
  return s;
}

// gradients with respect to the four pre-activation gates (in the gate order netin, i, f, o) and to c_prev, from dh and dc,
// the gradients of h = so tc and of c:
//   dct = dc + dh so (1 - tc^2)
//   d_o = dh tc so (1 - so)     d_f = dct c_prev sf (1 - sf)     d_i = dct tn si (1 - si)     d_netin = dct si (1 - tn^2)
//   dc_prev = dct sf
// Saturated gates give exact zeros, never a NaN: sigma is 0 or 1 there, tanhf +-1, and every factor stays finite.
struct CellGrad {
  float d_netin, d_i, d_f, d_o, dc_prev;
};

__device__ __forceinline__ CellGrad cell_backward(const Cell& s, float c_prev, float dh, float dc) {
  CellGrad g;
  const float dct = dc + dh * s.so * (1.f - s.tc * s.tc);
  g.d_o = dh * s.tc * s.so * (1.f - s.so);
  g.d_f = dct * c_prev * s.sf * (1.f - s.sf);
  g.d_i = dct * s.tn * s.si * (1.f - s.si);
  g.d_netin = dct * s.si * (1.f - s.tn * s.tn);
  g.dc_prev = dct * s.sf;
  return g;
}

}  // namespace clstm
}  // namespace dlwp
