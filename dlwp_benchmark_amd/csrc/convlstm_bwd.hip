// Backward of the ConvLSTM cell gate math (the forward: convlstm_gates_kernel in conv.hip; reference
// models/convlstm/convlstm.py:96-109 under scripts/train.py:271) on MI355X (gfx950).
//
// gates [B][4*hid][H][W] = (netin, igate, fgate, ogate) before their activations and c_prev [B][hid][H][W] are all the forward
// leaves behind: the kernel recomputes the activations, c and tanh(c) with the forward's own arithmetic (convlstm_cell.hpp)
// and evaluates the closed form stated there.  dgates [B][4*hid][H][W] and dc_prev [B][hid][H][W] from dh and dc, either of
// which may be missing (a zero gradient: the last frame's c_out has none); dc_prev may be unwanted (the first frame's state
// is a constant).  Indexing and grid as the forward: one (sample, channel, pixel) element per thread and loop trip, 64-bit
// indices, grid-stride, at most 256 * 8 workgroups.  Every output element has one writer; no atomics, no workspace: reruns
// are bitwise identical.  The kernel moves 48 bytes per element against ~6 transcendentals: it is memory- and launch-bound,
// so the one refinement is the 16-byte form -- four consecutive pixels per thread when H*W is a multiple of 4 and every
// pointer is 16-byte aligned (the plane offsets are then multiples of 16 bytes too); any other shape runs one pixel per thread.
#include "convlstm_cell.hpp"

namespace dlwp {
namespace clstm {

struct BwdParams {
  const float* gates;
  const float* c_prev;
  const float* dh;        // or null
  const float* dc;        // or null
  float* dgates;
  float* dc_prev;         // or null
  int hid;
  long long HW;
  long long total;        // B * hid * H * W elements
};

// V = 1: a float per thread and trip; V = 4: a float4 (HW % 4 == 0, aligned pointers)
template <int V>
__global__ __launch_bounds__(256) void convlstm_gates_bwd_kernel(const BwdParams p) {
  const long long HWV = p.HW / V, totalV = p.total / V;
  const long long plane = (long long)p.hid * p.HW;         // one gate's block of a sample
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < totalV; i += (long long)gridDim.x * blockDim.x) {
    const long long pix = (i % HWV) * V;
    const long long bc = i / HWV;
    const int ch = (int)(bc % p.hid);
    const long long b = bc / p.hid;
    const long long e = bc * p.HW + pix;                                  // into c_prev, dh, dc, dc_prev
    const long long g = (b * 4 * p.hid + ch) * p.HW + pix;                // the netin plane; i, f, o follow at `plane` strides
    float netin[V], ig[V], fg[V], og[V], cp[V];
    float dh[V] = {}, dc[V] = {};     // a missing gradient is a zero in the same arithmetic: the results are those of a call
                                      // with a zero tensor, bit for bit
    if constexpr (V == 4) {
      auto ld4 = [](const float* q, float (&v)[V]) {
        const float4 t = *reinterpret_cast<const float4*>(q);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
      };
      ld4(p.gates + g, netin);
      ld4(p.gates + g + plane, ig);
      ld4(p.gates + g + 2 * plane, fg);
      ld4(p.gates + g + 3 * plane, og);
      ld4(p.c_prev + e, cp);
      if (p.dh) ld4(p.dh + e, dh);
      if (p.dc) ld4(p.dc + e, dc);
    } else {
      netin[0] = p.gates[g];
      ig[0] = p.gates[g + plane];
      fg[0] = p.gates[g + 2 * plane];
      og[0] = p.gates[g + 3 * plane];
      cp[0] = p.c_prev[e];
      if (p.dh) dh[0] = p.dh[e];
      if (p.dc) dc[0] = p.dc[e];
    }
    CellGrad r[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const Cell s = cell_forward(netin[k], ig[k], fg[k], og[k], cp[k]);
      r[k] = cell_backward(s, cp[k], dh[k], dc[k]);
    }
    if constexpr (V == 4) {
      auto st4 = [](float* q, float a, float b_, float c, float d) { *reinterpret_cast<float4*>(q) = make_float4(a, b_, c, d); };
      st4(p.dgates + g, r[0].d_netin, r[1].d_netin, r[2].d_netin, r[3].d_netin);
      st4(p.dgates + g + plane, r[0].d_i, r[1].d_i, r[2].d_i, r[3].d_i);
      st4(p.dgates + g + 2 * plane, r[0].d_f, r[1].d_f, r[2].d_f, r[3].d_f);
      st4(p.dgates + g + 3 * plane, r[0].d_o, r[1].d_o, r[2].d_o, r[3].d_o);
      if (p.dc_prev) st4(p.dc_prev + e, r[0].dc_prev, r[1].dc_prev, r[2].dc_prev, r[3].dc_prev);
    } else {
      p.dgates[g] = r[0].d_netin;
      p.dgates[g + plane] = r[0].d_i;
      p.dgates[g + 2 * plane] = r[0].d_f;
      p.dgates[g + 3 * plane] = r[0].d_o;
      if (p.dc_prev) p.dc_prev[e] = r[0].dc_prev;
    }
  }
}

}  // namespace clstm
}  // namespace dlwp

using namespace dlwp;

extern "C" int32_t dlwp_convlstm_gates_bwd_f32(const float* gates, const float* c_prev, const float* dh, const float* dc,
                                               float* dgates, float* dc_prev, int32_t batch, int32_t hidden, int32_t H,
                                               int32_t W, void* stream) {
  DLWP_REQUIRE(gates && c_prev && dgates, DLWP_ERR_INVALID_ARGUMENT, "null argument");
  DLWP_REQUIRE(dh || dc, DLWP_ERR_INVALID_ARGUMENT, "neither dh nor dc given: there is nothing to differentiate");
  DLWP_REQUIRE(batch > 0 && hidden > 0 && H > 0 && W > 0, DLWP_ERR_INVALID_ARGUMENT, "bad shape");
  for (const float* in : {gates, c_prev, dh, dc})
    DLWP_REQUIRE(!in || (in != dgates && in != dc_prev), DLWP_ERR_INVALID_ARGUMENT, "an output may not alias an input");
  DLWP_REQUIRE(dgates != dc_prev, DLWP_ERR_INVALID_ARGUMENT, "dgates may not alias dc_prev");
  clstm::BwdParams p;
  p.gates = gates; p.c_prev = c_prev; p.dh = dh; p.dc = dc; p.dgates = dgates; p.dc_prev = dc_prev;
  p.hid = hidden;
  p.HW = (long long)H * W;
  p.total = (long long)batch * hidden * p.HW;
  bool vec = p.HW % 4 == 0;
  for (const void* q : {(const void*)gates, (const void*)c_prev, (const void*)dh, (const void*)dc, (const void*)dgates,
                        (const void*)dc_prev})
    vec = vec && reinterpret_cast<uintptr_t>(q) % 16 == 0;
  const long long work = vec ? p.total / 4 : p.total;
  long long blocks = (work + 255) / 256;
  if (blocks > 256 * 8) blocks = 256 * 8;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (vec) hipLaunchKernelGGL(clstm::convlstm_gates_bwd_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, s, p);
  else hipLaunchKernelGGL(clstm::convlstm_gates_bwd_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, p);
  DLWP_HIP_CHECK(hipGetLastError());
  return DLWP_OK;
}
