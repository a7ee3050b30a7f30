// Every kernel of the specialised FNO2d / SpectralConv2d path, as ONE translation unit made of two source files:
//
//   fno_unfused.hpp   one kernel per stage (lifting, modes, layer, projection, ...) and the host functions that launch them
//   fno_trunk.hpp     the fused kernel (all layers / a whole step / a whole rollout range in one launch) and its launch
//
// The two are read, changed and reviewed apart.  They are compiled together because the code hipcc generates for a
// kernel depends on the other kernels of its module wherever they share an inline helper (fno_device.hpp): compiled apart,
// the fused kernel stays as it is, but pw_lift_bf16x6_kernel<4, *> (lift_segment, shared with the step kernel) changes its
// registers, and without pw_mlp2_kernel in the module every user of fwd_dft_accumulate does (fwd_dft_kernel 108 -> 100
// VGPRs, fno_layer_kernel, all sixteen pw_lift_bf16x6_kernel).  In one module every kernel is text-identical to what has
// been measured; tools/kernel_isa_diff.py against the previous build is the check for any regrouping.
#include "fno_unfused.hpp"
#include "fno_trunk.hpp"
