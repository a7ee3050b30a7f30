// What the matrix-pipe convolutions share (conv_mfma.hip: pad(1) + Conv2d(3x3); conv2_mfma.hip: zero-padded Conv2d and
// ConvTranspose2d): the K-slab and LDS pitch, and the conversion of a staged K group into the MFMA operand images.  The
// splits and MFMA wrappers themselves (split3_pair, cvt_pk_bf16, mfma_bf16x6) are common.hpp's, the activation switch is
// act_common.hpp's.
#pragma once
#include "act_common.hpp"

namespace dlwp {
namespace convm {

using actc::apply_act;

constexpr int KSLAB = 32;    // input channels per K-slab: one v_mfma_f32_16x16x32_bf16 per tap and slab
// dwords per staged pixel in LDS (16 hold the 32 channels).  24: the four 16-lane groups of a ds_read_b128 (lanes
// {0-3, 12-15, 20-27}, ...) then start at bank (6 i + g) * 4 mod 64 for pixel i, channel group g -- even for one g, odd for
// the other, all distinct over a row of 16 pixels: reads of 16 consecutive staged pixels are conflict-free (16 would be 4-way,
// 20 2-way).  Where a fragment is two rows of 8 pixels, lanes 0-3 and 12-15 of a group can meet 2-way.  The staging stores are
// 16-byte stores of consecutive pixels, the same address pattern as the reads.
constexpr int PS = 24;

// eight consecutive channels of one staged pixel -> one 16-byte B-operand group per image (NIMG 3: the exact three-part
// split of form "bf16x6"; NIMG 1: the RNE value of form "bf16")
template <int NIMG>
__device__ __forceinline__ void convert_group(const float (&v)[8], u32x4 (&part)[3]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    unsigned h, m, l;
    if (NIMG == 3) split3_pair(v[2 * q], v[2 * q + 1], h, m, l);
    else { h = cvt_pk_bf16(v[2 * q], v[2 * q + 1]); m = 0u; l = 0u; }
    part[0][q] = h; part[1][q] = m; part[2][q] = l;
  }
}

// one element of the weight pack [image][tap][slab][16-channel fragment][lane][8 bf16]: the three bf16 parts of `v`
__device__ __forceinline__ void pack_store(float v, unsigned short* __restrict__ out, long long i, long long total) {
  unsigned h, m, l;
  split3_pair(v, 0.f, h, m, l);
  out[i] = (unsigned short)(h & 0xffffu);
  out[total + i] = (unsigned short)(m & 0xffffu);
  out[2 * total + i] = (unsigned short)(l & 0xffffu);
}

}  // namespace convm
}  // namespace dlwp
