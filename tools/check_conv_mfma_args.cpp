// Host-side check of the argument checks of csrc/conv_mfma.hip: a stand-alone program that calls the packed-size and variant
// entries, the three launch entries and the input-gradient entries with bad and oversized shapes.  Every such call returns before any launch, so the
// program needs no GPU; build it with the host sanitizers and run it directly:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -I include tools/check_conv_mfma_args.cpp dlwp_benchmark_amd/csrc/conv_mfma.hip dlwp_benchmark_amd/csrc/core.hip \
//         -o check_conv_mfma_args && ./check_conv_mfma_args
//
// Exit status 0 and "ok" on success; a sanitizer report or a failed expectation otherwise.  With -DPRINT_STATUS every call's
// result is printed too, one per line: the list two builds of the library are compared by.
#include <cstdint>
#include <cstdio>

#include "dlwp_hip.h"

static int failures = 0;
#ifdef PRINT_STATUS
static const bool print_status = true;
#else
static const bool print_status = false;
#endif

#define EXPECT(expr, want)                                                                       \
  do {                                                                                           \
    const long long got_ = (long long)(expr);                                                    \
    if (print_status) std::printf("%d %lld\n", __LINE__, got_);                                   \
    if (got_ != (long long)(want)) {                                                             \
      std::printf("%s:%d: %s = %lld, expected %lld\n", __FILE__, __LINE__, #expr, got_, (long long)(want)); \
      ++failures;                                                                                \
    }                                                                                            \
  } while (0)

int main() {
  // the pointers are never dereferenced on the host and no call below reaches a launch
  static float dummy[16];
  float* x = dummy;
  void* pk = dummy;
  const int32_t big = 0x7fffffff;

  EXPECT(dlwp_conv2d_mfma_packed_bytes(136, 272, 1), 3ll * 9 * 9 * 1024);
  EXPECT(dlwp_conv2d_mfma_packed_bytes(17, 33, 4), 3ll * 16 * 2 * 2 * 1024);
  EXPECT(dlwp_conv2d_mfma_packed_bytes(1, 1, 1), 3 * 1024);
  EXPECT(dlwp_conv2d_mfma_packed_bytes(0, 8, 1), 0);
  EXPECT(dlwp_conv2d_mfma_packed_bytes(8, -1, 1), 0);
  EXPECT(dlwp_conv2d_mfma_packed_bytes(8, 8, 0), 0);
  EXPECT(dlwp_conv2d_mfma_packed_bytes(8, 8, 5), 0);
  EXPECT(dlwp_conv2d_mfma_packed_bytes(big, big, 4), 0);
  EXPECT(dlwp_conv2d_mfma_packed_bytes(1 << 20, 1 << 20, 1), 0);

  EXPECT(dlwp_conv2d_mfma_variant(0, 384, 32, 32, 136, 1, 1, 0), 16 * 16 + 4);
  EXPECT(dlwp_conv2d_mfma_variant(0, 12, 8, 8, 6, 3, 2, 1), 8 * 16 + 2);
  EXPECT(dlwp_conv2d_mfma_variant(1, 384, 16, 16, 272, 4, 2, 1), 16 * 16 + 4);
  EXPECT(dlwp_conv2d_mfma_variant(1, 1, 8, 16, 8, 2, 2, 0), 16 * 16 + 1);
  EXPECT(dlwp_conv2d_mfma_variant(0, 0, 8, 8, 8, 1, 1, 0), 0);
  EXPECT(dlwp_conv2d_mfma_variant(0, 1, 8, 8, 8, 3, 3, 1), 0);
  EXPECT(dlwp_conv2d_mfma_variant(0, 1, 2, 2, 8, 4, 1, 0), 0);
  EXPECT(dlwp_conv2d_mfma_variant(1, 1, 8, 8, 8, 3, 2, 1), 0);
  EXPECT(dlwp_conv2d_mfma_variant(0, big, big, big, big, 1, 1, 0), 0);
  EXPECT(dlwp_conv2d_mfma_variant(1, big, big, big, big, 4, 2, 1), 0);
  EXPECT(dlwp_conv2d_mfma_variant(0, big, 46000, 46000, big, 4, 2, 3) > 0, 1);      // the largest grid the rule is asked about
  EXPECT(dlwp_conv2d_mfma_variant(0, 1, big, 1, 1, 4, 2, 3), 0);

  EXPECT(dlwp_conv2d_mfma_pack_f32(nullptr, 8, 8, 1, 0, pk, nullptr), DLWP_ERR_INVALID_ARGUMENT);
  EXPECT(dlwp_conv2d_mfma_pack_f32(x, 8, 8, 5, 0, pk, nullptr), DLWP_ERR_UNSUPPORTED);
  EXPECT(dlwp_conv2d_mfma_pack_f32(x, big, big, 4, 1, pk, nullptr), DLWP_ERR_UNSUPPORTED);

  auto conv = [&](int32_t batch, int32_t cin, int32_t H, int32_t W, int32_t cout, int32_t k, int32_t s, int32_t p, int32_t form) {
    return dlwp_conv2d_mfma_f32(x, pk, nullptr, nullptr, x, batch, cin, H, W, cout, k, s, p, 0, 0, form, nullptr);
  };
  auto tconv = [&](int32_t batch, int32_t cin, int32_t H, int32_t W, int32_t cout, int32_t k, int32_t s, int32_t p, int32_t form) {
    return dlwp_conv_transpose2d_mfma_f32(x, pk, nullptr, x, batch, cin, H, W, cout, k, s, p, 0, form, nullptr);
  };
  EXPECT(dlwp_conv2d_mfma_f32(nullptr, pk, nullptr, nullptr, x, 1, 4, 8, 8, 4, 1, 1, 0, 0, 0, 0, nullptr), DLWP_ERR_INVALID_ARGUMENT);
  EXPECT(dlwp_conv2d_mfma_f32(x, pk, nullptr, nullptr, x, 1, 4, 8, 8, 4, 1, 1, 0, 5, 0, 0, nullptr), DLWP_ERR_INVALID_ARGUMENT);
  EXPECT(conv(0, 4, 8, 8, 4, 1, 1, 0, 0), DLWP_ERR_INVALID_ARGUMENT);
  EXPECT(conv(1, 4, 8, 8, 4, 1, 1, 0, 2), DLWP_ERR_INVALID_ARGUMENT);            // unknown form
  EXPECT(conv(1, 4, 2, 2, 4, 4, 1, 0, 0), DLWP_ERR_INVALID_ARGUMENT);            // empty output
  EXPECT(conv(1, 4, 8, 8, 4, 5, 1, 2, 0), DLWP_ERR_UNSUPPORTED);                 // geometry
  EXPECT(conv(1, 4, 8, 8, 4, 3, 3, 1, 0), DLWP_ERR_UNSUPPORTED);
  EXPECT(conv(1, 4, 8, 8, 4, 3, 1, 3, 0), DLWP_ERR_UNSUPPORTED);
  EXPECT(conv(65536, 4, 8, 8, 4, 1, 1, 0, 0), DLWP_ERR_UNSUPPORTED);             // batch over the grid
  EXPECT(conv(1, 4, 32768, 32768, 4, 1, 1, 0, 0), DLWP_ERR_UNSUPPORTED);         // 32-bit offsets inside a sample
  EXPECT(conv(1, 4, big, big, 4, 4, 2, 3, 0), DLWP_ERR_UNSUPPORTED);
  EXPECT(conv(1, big, 1, 1, 4, 1, 1, 0, 0), DLWP_ERR_UNSUPPORTED);
  EXPECT(conv(1, 1 << 20, 4, 4, 1 << 20, 1, 1, 0, 0), DLWP_ERR_UNSUPPORTED);     // pack of 2 GiB and more
  EXPECT(conv(big, big, big, big, big, 4, 2, 3, 1), DLWP_ERR_UNSUPPORTED);

  EXPECT(dlwp_conv_transpose2d_mfma_f32(x, nullptr, nullptr, x, 1, 4, 8, 8, 4, 4, 2, 1, 0, 0, nullptr), DLWP_ERR_INVALID_ARGUMENT);
  EXPECT(dlwp_conv_transpose2d_mfma_f32(x, pk, nullptr, x, 1, 4, 8, 8, 4, 4, 2, 1, -1, 0, nullptr), DLWP_ERR_INVALID_ARGUMENT);
  EXPECT(tconv(1, 4, 0, 8, 4, 4, 2, 1, 0), DLWP_ERR_INVALID_ARGUMENT);
  EXPECT(tconv(1, 4, 8, 8, 4, 4, 2, 1, 7), DLWP_ERR_INVALID_ARGUMENT);
  EXPECT(tconv(1, 4, 8, 8, 4, 3, 2, 1, 0), DLWP_ERR_UNSUPPORTED);
  EXPECT(tconv(1, 4, 8, 8, 4, 4, 2, 0, 0), DLWP_ERR_UNSUPPORTED);
  EXPECT(tconv(1, 4, 8, 8, 4, 2, 1, 0, 0), DLWP_ERR_UNSUPPORTED);
  EXPECT(tconv(65536, 4, 8, 8, 4, 2, 2, 0, 0), DLWP_ERR_UNSUPPORTED);
  EXPECT(tconv(1, 4, 32768, 32768, 4, 4, 2, 1, 0), DLWP_ERR_UNSUPPORTED);
  EXPECT(tconv(1, 4, big, big, 4, 4, 2, 1, 0), DLWP_ERR_UNSUPPORTED);
  EXPECT(tconv(1, 1 << 20, 4, 4, 1 << 20, 2, 2, 0, 0), DLWP_ERR_UNSUPPORTED);
  EXPECT(tconv(big, big, big, big, big, 2, 2, 0, 1), DLWP_ERR_UNSUPPORTED);
  EXPECT(dlwp_conv_transpose2d_mfma_f32(x, pk, nullptr, x + 1, 1, 4, 8, 8, 4, 2, 2, 0, 0, 0, nullptr), DLWP_ERR_INVALID_ARGUMENT);  // y 4-byte aligned

  // the padded 3x3 layer: the k x k queries at k = 3, and its own launch entry
  EXPECT(dlwp_conv3x3_mfma_packed_bytes(170, 19), 3ll * 9 * 1 * 11 * 1024);
  EXPECT(dlwp_conv3x3_mfma_packed_bytes(272, 272), dlwp_conv2d_mfma_packed_bytes(272, 272, 3));
  EXPECT(dlwp_conv3x3_mfma_packed_bytes(0, 8), 0);
  EXPECT(dlwp_conv3x3_mfma_packed_bytes(8, -1), 0);
  EXPECT(dlwp_conv3x3_mfma_packed_bytes(1 << 20, 1 << 20), 0);
  EXPECT(dlwp_conv3x3_mfma_packed_bytes(big, 8), 0);
  EXPECT(dlwp_conv3x3_mfma_packed_bytes(8, big), 0);                               // cin + 31 in int: overflowed before
  EXPECT(dlwp_conv3x3_mfma_packed_bytes(big, big), 0);                             // 27 KiB * slabs * fragments: past long long before

  EXPECT(dlwp_conv3x3_mfma_variant(12, 8, 8, 6), 8 * 16 + 1);
  EXPECT(dlwp_conv3x3_mfma_variant(384, 32, 32, 136), dlwp_conv2d_mfma_variant(0, 384, 32, 32, 136, 3, 1, 1));
  EXPECT(dlwp_conv3x3_mfma_variant(0, 8, 8, 8), 0);
  EXPECT(dlwp_conv3x3_mfma_variant(1, -8, 8, 8), 0);
  EXPECT(dlwp_conv3x3_mfma_variant(1, 8, 8, 0), 0);
  EXPECT(dlwp_conv3x3_mfma_variant(big, 20, 20, big) > 0, 1);

  EXPECT(dlwp_conv3x3_mfma_pack_f32(nullptr, 8, 8, pk, nullptr), DLWP_ERR_INVALID_ARGUMENT);
  EXPECT(dlwp_conv3x3_mfma_pack_f32(x, 0, 8, pk, nullptr), DLWP_ERR_UNSUPPORTED);
  EXPECT(dlwp_conv3x3_mfma_pack_f32(x, 1 << 20, 1 << 20, pk, nullptr), DLWP_ERR_UNSUPPORTED);
  EXPECT(dlwp_conv3x3_mfma_pack_f32(x, big, big, pk, nullptr), DLWP_ERR_UNSUPPORTED);

  static int32_t ring[16];
  auto c3 = [&](int32_t batch, int32_t c0, int32_t c1, int32_t H, int32_t W, int32_t cout, int32_t form, const int32_t* table) {
    return dlwp_conv3x3_mfma_f32(x, c0, c1 ? x : nullptr, c1, pk, nullptr, nullptr, x, batch, H, W, cout, 0, 0, table, form, nullptr);
  };
  EXPECT(dlwp_conv3x3_mfma_f32(nullptr, 4, nullptr, 0, pk, nullptr, nullptr, x, 1, 8, 8, 4, 0, 0, nullptr, 0, nullptr), DLWP_ERR_INVALID_ARGUMENT);
  EXPECT(dlwp_conv3x3_mfma_f32(x, 4, nullptr, 2, pk, nullptr, nullptr, x, 1, 8, 8, 4, 0, 0, nullptr, 0, nullptr), DLWP_ERR_INVALID_ARGUMENT);  // c1 > 0, x1 null
  EXPECT(dlwp_conv3x3_mfma_f32(x, 4, nullptr, 0, pk, nullptr, nullptr, x, 1, 8, 8, 4, 5, 0, nullptr, 0, nullptr), DLWP_ERR_INVALID_ARGUMENT);  // unknown pre_act
  EXPECT(dlwp_conv3x3_mfma_f32(x, 4, nullptr, 0, pk, nullptr, nullptr, x, 1, 8, 8, 4, 0, -1, nullptr, 0, nullptr), DLWP_ERR_INVALID_ARGUMENT); // unknown act
  EXPECT(c3(0, 4, 0, 8, 8, 4, 0, nullptr), DLWP_ERR_INVALID_ARGUMENT);            // zero and negative extents
  EXPECT(c3(1, 0, 0, 8, 8, 4, 0, nullptr), DLWP_ERR_INVALID_ARGUMENT);
  EXPECT(c3(1, 4, -1, 8, 8, 4, 0, nullptr), DLWP_ERR_INVALID_ARGUMENT);
  EXPECT(c3(1, 4, 0, -8, 8, 4, 0, nullptr), DLWP_ERR_INVALID_ARGUMENT);
  EXPECT(c3(1, 4, 0, 8, 0, 4, 0, nullptr), DLWP_ERR_INVALID_ARGUMENT);
  EXPECT(c3(1, 4, 0, 8, 8, -4, 0, nullptr), DLWP_ERR_INVALID_ARGUMENT);
  EXPECT(c3(1, 4, 0, 8, 1, 4, 0, nullptr), DLWP_ERR_INVALID_ARGUMENT);            // a cylinder of one column
  EXPECT(c3(1, 4, 0, 8, 8, 4, 2, nullptr), DLWP_ERR_INVALID_ARGUMENT);            // unknown form
  EXPECT(c3(13, 4, 0, 8, 8, 4, 0, ring), DLWP_ERR_INVALID_ARGUMENT);              // faces not a multiple of 12
  EXPECT(c3(12, 4, 0, 16384, 16384, 4, 0, ring), DLWP_ERR_INVALID_ARGUMENT);      // face too large for the ring table
  EXPECT(c3(65536, 4, 0, 8, 8, 4, 0, nullptr), DLWP_ERR_UNSUPPORTED);             // batch over the grid
  EXPECT(c3(big, 4, 0, 8, 8, 4, 0, nullptr), DLWP_ERR_UNSUPPORTED);
  EXPECT(c3(1, 4, 0, 32768, 32768, 4, 0, nullptr), DLWP_ERR_UNSUPPORTED);         // 32-bit offsets inside a sample
  EXPECT(c3(1, 4, 0, big, 8, 4, 0, nullptr), DLWP_ERR_UNSUPPORTED);
  EXPECT(c3(1, 4, 0, 8, big, 4, 0, nullptr), DLWP_ERR_UNSUPPORTED);
  EXPECT(c3(1, 4, 0, big, big, 4, 0, nullptr), DLWP_ERR_UNSUPPORTED);
  EXPECT(c3(1, big, 0, 1, 2, 4, 0, nullptr), DLWP_ERR_UNSUPPORTED);               // input channels
  EXPECT(c3(1, big, big, 1, 2, 4, 0, nullptr), DLWP_ERR_UNSUPPORTED);             // c0 + c1 past int
  EXPECT(c3(1, 4, 0, 1, 2, big, 0, nullptr), DLWP_ERR_UNSUPPORTED);               // output channels
  EXPECT(c3(1, 1 << 20, 0, 4, 4, 1 << 20, 0, nullptr), DLWP_ERR_UNSUPPORTED);     // pack of 2 GiB and more
  EXPECT(c3(big, big, big, big, big, big, 1, nullptr), DLWP_ERR_UNSUPPORTED);

  // the Conv2d input gradient: the variant query runs the launcher's own checks, the entry returns before any launch
  auto dv = [&](int32_t batch, int32_t cin, int32_t cout, int32_t H, int32_t W, int32_t k, int32_t s, int32_t p) {
    return dlwp_conv2d_dgrad_mfma_variant(batch, cin, cout, H, W, k, s, p);
  };
  auto dg = [&](int32_t batch, int32_t cin, int32_t H, int32_t W, int32_t cout, int32_t k, int32_t s, int32_t p) {
    return dlwp_conv2d_dgrad_mfma_f32(x, pk, x, batch, cin, H, W, cout, k, s, p, nullptr);
  };
  EXPECT(dv(2, 6, 4, 8, 16, 3, 2, 1), 4096 * 4 + 1024 + 16 * 8 + 1);              // 3x3 s2 p1: the 4x4 window, parity form
  EXPECT(dv(1, 3, 2, 5, 7, 2, 2, 0), 4096 * 2 + 1024 + 16 * 8 + 1);
  EXPECT(dv(1, 3, 2, 5, 7, 1, 2, 0), 4096 * 2 + 1024 + 16 * 8 + 1);               // 1x1 s2: the 2x2 window
  EXPECT(dv(1, 2, 3, 8, 16, 3, 1, 1), 4096 * 3 + 16 * 16 + 1);                    // stride 1: the reversed pack, ZeroPadWindow<8>
  EXPECT(dv(64, 208, 8, 16, 32, 4, 2, 1), 4096 * 4 + 1024 + 16 * 16 + 4);
  EXPECT(dv(1, 3, 2, 6, 9, 3, 2, 0) > 0, 1);                                      // what the 4x4 window holds as well
  EXPECT(dv(1, 3, 2, 6, 9, 4, 2, 2) > 0, 1);
  EXPECT(dv(0, 3, 2, 8, 8, 1, 1, 0), 0);                                          // bad shapes
  EXPECT(dv(1, 0, 2, 8, 8, 1, 1, 0), 0);
  EXPECT(dv(1, 3, -2, 8, 8, 1, 1, 0), 0);
  EXPECT(dv(1, 3, 2, 0, 8, 1, 1, 0), 0);
  EXPECT(dv(1, 3, 2, 8, 8, 0, 1, 0), 0);
  EXPECT(dv(1, 3, 2, 8, 8, 3, 0, 1), 0);
  EXPECT(dv(1, 3, 2, 8, 8, 3, 1, -1), 0);
  EXPECT(dv(1, 3, 2, 2, 2, 4, 1, 0), 0);                                          // empty output
  EXPECT(dv(1, 3, 2, 8, 8, 4, 2, 3), 0);                                          // geometry
  EXPECT(dv(1, 3, 2, 8, 8, 2, 2, 1), 0);
  EXPECT(dv(1, 3, 2, 8, 8, 1, 2, 1), 0);
  EXPECT(dv(1, 3, 2, 8, 8, 5, 1, 2), 0);
  EXPECT(dv(1, 3, 2, 8, 8, 3, 3, 1), 0);
  EXPECT(dv(65536, 3, 2, 8, 8, 3, 2, 1), 0);                                      // batch over the grid
  EXPECT(dv(1, 3, 2, 32768, 32768, 3, 2, 1), 0);                                  // 32-bit offsets inside a sample
  EXPECT(dv(1, 3, 2, big, big, 4, 2, 1), 0);                                      // ceil(H / 2) of INT_MAX: no H + 1 in int
  EXPECT(dv(1, 3, 2, big, 1, 1, 2, 0), 0);
  EXPECT(dv(1, 3, 2, 1, big, 2, 2, 0), 0);
  EXPECT(dv(1, 3, 2, big, big, 3, 1, 1), 0);
  EXPECT(dv(1, big, 2, 1, 1, 1, 1, 0), 0);                                        // channels
  EXPECT(dv(1, 3, big, 1, 1, 1, 1, 0), 0);
  EXPECT(dv(1, 1 << 20, 1 << 20, 4, 4, 1, 1, 0), 0);                              // pack of 2 GiB and more
  EXPECT(dv(big, big, big, big, big, 4, 2, 2), 0);
  EXPECT(dv(1, 1, 2, 8000, 8000, 4, 2, 1) > 0, 1);                                // large maps inside the 32-bit offsets
  EXPECT(dv(1, 1, 2, 8001, 7999, 3, 2, 1) > 0, 1);
  EXPECT(dv(1, 3, 2, 46000, 46000, 4, 2, 1), 0);                                  // 3 x 46000^2 elements per sample of dx

  EXPECT(dlwp_conv2d_dgrad_mfma_f32(nullptr, pk, x, 1, 3, 8, 8, 2, 3, 2, 1, nullptr), DLWP_ERR_INVALID_ARGUMENT);
  EXPECT(dlwp_conv2d_dgrad_mfma_f32(x, nullptr, x, 1, 3, 8, 8, 2, 3, 2, 1, nullptr), DLWP_ERR_INVALID_ARGUMENT);
  EXPECT(dlwp_conv2d_dgrad_mfma_f32(x, pk, nullptr, 1, 3, 8, 8, 2, 3, 2, 1, nullptr), DLWP_ERR_INVALID_ARGUMENT);
  EXPECT(dg(0, 3, 8, 8, 2, 3, 2, 1), DLWP_ERR_INVALID_ARGUMENT);
  EXPECT(dg(1, 3, 8, -8, 2, 3, 2, 1), DLWP_ERR_INVALID_ARGUMENT);
  EXPECT(dg(1, 3, 8, 8, 2, 3, 2, -1), DLWP_ERR_INVALID_ARGUMENT);
  EXPECT(dg(1, 3, 2, 2, 2, 4, 1, 0), DLWP_ERR_UNSUPPORTED);                       // no output pixel: outside the envelope
  EXPECT(dg(1, 3, 8, 8, 2, 4, 2, 3), DLWP_ERR_UNSUPPORTED);
  EXPECT(dg(1, 3, 8, 8, 2, 2, 2, 1), DLWP_ERR_UNSUPPORTED);
  EXPECT(dg(1, 3, 8, 8, 2, 5, 1, 2), DLWP_ERR_UNSUPPORTED);
  EXPECT(dg(1, 3, 8, 8, 2, 3, 3, 1), DLWP_ERR_UNSUPPORTED);
  EXPECT(dg(65536, 3, 8, 8, 2, 3, 2, 1), DLWP_ERR_UNSUPPORTED);
  EXPECT(dg(1, 3, 32768, 32768, 2, 3, 2, 1), DLWP_ERR_UNSUPPORTED);
  EXPECT(dg(1, 3, big, big, 2, 4, 2, 1), DLWP_ERR_UNSUPPORTED);
  EXPECT(dg(1, 3, big, big, 2, 1, 2, 0), DLWP_ERR_UNSUPPORTED);
  EXPECT(dg(1, 3, big, 1, 2, 3, 1, 1), DLWP_ERR_UNSUPPORTED);
  EXPECT(dg(1, big, 1, 1, 2, 1, 1, 0), DLWP_ERR_UNSUPPORTED);
  EXPECT(dg(1, 3, 1, 1, big, 1, 1, 0), DLWP_ERR_UNSUPPORTED);
  EXPECT(dg(1, 1 << 20, 4, 4, 1 << 20, 1, 1, 0), DLWP_ERR_UNSUPPORTED);
  EXPECT(dg(big, big, big, big, big, 4, 2, 2), DLWP_ERR_UNSUPPORTED);

  EXPECT(dlwp_conv2d_mfma_pack_ex_f32(nullptr, 8, 8, 3, 4, 1, 0, pk, nullptr), DLWP_ERR_INVALID_ARGUMENT);
  EXPECT(dlwp_conv2d_mfma_pack_ex_f32(x, 8, 8, 3, 2, 1, 0, pk, nullptr), DLWP_ERR_INVALID_ARGUMENT);     // k_packed < k
  EXPECT(dlwp_conv2d_mfma_pack_ex_f32(x, 8, 8, 0, 2, 1, 0, pk, nullptr), DLWP_ERR_INVALID_ARGUMENT);
  EXPECT(dlwp_conv2d_mfma_pack_ex_f32(x, 8, 8, 4, 5, 1, 1, pk, nullptr), DLWP_ERR_UNSUPPORTED);
  EXPECT(dlwp_conv2d_mfma_pack_ex_f32(x, big, big, 3, 4, 1, 0, pk, nullptr), DLWP_ERR_UNSUPPORTED);

  if (failures == 0) std::printf("ok\n");
  return failures ? 1 : 0;
}
