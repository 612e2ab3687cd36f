// tests/cpp/f16_add.cpp -- HiCCL::f16's `+=` on every bit pattern (host only).
//
//   f16_add OUT
//
// For each of 16 fixed addends a (tests/hostile_f16.py ADDENDS: +-0, +-2^-24,
// +-2^-14, +-1, 1 + 2^-10, -2048, +-65504, 16, +-Inf, one NaN) and each of the
// 65,536 patterns x:  T acc = x; acc += a;  the resulting bits go to OUT as
// uint16[16][65536].  tests/test_f16_cpu.py compares them with NumPy's half
// add.  Also checks, on every pattern, that float -> f16 -> float is the
// identity on half values (NaN by NaN-ness) and that `T acc = 0` is +0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "hiccl/compute.h"  // built with -DHICCL_PORT_HOST: no HIP

using HiCCL::f16;

static_assert(HiCCL::dtype_of<f16>() == 6, "f16 -> HICCL_FLOAT16");
static_assert(HiCCL::dtype_of<HiCCL::bf16>() == 2, "bf16 -> HICCL_BFLOAT16");
static_assert(HiCCL::dtype_of<uint16_t>() == -1, "other 2-byte types have no reduction");
#ifdef __FLT16_MANT_DIG__
static_assert(HiCCL::dtype_of<_Float16>() == 6, "_Float16 -> HICCL_FLOAT16");
#endif

static const uint16_t kAddends[16] = {0x0000, 0x8000, 0x0001, 0x8001, 0x0400, 0x8400, 0x3C00, 0xBC00,
                                      0x3C01, 0xE800, 0x7BFF, 0xFBFF, 0x4C00, 0x7C00, 0xFC00, 0x7E01};

static bool is_nan(uint16_t b) { return (b & 0x7C00) == 0x7C00 && (b & 0x03FF); }

int main(int argc, char **argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: f16_add OUT\n");
    return 2;
  }
  f16 zero = 0;
  if (zero.bits != 0) {
    std::fprintf(stderr, "f16 acc = 0 is %#06x\n", zero.bits);
    return 1;
  }
  for (uint32_t b = 0; b < 65536; b++) {
    f16 x;
    x.bits = (uint16_t)b;
    const float f = (float)x;
    const f16 back(f);
    if (is_nan(x.bits) ? !(std::isnan(f) && is_nan(back.bits)) : back != x) {
      std::fprintf(stderr, "round trip of %#06x gives %#06x\n", b, back.bits);
      return 1;
    }
  }
  std::vector<uint16_t> out(16u * 65536u);
  for (int a = 0; a < 16; a++) {
    f16 add;
    add.bits = kAddends[a];
    for (uint32_t b = 0; b < 65536; b++) {
      f16 acc;
      acc.bits = (uint16_t)b;
      acc += add;
      out[(size_t)a * 65536 + b] = acc.bits;
    }
  }
  FILE *fh = std::fopen(argv[1], "wb");
  if (!fh || std::fwrite(out.data(), 2, out.size(), fh) != out.size() || std::fclose(fh)) {
    std::fprintf(stderr, "cannot write %s\n", argv[1]);
    return 1;
  }
  std::printf("f16_add: wrote %zu sums\n", out.size());
  return 0;
}
