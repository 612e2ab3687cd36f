// tests/cpp/scale_finish.cpp -- HiCCL::scale_finish<T> (include/hiccl/
// elem_types.h), the finishing multiply of a scaled sum, on the host and
// stand-alone: no GPU, no MPI.
//
// For T = bf16 and f16, every one of the 65,536 patterns times each alpha given
// on the command line (hex floats) is compared with the definition worked out
// independently: the product of the widened value and (float)alpha taken
// EXACTLY in double (8 or 11 significand bits times 24 fit), rounded to float,
// then rounded to T -- two roundings.  For float the product in double rounded
// to float (one rounding: exact product, 48 bits), for double the plain
// multiply.  A NaN compares by NaN-ness.  With f16 and alpha 0.7 / 0.1 it also
// counts the finite patterns where ONE rounding of the exact product gives
// another word, and prints the counts: the two-step definition is what is
// tested, and the test stays able to tell.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hiccl/elem_types.h"

static int failures = 0;

template <class T>
static bool is_nan16(uint16_t b);
template <>
bool is_nan16<HiCCL::bf16>(uint16_t b) { return (b & 0x7fff) > 0x7f80; }
template <>
bool is_nan16<HiCCL::f16>(uint16_t b) { return (b & 0x7fff) > 0x7c00; }

// double -> f16 in ONE rounding (to nearest even), for the finite products here
static uint16_t f16_once(double x) {
  if (std::isnan(x)) return 0x7e00;
  const uint16_t sign = std::signbit(x) ? 0x8000 : 0;
  const double a = std::fabs(x);
  if (a == 0) return sign;
  if (std::isinf(a)) return sign | 0x7c00;
  int e;
  std::frexp(a, &e);                      // a = m * 2^e, 0.5 <= m < 1
  const int lsb = e - 11 < -24 ? -24 : e - 11;  // exponent of the last kept bit
  const double q = std::nearbyint(std::ldexp(a, -lsb));  // ties to even (default mode)
  const double v = std::ldexp(q, lsb);
  if (v >= 65520.0) return sign | 0x7c00;
  return sign | HiCCL::f16::round((float)v);  // exact: v is a half value
}

template <class T>
static void halves(const char *name, double alpha, bool count_one_step) {
  const float a32 = (float)alpha;
  long differ_once = 0;
  for (uint32_t p = 0; p < 65536; p++) {
    T s;
    s.bits = (uint16_t)p;
    const T got = HiCCL::scale_finish<T>(s, alpha);
    const double exact = (double)(float)s * (double)a32;
    const T want((float)exact);  // rounded to float, then to T
    const bool gn = is_nan16<T>(got.bits), wn = is_nan16<T>(want.bits);
    if (gn != wn || (!gn && got.bits != want.bits)) {
      if (failures++ < 10)
        std::fprintf(stderr, "%s alpha %a pattern %#06x: got %#06x, the definition gives %#06x\n", name, alpha, p,
                     got.bits, want.bits);
    }
    if (count_one_step && std::isfinite((float)s) && f16_once(exact) != want.bits) differ_once++;
  }
  if (count_one_step) std::printf("scale_finish: f16 alpha %a one-step differs on %ld finite patterns\n", alpha, differ_once);
}

int main(int argc, char **argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: scale_finish ALPHA...\n");
    return 2;
  }
  uint64_t z = 0x9e3779b97f4a7c15ull;
  for (int i = 1; i < argc; i++) {
    const double alpha = std::strtod(argv[i], nullptr);
    const float a32 = (float)alpha;
    halves<HiCCL::bf16>("bf16", alpha, false);
    halves<HiCCL::f16>("f16", alpha, alpha == 0.7 || alpha == 0.1);
    for (int k = 0; k < 200000; k++) {  // float and double on random bit patterns
      z ^= z << 13, z ^= z >> 7, z ^= z << 17;
      float f;
      const uint32_t w = (uint32_t)(z >> 17);
      std::memcpy(&f, &w, 4);
      const float gf = HiCCL::scale_finish<float>(f, alpha), wf = (float)((double)f * (double)a32);
      if (std::isnan(gf) != std::isnan(wf) || (!std::isnan(gf) && std::memcmp(&gf, &wf, 4))) {
        if (failures++ < 10) std::fprintf(stderr, "float alpha %a value %a: got %a want %a\n", alpha, f, gf, wf);
      }
      double d;
      std::memcpy(&d, &z, 8);
      const double gd = HiCCL::scale_finish<double>(d, alpha), wd = d * alpha;
      if (std::isnan(gd) != std::isnan(wd) || (!std::isnan(gd) && std::memcmp(&gd, &wd, 8))) failures++;
    }
  }
  // the plain statements
  const float nz = HiCCL::scale_finish<float>(0.0f, -2.0);
  if (!std::signbit(nz) || nz != 0.0f) failures++, std::fprintf(stderr, "finish(+0, -2) is not -0\n");
  if (!std::isnan(HiCCL::scale_finish<float>(INFINITY, 0.0))) failures++, std::fprintf(stderr, "Inf * 0 is not NaN\n");
  if (failures) {
    std::fprintf(stderr, "scale_finish: %d mismatches\n", failures);
    return 1;
  }
  std::printf("scale_finish: PASSED (%d alphas)\n", argc - 1);
  return 0;
}
