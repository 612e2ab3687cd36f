// tests/cpp/prod_add.cpp -- HiCCL::prodof / bandof / borof / bxorof
// (include/hiccl/ops.h) on the host: a stand-alone program that checks itself.
//
//   prod_add
//
//  * prodof<bf16> and prodof<f16>: `acc = x; acc += m` for all 65,536 patterns
//    x and each of 16 multipliers m (+-0, +-smallest subnormal, +-smallest
//    normal, +-1, 1 + ulp, -2048, +-max, 16, +-Inf, a NaN).  The independent
//    statement is the exact product in double (two significands of at most 11
//    bits: exact) rounded ONCE to the 16-bit format, to nearest even, on the
//    double's bits; a NaN compares by NaN-ness.
//  * prodof<int32_t>, prodof<uint32_t>, prodof<int64_t>, prodof<uint64_t> at
//    the wrap-around extremes (the multiply is done in unsigned: under
//    -fsanitize=undefined a signed overflow would be reported).
//  * bandof / borof / bxorof of 4- and 8-byte integers: identities and folds.
//  * T acc = 0 is the identity for every wrapper; sizes and op_of.
// tests/test_prod_cpu.py builds it plainly and with -fsanitize=address,undefined
// and runs both.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "hiccl/ops.h"

using namespace HiCCL;

static unsigned long errors = 0;

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      if (!errors) std::printf("prod_add: line %d: %s\n", __LINE__, #cond); \
      errors++;                                                       \
    }                                                                 \
  } while (0)

// A 16-bit format: M explicit mantissa bits, smallest normal exponent EMIN.
template <int M, int EMIN>
struct Fmt {
  static constexpr int kExpBits = 15 - M;
  static constexpr uint16_t kInf = (uint16_t)(((1u << kExpBits) - 1u) << M);
  static bool is_nan(uint16_t b) { return (b & 0x7fffu) > kInf; }
  static double widen(uint16_t b) {  // exact
    const int e = (b >> M) & ((1 << kExpBits) - 1), m = b & ((1 << M) - 1);
    double v;
    if (e == (1 << kExpBits) - 1) v = m ? std::numeric_limits<double>::quiet_NaN() : std::numeric_limits<double>::infinity();
    else if (e == 0) v = std::ldexp((double)m, EMIN - M);
    else v = std::ldexp((double)(m | (1 << M)), e - 1 + EMIN - M);
    return (b & 0x8000u) ? -v : v;
  }
  // One rounding to nearest even, on the double's bits.
  static uint16_t round_once(double d) {
    uint64_t w;
    std::memcpy(&w, &d, 8);
    const uint16_t sign = (uint16_t)((w >> 48) & 0x8000u);
    const int de = (int)((w >> 52) & 0x7ff);
    const uint64_t frac = w & ((1ull << 52) - 1);
    if (de == 0x7ff) return (uint16_t)(sign | kInf | (frac ? (1u << (M - 1)) : 0u));
    if (de == 0) return sign;  // zero (a double subnormal is far below half the smallest 16-bit subnormal)
    const int E = de - 1023;
    const uint64_t sig = frac | (1ull << 52);
    const int shift = (52 - M) + (E < EMIN ? EMIN - E : 0);
    if (shift > 63) return sign;
    const uint64_t q = sig >> shift, rem = sig & ((1ull << shift) - 1), half = 1ull << (shift - 1);
    const uint64_t r = q + ((rem > half || (rem == half && (q & 1))) ? 1 : 0);
    // subnormal: r is the word (r == 2^M is the smallest normal); normal: the
    // hidden bit adds into the exponent field, and so does a carry out of r
    const uint64_t bits = E < EMIN ? r : ((uint64_t)(E - EMIN) << M) + r;
    return bits >= kInf ? (uint16_t)(sign | kInf) : (uint16_t)(sign | bits);
  }
};

typedef Fmt<7, -126> BF;
typedef Fmt<10, -14> HF;

static const uint16_t kF16Mul[16] = {0x0000, 0x8000, 0x0001, 0x8001, 0x0400, 0x8400, 0x3C00, 0xBC00,
                                     0x3C01, 0xE800, 0x7BFF, 0xFBFF, 0x4C00, 0x7C00, 0xFC00, 0x7E01};
static const uint16_t kBF16Mul[16] = {0x0000, 0x8000, 0x0001, 0x8001, 0x0080, 0x8080, 0x3F80, 0xBF80,
                                      0x3F81, 0xC500, 0x7F7F, 0xFF7F, 0x4180, 0x7F80, 0xFF80, 0x7FC1};

template <class U, class F>
static void all_patterns(const uint16_t (&mul)[16], const char *name) {
  unsigned long bad = 0;
  for (int a = 0; a < 16; a++) {
    for (uint32_t x = 0; x < 65536; x++) {
      prodof<U> acc, m;
      acc.v.bits = (uint16_t)x;
      m.v.bits = mul[a];
      acc += m;
      const double exact = F::widen((uint16_t)x) * F::widen(mul[a]);
      const uint16_t want = F::round_once(exact);
      const bool ok = F::is_nan(want) ? F::is_nan(acc.v.bits) : acc.v.bits == want;
      if (!ok) {
        if (!bad) std::printf("prod_add: prodof<%s>: %#06x *= %#06x gives %#06x, want %#06x\n", name, x, mul[a], acc.v.bits, want);
        bad++;
      }
    }
  }
  errors += bad;
}

template <class I>
static void integers() {
  typedef std::numeric_limits<I> L;
  typedef typename std::make_unsigned<I>::type W;
  auto mul = [](I a, I b) {
    prodof<I> x, y;
    x.v = a;
    y.v = b;
    x += y;
    return x.v;
  };
  const I top = (I)((W)1 << (sizeof(I) * 8 - 1));  // INT_MIN of a signed type
  CHECK(prodof<I>(0).v == 1);
  CHECK(mul(top, (I)~(I)0) == top);  // -1 x INT_MIN wraps to INT_MIN
  CHECK(mul(L::max(), 2) == (I)((W)L::max() * 2u));
  CHECK(mul(L::max(), L::max()) == (I)((W)L::max() * (W)L::max()));
  CHECK(mul((I)~(I)0, (I)~(I)0) == 1);
  CHECK(mul((I)((W)1 << (sizeof(I) * 4)), (I)((W)1 << (sizeof(I) * 4))) == 0);
  CHECK(mul(top, 2) == 0);
  CHECK(mul((I)3, (I)((W)0x5555555555555555ull)) == (I)~(I)0);
  bandof<I> a = 0;
  borof<I> o = 0;
  bxorof<I> x = 0;
  CHECK(a.v == (I)~(I)0 && o.v == 0 && x.v == 0);
  const I p = (I)((W)0xF0F0F0F0F0F0F0F0ull), q = (I)((W)0xFF00FF00FF00FF00ull);
  bandof<I> ap, aq;
  ap.v = p;
  aq.v = q;
  a += ap;
  CHECK(a.v == p);
  a += aq;
  CHECK(a.v == (I)((W)0xF000F000F000F000ull));
  borof<I> op, oq;
  op.v = p;
  oq.v = q;
  o += op;
  o += oq;
  CHECK(o.v == (I)((W)0xFFF0FFF0FFF0FFF0ull));
  bxorof<I> xp, xq;
  xp.v = p;
  xq.v = q;
  x += xp;
  x += xq;
  CHECK(x.v == (I)((W)0x0FF00FF00FF00FF0ull));
  x += xq;
  CHECK(x.v == p);
}

int main() {
  static_assert(sizeof(prodof<bf16>) == 2 && sizeof(prodof<f16>) == 2 && sizeof(prodof<float>) == 4 &&
                    sizeof(prodof<double>) == 8 && sizeof(bxorof<uint64_t>) == 8 && sizeof(bandof<int32_t>) == 4,
                "a wrapper is its value");
  static_assert(op_of<prodof<float>>() == 16 && op_of<bandof<int>>() == 17 && op_of<borof<long>>() == 18 &&
                    op_of<bxorof<uint64_t>>() == 19 && op_of<maxof<float>>() == 1 && op_of<minof<bf16>>() == 2 &&
                    op_of<float>() == 0,
                "op_of");
  all_patterns<bf16, BF>(kBF16Mul, "bf16");
  all_patterns<f16, HF>(kF16Mul, "f16");
  integers<int32_t>();
  integers<uint32_t>();
  integers<int64_t>();
  integers<uint64_t>();
  // the identity, whatever the int; floats: the sign rule and Inf x 0
  CHECK(prodof<float>(0).v == 1.0f && prodof<double>(7).v == 1.0 && prodof<bf16>(0).v.bits == 0x3f80 &&
        prodof<f16>(0).v.bits == 0x3c00);
  prodof<float> z = 0, nz, inf;
  nz.v = -0.0f;
  inf.v = std::numeric_limits<float>::infinity();
  z += nz;
  CHECK(std::signbit(z.v) && z.v == 0.0f);
  z += inf;
  CHECK(z.v != z.v);
  std::printf("prod_add: %s (%lu errors)\n", errors ? "FAILED" : "PASSED", errors);
  return errors ? 1 : 0;
}
