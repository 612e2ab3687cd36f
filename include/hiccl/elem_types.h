// include/hiccl/elem_types.h -- the 2-byte and 1-byte element types of Comm<T>
// / Compute<T>: HiCCL::bf16, HiCCL::f16 and the OCP FP8 pair HiCCL::f8e4m3 /
// f8e5m2 (storage structs whose `+=` is the
// reference's `T acc = 0; acc += x` in that type), and scale_finish<T>, the
// finishing multiply of a scaled sum.  Plain C++, no dependency:
// compute.h and ops.h include it, and so can a host-only test.
#ifndef HICCL_ELEM_TYPES_H
#define HICCL_ELEM_TYPES_H

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <type_traits>

namespace HiCCL {

// bfloat16 storage type for Comm<bf16> / Compute<bf16>.  The arithmetic is
// the reference's `T acc = 0; acc += x` (compute.h:7-9) with T = bf16: an
// f32 add rounded to nearest-even bf16 after every add -- the host port
// below and the GPU kernels (HICCL_BFLOAT16, HICCL_ACC_NATIVE) give the same
// bits.  Two 2-byte types have a reduction: this one (HICCL_BFLOAT16) and
// f16 below (HICCL_FLOAT16, with the compiler's _Float16 where it has one);
// other 2-byte types (int16_t, uint16_t) fail to compile.
struct bf16 {
  uint16_t bits = 0;
  bf16() = default;
  bf16(int v) : bits(round((float)v)) {}  // T acc = 0
  explicit bf16(float f) : bits(round(f)) {}
  explicit operator float() const {
    uint32_t w = (uint32_t)bits << 16;
    float f;
    std::memcpy(&f, &w, 4);
    return f;
  }
  bf16 &operator+=(bf16 o) {
    bits = round((float)*this + (float)o);
    return *this;
  }
  bool operator==(bf16 o) const { return bits == o.bits; }
  bool operator!=(bf16 o) const { return bits != o.bits; }
  static uint16_t round(float f) {  // round to nearest even; NaN stays NaN
    uint32_t w;
    std::memcpy(&w, &f, 4);
    if ((w & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((w >> 16) | 0x40);
    w += 0x7fffu + ((w >> 16) & 1u);
    return (uint16_t)(w >> 16);
  }
};
static_assert(sizeof(bf16) == 2, "bf16 storage");

// IEEE half (binary16) storage type for Comm<f16> / Compute<f16>, shaped
// like bf16 above.  `+=` widens both operands (exact), adds in f32 and rounds
// to nearest-even half: the same bits as a half add, since f32's 24
// significand bits >= 2 * 11 + 2 make the double rounding innocuous.  The host
// port below and the GPU kernels (HICCL_FLOAT16, HICCL_ACC_NATIVE: a native
// v_pk_add_f16) give the same bits; a NaN stays a NaN (payloads may differ).
struct f16 {
  uint16_t bits = 0;
  f16() = default;
  f16(int v) : bits(round((float)v)) {}  // T acc = 0
  explicit f16(float f) : bits(round(f)) {}
  explicit operator float() const {
    const uint32_t sign = (uint32_t)(bits & 0x8000u) << 16;
    uint32_t e = (bits >> 10) & 0x1fu, m = bits & 0x3ffu, w;
    if (e == 0x1fu) {
      w = sign | 0x7f800000u | (m << 13);  // Inf / NaN
    } else if (e) {
      w = sign | ((e + 112u) << 23) | (m << 13);
    } else if (m) {  // subnormal: m * 2^-24, normalised
      e = 113;
      while (!(m & 0x400u)) {
        m <<= 1;
        e--;
      }
      w = sign | (e << 23) | ((m & 0x3ffu) << 13);
    } else {
      w = sign;
    }
    float f;
    std::memcpy(&f, &w, 4);
    return f;
  }
  f16 &operator+=(f16 o) {
    bits = round((float)*this + (float)o);
    return *this;
  }
  bool operator==(f16 o) const { return bits == o.bits; }
  bool operator!=(f16 o) const { return bits != o.bits; }
  // round to nearest even; overflow gives Inf, results below 2^-14 are
  // subnormal halves, NaN stays NaN
  static uint16_t round(float f) {
    uint32_t w;
    std::memcpy(&w, &f, 4);
    const uint16_t sign = (uint16_t)((w >> 16) & 0x8000u);
    const uint32_t a = w & 0x7fffffffu;
    if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u | ((a >> 13) & 0x3ffu));  // NaN (quiet)
    if (a >= 0x47800000u) return (uint16_t)(sign | 0x7c00u);  // >= 2^16 (Inf too): Inf
    if (a >= 0x38800000u) {  // normal half (>= 2^-14); a carry out of the mantissa moves into the
                             // exponent, and from 65520 on into Inf
      const uint32_t r = a - 0x38000000u + 0xfffu + ((a >> 13) & 1u);
      return (uint16_t)(sign | (r >> 13));
    }
    if (a < 0x33000000u) return sign;  // < 2^-25: rounds to zero (2^-25 itself ties to even, zero)
    // subnormal half: the 24-bit significand shifted down to units of 2^-24
    const uint32_t e = a >> 23, sig = (a & 0x7fffffu) | 0x800000u;
    const uint32_t shift = 126u - e;  // 14..24
    const uint32_t q = sig >> shift, rem = sig & ((1u << shift) - 1u), half = 1u << (shift - 1);
    return (uint16_t)(sign | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u)));
  }
};
static_assert(sizeof(f16) == 2, "f16 storage");

// OCP FP8 storage types for Comm<T> / Compute<T>, shaped like bf16 above:
// f8e4m3 (e4m3fn: bias 7, largest finite value 448, no infinities, NaN is
// (b & 0x7f) == 0x7f; HICCL_FLOAT8_E4M3) and f8e5m2 (bias 15, largest finite
// value 57344, infinities 0x7c / 0xfc, NaN above them; HICCL_FLOAT8_E5M2).
// `operator float` is the exact value.  round(f): a NaN gives a NaN, +-Inf
// gives +-Inf in e5m2 and a NaN in e4m3, a finite f is clamped to [-max, +max]
// (saturate to finite) and then rounded to nearest even, subnormals kept, and
// a magnitude of at most half the smallest subnormal gives a zero with f's
// sign.  `+=` is the reference's `T acc = 0; acc += x` in that type: widen
// both (exact), add in f32, round -- the bits of the GPU kernels
// (HICCL_ACC_NATIVE).
template <bool E5M2>
struct fp8 {
  static constexpr int kMan = E5M2 ? 2 : 3, kBias = E5M2 ? 15 : 7;
  static constexpr uint32_t kMaxF32 = E5M2 ? 0x47600000u : 0x43e00000u;  // 57344.0f / 448.0f
  uint8_t bits = 0;
  fp8() = default;
  fp8(int v) : bits(round((float)v)) {}  // T acc = 0
  explicit fp8(float f) : bits(round(f)) {}
  bool isnan() const { return E5M2 ? (bits & 0x7fu) > 0x7cu : (bits & 0x7fu) == 0x7fu; }
  explicit operator float() const {
    const uint32_t sign = (uint32_t)(bits & 0x80u) << 24;
    const uint32_t e = (bits & 0x7fu) >> kMan, m = bits & ((1u << kMan) - 1u);
    uint32_t w;
    if (isnan()) {
      w = sign | 0x7fc00000u;
    } else if (E5M2 && e == 0x1fu) {
      w = sign | 0x7f800000u;
    } else if (e) {
      w = sign | ((e + 127u - kBias) << 23) | (m << (23 - kMan));
    } else {  // zero or subnormal: m * 2^(1 - bias - man), exact in f32
      const float sub = (float)m * (E5M2 ? 1.52587890625e-05f : 0.001953125f);  // 2^-16 / 2^-9
      std::memcpy(&w, &sub, 4);
      w |= sign;
    }
    float f;
    std::memcpy(&f, &w, 4);
    return f;
  }
  fp8 &operator+=(fp8 o) {
    bits = round((float)*this + (float)o);
    return *this;
  }
  bool operator==(fp8 o) const { return bits == o.bits; }
  bool operator!=(fp8 o) const { return bits != o.bits; }
  static uint8_t round(float f) {
    uint32_t w;
    std::memcpy(&w, &f, 4);
    const uint8_t sign = (uint8_t)((w >> 24) & 0x80u);
    uint32_t a = w & 0x7fffffffu;
    if (a > 0x7f800000u) return (uint8_t)(sign | 0x7fu);                    // NaN
    if (a == 0x7f800000u) return (uint8_t)(sign | (E5M2 ? 0x7cu : 0x7fu));  // Inf: e4m3 has none
    if (a > kMaxF32) a = kMaxF32;                                           // saturate to finite
    constexpr int sh = 23 - kMan;
    if (a >= ((uint32_t)(128 - kBias) << 23)) {  // a normal FP8 value (>= 2^(1 - bias)); a carry out of the
                                                 // mantissa moves into the exponent, never past the maximum
      const uint32_t r = a - ((uint32_t)(127 - kBias) << 23) + ((1u << (sh - 1)) - 1u) + ((a >> sh) & 1u);
      return (uint8_t)(sign | (r >> sh));
    }
    // below half the smallest subnormal, 2^(-bias - man): zero (the half itself ties to even, zero)
    if (a < ((uint32_t)(127 - kBias - kMan) << 23)) return sign;
    // subnormal: the 24-bit significand shifted down to units of 2^(1 - bias - man)
    const uint32_t e = a >> 23, sig = (a & 0x7fffffu) | 0x800000u;
    const uint32_t shift = 151u - kBias - kMan - e;  // 21..24 (e4m3), 22..24 (e5m2)
    const uint32_t q = sig >> shift, rem = sig & ((1u << shift) - 1u), half = 1u << (shift - 1);
    return (uint8_t)(sign | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u)));
  }
};
typedef fp8<false> f8e4m3;
typedef fp8<true> f8e5m2;
static_assert(sizeof(f8e4m3) == 1 && sizeof(f8e5m2) == 1, "fp8 storage");

// The finishing step of a scaled sum (Compute<T>::set_scale; the C ABI's
// hiccl_reduce_scaled): f64 one multiply by alpha; f32 one multiply by a32 =
// (float)alpha; bf16 / f16 widen (exact), multiply in f32 ROUNDED TO F32, then
// round to nearest even to T -- two roundings, by definition.  `volatile`
// keeps the f32 product a rounded float on hosts that evaluate in a wider
// format.
template <typename T>
inline T scale_finish(T s, double alpha) {
  if constexpr (std::is_same<T, double>::value) {
    return s * alpha;
  } else {
    volatile float p = (float)s * (float)alpha;
    return (T)p;
  }
}

// The element types a widened sum reads (WidenCompute<T>, compute.h; the C
// ABI's hiccl_reduce_widened): the 2-byte and 1-byte floating types.
template <typename T>
constexpr bool widenable() {
  return std::is_same<T, bf16>::value || std::is_same<T, f16>::value || std::is_same<T, f8e4m3>::value ||
         std::is_same<T, f8e5m2>::value
#ifdef __FLT16_MANT_DIG__
         || std::is_same<T, _Float16>::value
#endif
      ;
}

// One element of a widened sum, the host port's arithmetic: widen every input
// through its `operator float` (exact), add in f32 in list order from +0, and
// for a scaled sum multiply once by (float)alpha (scale_finish<float>).
// `volatile` keeps every partial sum a rounded float on hosts that evaluate in
// a wider format.
template <typename T>
inline float widen_sum(T *const *in, int k, size_t i, bool scaled, double alpha) {
  static_assert(widenable<T>(), "HiCCL::widen_sum: bf16, f16 (_Float16), f8e4m3 or f8e5m2 inputs only");
  volatile float acc = 0.0f;
  for (int j = 0; j < k; j++) acc = acc + (float)in[j][i];
  return scaled ? scale_finish<float>(acc, alpha) : (float)acc;
}

// One element of a WEIGHTED widened sum: input j counts as fl32(w[j] *
// widen(in[j][i])), a product rounded to f32 -- it goes into a volatile float
// in a statement of its own, so a contracting compiler cannot fuse it with the
// add that follows (a fused multiply-add rounds once: another word).
template <typename T>
inline float weighted_widen_sum(T *const *in, const float *w, int k, size_t i, bool scaled, double alpha) {
  static_assert(widenable<T>(), "HiCCL::weighted_widen_sum: bf16, f16 (_Float16), f8e4m3 or f8e5m2 inputs only");
  volatile float acc = 0.0f;
  for (int j = 0; j < k; j++) {
    volatile float t = w[j] * (float)in[j][i];
    acc = acc + t;
  }
  return scaled ? scale_finish<float>(acc, alpha) : (float)acc;
}

}  // namespace HiCCL

#endif  // HICCL_ELEM_TYPES_H
