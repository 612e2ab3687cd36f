// include/hiccl/ops.h -- HiCCL::maxof<U>, minof<U>, prodof<U>, bandof<U>,
// borof<U> and bxorof<U>: element types whose `+=` is a maximum, a minimum, a
// product or a bitwise AND / OR / XOR.
//
// The reduction is a template over T, `T acc = 0; acc += x` (the reference's
// reduce_kernel, source/compute.h:2-23), so another reduction is a type whose
// T(0) is the operator's identity and whose `+=` is the operator.  These
// wrappers are such types, and Comm<maxof<float>> / Compute<minof<bf16>> run
// them (and Comm<prodof<float>>, Comm<bxorof<uint64_t>>, ...): on the host
// port through `+=` itself, on the GPU through the operator's kernels
// (hiccl_op_t in include/hiccl_reduce.h; dtype_of<maxof<U>>() is
// dtype_of<U>() and op_of<maxof<U>>() is HICCL_OP_MAX).  The wrappers are
// plain C++ and depend on nothing else here, so the same Comm<maxof<float>>
// source compiles against the reference once it is given this struct.
//
// Semantics:
//   float, double, bf16, f16, _Float16   IEEE 754-2019 maximum / minimum: a
//       NaN operand gives NaN, -0 < +0, subnormals are kept, nothing rounds;
//       identity -Inf (maxof) / +Inf (minof).
//   f8e4m3, f8e5m2 (maxof / minof only)   the same maximum / minimum; identity
//       -Inf / +Inf for e5m2, -448 / +448 (0xfe / 0x7e) for e4m3, which has
//       no infinity.  prodof and the bitwise wrappers of them do not compile.
//   signed 4-byte integers     signed compare, INT32_MIN / INT32_MAX.
//   unsigned 8-byte integers   unsigned compare, 0 / UINT64_MAX.
// prodof (identity 1): float, double, _Float16 -- one multiply in U per `+=`;
//       bf16, f16 -- widen, one f32 multiply, round once to nearest even
//       (f16: the half multiply's bits); 4- and 8-byte integers of either
//       signedness -- wrap-around multiply, done in unsigned.
// bandof / borof / bxorof (identities all-ones / 0 / 0): 4- and 8-byte
//       integers of either signedness only.
// Included by compute.h.
#ifndef HICCL_OPS_H
#define HICCL_OPS_H

#include <cmath>
#include <cstdint>
#include <limits>
#include <type_traits>

#include "elem_types.h"

namespace HiCCL {

namespace ops_detail {

// the two 2-byte storage structs: ordered through their bit patterns
template <class U> struct half_bits : std::false_type {};
template <> struct half_bits<bf16> : std::true_type { static constexpr uint16_t inf = 0x7f80u; };
template <> struct half_bits<f16> : std::true_type { static constexpr uint16_t inf = 0x7c00u; };

// the two 1-byte storage structs (OCP FP8): ordered through their bit patterns
// too.  e5m2's identities are its infinities; e4m3fn has none and takes its
// largest finite values, -448 (0xfe) for a maximum and +448 (0x7e) for a minimum.
template <class U> struct f8_bits : std::false_type {};
template <> struct f8_bits<f8e4m3> : std::true_type { static constexpr uint8_t top = 0x7eu; };
template <> struct f8_bits<f8e5m2> : std::true_type { static constexpr uint8_t top = 0x7cu; };

template <class U>
constexpr bool is_float_like() {
#ifdef __FLT16_MANT_DIG__
  if (std::is_same<U, _Float16>::value) return true;
#endif
  return std::is_floating_point<U>::value;
}

// the operator a wrapper folds with; its value is the hiccl_op_t
enum class tag : int { max = 1, min = 2, prod = 16, band = 17, bor = 18, bxor = 19 };

constexpr bool is_bitwise(tag OP) { return OP == tag::band || OP == tag::bor || OP == tag::bxor; }

template <tag OP, class U>
U identity() {
  if constexpr (OP == tag::prod) {
    if constexpr (half_bits<U>::value) return U(1.0f);
    else return (U)1;
  } else if constexpr (is_bitwise(OP)) {
    return OP == tag::band ? (U) ~(U)0 : (U)0;
  } else {
    constexpr bool MAX = OP == tag::max;
    if constexpr (half_bits<U>::value) {
      U r;
      r.bits = (uint16_t)(half_bits<U>::inf | (MAX ? 0x8000u : 0u));
      return r;
    } else if constexpr (f8_bits<U>::value) {
      U r;
      r.bits = (uint8_t)(f8_bits<U>::top | (MAX ? 0x80u : 0u));
      return r;
    } else if constexpr (std::is_integral<U>::value) {
      return MAX ? std::numeric_limits<U>::min() : std::numeric_limits<U>::max();
    } else {
      const float inf = std::numeric_limits<float>::infinity();
      return (U)(MAX ? -inf : inf);
    }
  }
}

// sign-magnitude pattern -> an integer ordered like the value (-0 below +0)
inline int half_key(uint16_t bits) {
  const int mag = bits & 0x7fff;
  return (bits & 0x8000u) ? -mag - 1 : mag;
}

inline int f8_key(uint8_t bits) {
  const int mag = bits & 0x7f;
  return (bits & 0x80u) ? -mag - 1 : mag;
}

template <bool MAX, class U>
U fold_mm(U a, U b) {
  if constexpr (half_bits<U>::value) {
    if ((a.bits & 0x7fffu) > half_bits<U>::inf) return a;  // NaN
    if ((b.bits & 0x7fffu) > half_bits<U>::inf) return b;
    const int ka = half_key(a.bits), kb = half_key(b.bits);
    return MAX ? (ka < kb ? b : a) : (kb < ka ? b : a);
  } else if constexpr (f8_bits<U>::value) {
    if (a.isnan()) return a;
    if (b.isnan()) return b;
    const int ka = f8_key(a.bits), kb = f8_key(b.bits);
    return MAX ? (ka < kb ? b : a) : (kb < ka ? b : a);
  } else if constexpr (std::is_integral<U>::value) {
    return MAX ? (a < b ? b : a) : (b < a ? b : a);
  } else {
    if (a != a) return a;  // NaN
    if (b != b) return b;
    if (a == b) {  // equal values, or zeros of either sign: -0 < +0
      const bool neg_a = std::signbit((double)a);
      return MAX ? (neg_a ? b : a) : (neg_a ? a : b);
    }
    return MAX ? (a < b ? b : a) : (b < a ? b : a);
  }
}

template <tag OP, class U>
U fold(U a, U b) {
  if constexpr (OP == tag::prod) {
    if constexpr (half_bits<U>::value) {
      // widen (exact), one f32 multiply, round once to U: bf16's definition,
      // and for f16 the half multiply itself (the product of two 11-bit
      // significands is exact in f32)
      U r;
      r.bits = U::round((float)a * (float)b);
      return r;
    } else if constexpr (std::is_integral<U>::value) {
      typedef typename std::make_unsigned<U>::type W;  // wrap-around: a signed overflow is undefined
      return (U)((W)a * (W)b);
    } else {
      return (U)(a * b);
    }
  } else if constexpr (is_bitwise(OP)) {
    typedef typename std::make_unsigned<U>::type W;
    const W x = (W)a, y = (W)b;
    return (U)(OP == tag::band ? (W)(x & y) : OP == tag::bor ? (W)(x | y) : (W)(x ^ y));
  } else {
    return fold_mm<OP == tag::max, U>(a, b);
  }
}

template <tag OP, class U>
struct wrap {
  typedef U value_type;
  static constexpr int hiccl_op = (int)OP;  // HICCL_OP_MAX ... HICCL_OP_BXOR
  static constexpr bool kMM = OP == tag::max || OP == tag::min;
  static_assert(half_bits<U>::value || f8_bits<U>::value || is_float_like<U>() || std::is_integral<U>::value,
                "HiCCL::maxof / minof / prodof: U must be float, double, bf16, f16, int32 or uint64 "
                "(maxof / minof: f8e4m3 and f8e5m2 too)");
  static_assert(kMM || !f8_bits<U>::value,
                "HiCCL::prodof / bandof / borof / bxorof: the FP8 types (f8e4m3, f8e5m2) have a sum, a maximum "
                "and a minimum only");
  // dtype_of maps every 8-byte integer to HICCL_UINT64 (sums, products and
  // the bitwise operators wrap alike) and every 4-byte integer to
  // HICCL_INT32; a maximum is not sign-agnostic
  static_assert(!std::is_integral<U>::value || sizeof(U) == 4 || sizeof(U) == 8,
                "HiCCL operator wrappers: integers of 4 or 8 bytes only");
  static_assert(!is_bitwise(OP) || std::is_integral<U>::value,
                "HiCCL::bandof / borof / bxorof: integers of 4 or 8 bytes only");
  static_assert(!kMM || !std::is_integral<U>::value || sizeof(U) != 8 || std::is_unsigned<U>::value,
                "HiCCL::maxof / minof: 8-byte integers run as HICCL_UINT64, which compares UNSIGNED: "
                "a signed 8-byte type would order negative values above positive ones");
  static_assert(!kMM || !std::is_integral<U>::value || sizeof(U) != 4 || std::is_signed<U>::value,
                "HiCCL::maxof / minof: 4-byte integers run as HICCL_INT32, which compares SIGNED: "
                "an unsigned 4-byte type would order values above INT32_MAX below zero");
  U v;  // the value (public, as bf16's bits: a buffer of U is a buffer of wrap<U>)
  wrap() = default;
  wrap(int) : v(identity<OP, U>()) {}  // T acc = 0: the identity, whatever the int
  wrap &operator+=(wrap o) {
    v = fold<OP, U>(v, o.v);
    return *this;
  }
  bool operator==(wrap o) const { return v == o.v; }
  bool operator!=(wrap o) const { return !(v == o.v); }
};

}  // namespace ops_detail

// name<U>: wrap<TAG, U> under a public name of its own
#define HICCL_OP_WRAPPER(name, TAG)                                            \
  template <class U> struct name : ops_detail::wrap<ops_detail::tag::TAG, U> { \
    using ops_detail::wrap<ops_detail::tag::TAG, U>::wrap;                     \
    name() = default;                                                          \
  }
HICCL_OP_WRAPPER(maxof, max);
HICCL_OP_WRAPPER(minof, min);
HICCL_OP_WRAPPER(prodof, prod);
HICCL_OP_WRAPPER(bandof, band);
HICCL_OP_WRAPPER(borof, bor);
HICCL_OP_WRAPPER(bxorof, bxor);
#undef HICCL_OP_WRAPPER

// the wrapped type of an operator wrapper (T itself otherwise), and its op
template <class T> struct op_traits { typedef T value_type; static constexpr int op = 0; };
template <class U> struct op_traits<maxof<U>> { typedef U value_type; static constexpr int op = 1; };
template <class U> struct op_traits<minof<U>> { typedef U value_type; static constexpr int op = 2; };
template <class U> struct op_traits<prodof<U>> { typedef U value_type; static constexpr int op = 16; };
template <class U> struct op_traits<bandof<U>> { typedef U value_type; static constexpr int op = 17; };
template <class U> struct op_traits<borof<U>> { typedef U value_type; static constexpr int op = 18; };
template <class U> struct op_traits<bxorof<U>> { typedef U value_type; static constexpr int op = 19; };

// T -> hiccl_op_t
template <typename T>
constexpr int op_of() { return op_traits<T>::op; }

}  // namespace HiCCL

#endif  // HICCL_OPS_H
