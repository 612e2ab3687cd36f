// include/hiccl/ops.h -- HiCCL::maxof<U> and HiCCL::minof<U>: element types
// whose `+=` is a maximum or a minimum.
//
// The reduction is a template over T, `T acc = 0; acc += x` (the reference's
// reduce_kernel, source/compute.h:2-23), so another reduction is a type whose
// T(0) is the operator's identity and whose `+=` is the operator.  These two
// wrappers are such types, and Comm<maxof<float>> / Compute<minof<bf16>> run
// them: on the host port through `+=` itself, on the GPU through the MAX / MIN
// kernels (hiccl_op_t in include/hiccl_reduce.h; dtype_of<maxof<U>>() is
// dtype_of<U>() and op_of<maxof<U>>() is HICCL_OP_MAX).  The wrappers are
// plain C++ and depend on nothing else here, so the same Comm<maxof<float>>
// source compiles against the reference once it is given this struct.
//
// Semantics:
//   float, double, bf16, f16, _Float16   IEEE 754-2019 maximum / minimum: a
//       NaN operand gives NaN, -0 < +0, subnormals are kept, nothing rounds;
//       identity -Inf (maxof) / +Inf (minof).
//   signed 4-byte integers     signed compare, INT32_MIN / INT32_MAX.
//   unsigned 8-byte integers   unsigned compare, 0 / UINT64_MAX.
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

template <class U>
constexpr bool is_float_like() {
#ifdef __FLT16_MANT_DIG__
  if (std::is_same<U, _Float16>::value) return true;
#endif
  return std::is_floating_point<U>::value;
}

template <bool MAX, class U>
U identity() {
  if constexpr (half_bits<U>::value) {
    U r;
    r.bits = (uint16_t)(half_bits<U>::inf | (MAX ? 0x8000u : 0u));
    return r;
  } else if constexpr (std::is_integral<U>::value) {
    return MAX ? std::numeric_limits<U>::min() : std::numeric_limits<U>::max();
  } else {
    const float inf = std::numeric_limits<float>::infinity();
    return (U)(MAX ? -inf : inf);
  }
}

// sign-magnitude pattern -> an integer ordered like the value (-0 below +0)
inline int half_key(uint16_t bits) {
  const int mag = bits & 0x7fff;
  return (bits & 0x8000u) ? -mag - 1 : mag;
}

template <bool MAX, class U>
U fold(U a, U b) {
  if constexpr (half_bits<U>::value) {
    if ((a.bits & 0x7fffu) > half_bits<U>::inf) return a;  // NaN
    if ((b.bits & 0x7fffu) > half_bits<U>::inf) return b;
    const int ka = half_key(a.bits), kb = half_key(b.bits);
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

template <bool MAX, class U>
struct wrap {
  typedef U value_type;
  static constexpr int hiccl_op = MAX ? 1 : 2;  // HICCL_OP_MAX / HICCL_OP_MIN
  static_assert(half_bits<U>::value || is_float_like<U>() || std::is_integral<U>::value,
                "HiCCL::maxof / minof: U must be float, double, bf16, f16, int32 or uint64");
  // dtype_of maps every 8-byte integer to HICCL_UINT64 (sums wrap alike) and
  // every 4-byte integer to HICCL_INT32; a maximum is not sign-agnostic
  static_assert(!std::is_integral<U>::value || sizeof(U) == 4 || sizeof(U) == 8,
                "HiCCL::maxof / minof: integers of 4 or 8 bytes only");
  static_assert(!std::is_integral<U>::value || sizeof(U) != 8 || std::is_unsigned<U>::value,
                "HiCCL::maxof / minof: 8-byte integers run as HICCL_UINT64, which compares UNSIGNED: "
                "a signed 8-byte type would order negative values above positive ones");
  static_assert(!std::is_integral<U>::value || sizeof(U) != 4 || std::is_signed<U>::value,
                "HiCCL::maxof / minof: 4-byte integers run as HICCL_INT32, which compares SIGNED: "
                "an unsigned 4-byte type would order values above INT32_MAX below zero");
  U v;  // the value (public, as bf16's bits: a buffer of U is a buffer of wrap<U>)
  wrap() = default;
  wrap(int) : v(identity<MAX, U>()) {}  // T acc = 0: the identity, whatever the int
  wrap &operator+=(wrap o) {
    v = fold<MAX, U>(v, o.v);
    return *this;
  }
  bool operator==(wrap o) const { return v == o.v; }
  bool operator!=(wrap o) const { return !(v == o.v); }
};

}  // namespace ops_detail

template <class U> struct maxof : ops_detail::wrap<true, U> {
  using ops_detail::wrap<true, U>::wrap;
  maxof() = default;
};
template <class U> struct minof : ops_detail::wrap<false, U> {
  using ops_detail::wrap<false, U>::wrap;
  minof() = default;
};

// the wrapped type of an operator wrapper (T itself otherwise), and its op
template <class T> struct op_traits { typedef T value_type; static constexpr int op = 0; };
template <class U> struct op_traits<maxof<U>> { typedef U value_type; static constexpr int op = 1; };
template <class U> struct op_traits<minof<U>> { typedef U value_type; static constexpr int op = 2; };

// T -> hiccl_op_t
template <typename T>
constexpr int op_of() { return op_traits<T>::op; }

}  // namespace HiCCL

#endif  // HICCL_OPS_H
