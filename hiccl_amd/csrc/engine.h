// hiccl_amd/csrc/engine.h -- the device code every kernel translation unit
// shares: the element ops, the TILE and PHASE engines, the unit schedules, the
// one-shot / plan / program kernels and their instantiation tables.
//
// The library's kernels are compiled as five translation units that run side
// by side in the build: reduce.hip instantiates the tables for the SUM ops
// (kPartSum), reduce_ops.hip for the MAX / MIN ops (kPartMaxMin),
// reduce_prod.hip for PROD and the bitwise ops (kPartProd),
// reduce_scale.hip for the post-scaled sums (kPartScale), reduce_f8.hip
// for every op of the two OCP FP8 types (kPartF8), reduce_widen.hip for the
// widened sums (kPartWiden), reduce_accum.hip for the accumulating widened
// sums (kPartAccum) and reduce_mixed.hip for the mixed plan kernels
// (kPartMixed; the last four are included from reduce_scale.hip).  All
// take their ops from the one list below (with_elem<PART>), so a type or an
// operator is still added in one place.  Everything here is in an anonymous
// namespace: a kernel belongs to the unit that instantiates it.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <limits>
#include <type_traits>

#include "../../include/hiccl_reduce.h"
#include "kernels.h"

using namespace hiccl_impl;

namespace {

// ------------------------------------------------------------ vector types --

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// 16-byte packet type with 1-byte alignment: a misaligned input still loads
// as one global_load_dwordx4 (gfx950 unaligned access mode).
typedef uint32_t u32x4u __attribute__((ext_vector_type(4), aligned(1)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// Buffer resources: one SGPR descriptor per input per tile (base = input +
// tile offset, range = the tile's valid bytes).  Loads/stores then take only
// the tile-invariant 32-bit lane offset, and the hardware range check turns
// the lanes past the end of the last (partial) tile into no-ops.
typedef __amdgpu_buffer_rsrc_t rsrc_t;
constexpr int kRsrcFlags = 0x00020000;  // raw buffer, 32-bit data format

__device__ __forceinline__ rsrc_t make_rsrc(const char *base, uint32_t nbytes) {
  return __builtin_amdgcn_make_buffer_rsrc((void *)base, (short)0, (int)nbytes, kRsrcFlags);
}

// Cache policy POL = 10*store + load: kernels.h.
template <int POL>
__device__ __forceinline__ u32x4 load_pkt(rsrc_t r, uint32_t voff) {
  constexpr int lp = POL % 10;
  return __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, 0, lp == 1 ? 2 : lp == kPolLoadSys ? 17 : 0);
}

// The narrow input packets of the widened sums (four elements: 8 B of a
// 2-byte type, 4 B of FP8), under the same load policies.
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <int POL>
__device__ __forceinline__ u32x2 load_pkt_b64(rsrc_t r, uint32_t voff) {
  constexpr int lp = POL % 10;
  return __builtin_amdgcn_raw_buffer_load_b64(r, (int)voff, 0, lp == 1 ? 2 : lp == kPolLoadSys ? 17 : 0);
}

template <int POL>
__device__ __forceinline__ uint32_t load_pkt_b32(rsrc_t r, uint32_t voff) {
  constexpr int lp = POL % 10;
  return __builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, 0, lp == 1 ? 2 : lp == kPolLoadSys ? 17 : 0);
}

template <int POL>
__device__ __forceinline__ void store_pkt(rsrc_t r, uint32_t voff, u32x4 v) {
  constexpr int sp = POL / 10;
  __builtin_amdgcn_raw_buffer_store_b128(v, r, (int)voff, 0, sp == 1 ? 2 : sp == 2 ? 16 : sp == kPolStoreSys ? 17 : 0);
}

// bf16 <-> f32.  f32 -> bf16 is round-to-nearest-even; on gfx950 the cast
// lowers to v_cvt_pk_bf16_f32, which keeps a NaN a NaN.
__device__ __forceinline__ float bf_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }
__device__ __forceinline__ uint32_t bf_pack(float lo, float hi) {
  bf16x2 v = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(uint32_t, v);
}
__device__ __forceinline__ uint16_t bf_round(float f) {
  return __builtin_bit_cast(uint16_t, (__bf16)f);
}

// Scalar head/tail accesses through the GLOBAL address space: a generic
// pointer becomes a flat access, and a flat load pending anywhere inside the
// plan kernel's unit loop makes the waitcnt pass treat vmcnt as out of order
// -- every tile's adds then waited with vmcnt(0) instead of a staircase.
template <class T>
__device__ __forceinline__ T gld(const char *p) {
  return *(const __attribute__((address_space(1))) T *)p;
}
template <class T>
__device__ __forceinline__ void gst(char *p, T v) {
  *(__attribute__((address_space(1))) T *)p = v;
}

// ------------------------------------------------------------ element ops --
// Each op: elem size, packet accumulator (acc_t) with zero/add/pack, and a
// scalar accumulator for the peeled head/tail elements.  zero() + x keeps the
// reference's `T acc = 0; acc += x` (so -0 inputs sum to +0).

struct OpF32 {
  static constexpr bool kWidens = false;
  static constexpr int kEsz = 4;
  typedef f32x4 acc_t;
  __device__ static acc_t zero() { return (f32x4)(0.0f); }
  __device__ static acc_t add(acc_t a, u32x4 p) { return a + __builtin_bit_cast(f32x4, p); }
  __device__ static u32x4 pack(acc_t a) { return __builtin_bit_cast(u32x4, a); }
  typedef float sacc_t;
  __device__ static sacc_t szero() { return 0.0f; }
  __device__ static sacc_t sadd(sacc_t a, const char *p) { return a + gld<float>(p); }
  __device__ static void sstore(char *p, sacc_t a) { gst<float>(p, a); }
};

struct OpF64 {
  static constexpr bool kWidens = false;
  static constexpr int kEsz = 8;
  typedef f64x2 acc_t;
  __device__ static acc_t zero() { return (f64x2)(0.0); }
  __device__ static acc_t add(acc_t a, u32x4 p) { return a + __builtin_bit_cast(f64x2, p); }
  __device__ static u32x4 pack(acc_t a) { return __builtin_bit_cast(u32x4, a); }
  typedef double sacc_t;
  __device__ static sacc_t szero() { return 0.0; }
  __device__ static sacc_t sadd(sacc_t a, const char *p) { return a + gld<double>(p); }
  __device__ static void sstore(char *p, sacc_t a) { gst<double>(p, a); }
};

struct OpU64 {
  static constexpr bool kWidens = false;
  static constexpr int kEsz = 8;
  typedef u64x2 acc_t;
  __device__ static acc_t zero() { return (u64x2)(0); }
  __device__ static acc_t add(acc_t a, u32x4 p) { return a + __builtin_bit_cast(u64x2, p); }
  __device__ static u32x4 pack(acc_t a) { return __builtin_bit_cast(u32x4, a); }
  typedef uint64_t sacc_t;
  __device__ static sacc_t szero() { return 0; }
  __device__ static sacc_t sadd(sacc_t a, const char *p) { return a + gld<uint64_t>(p); }
  __device__ static void sstore(char *p, sacc_t a) { gst<uint64_t>(p, a); }
};

struct OpI32 {  // two's-complement wrap-around, done in unsigned
  static constexpr bool kWidens = false;
  static constexpr bool kHalfChunk = true;  // phase_p_of
  static constexpr int kEsz = 4;
  typedef u32x4 acc_t;
  __device__ static acc_t zero() { return (u32x4)(0u); }
  __device__ static acc_t add(acc_t a, u32x4 p) { return a + p; }
  __device__ static u32x4 pack(acc_t a) { return a; }
  typedef uint32_t sacc_t;
  __device__ static sacc_t szero() { return 0u; }
  __device__ static sacc_t sadd(sacc_t a, const char *p) { return a + gld<uint32_t>(p); }
  __device__ static void sstore(char *p, sacc_t a) { gst<uint32_t>(p, a); }
};

// bf16, reference semantics: acc is bf16, every add = f32 add then round to
// bf16.  The accumulator is kept PACKED (8 bf16 in a u32x4, the packet's own
// layout): widen both operands (exact), add in f32, round-to-nearest-even
// back (v_cvt_pk_bf16_f32).  4 VGPRs per packet, so the phased engine runs
// bf16 at the same 128 KiB chunk as f32.
// The pack is an opaque v_cvt_pk_bf16_f32 (the same instruction the __bf16
// casts lower to) so the compiler cannot see through pack->widen and keep the
// accumulator widened in 8 VGPRs per packet (it does, and spills).
__device__ __forceinline__ uint32_t bf_pack_opaque(float lo, float hi) {
  uint32_t r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

struct OpBF16 {
  static constexpr bool kWidens = true;
  static constexpr int kEsz = 2;
  typedef u32x4 acc_t;
  __device__ static acc_t zero() { return (u32x4)(0u); }  // +0 bf16
  __device__ static acc_t add(acc_t a, u32x4 p) {
    acc_t r;
#pragma unroll
    for (int w = 0; w < 4; w++)
      r[w] = bf_pack_opaque(bf_lo(a[w]) + bf_lo(p[w]), bf_hi(a[w]) + bf_hi(p[w]));
    return r;
  }
  __device__ static u32x4 pack(acc_t a) { return a; }
  typedef float sacc_t;
  __device__ static sacc_t szero() { return 0.0f; }
  __device__ static sacc_t sadd(sacc_t a, const char *p) {
    float s = a + __uint_as_float((uint32_t)(gld<uint16_t>(p)) << 16);
    return __uint_as_float((uint32_t)bf_round(s) << 16);
  }
  __device__ static void sstore(char *p, sacc_t a) { gst<uint16_t>(p, bf_round(a)); }
};

// bf16 inputs, f32 accumulator, one rounding at the end (HICCL_ACC_WIDE).
struct OpBF16Wide {
  static constexpr bool kWidens = true;
  static constexpr int kEsz = 2;
  typedef f32x8 acc_t;
  __device__ static acc_t zero() { return (f32x8)(0.0f); }
  __device__ static acc_t add(acc_t a, u32x4 p) {
#pragma unroll
    for (int w = 0; w < 4; w++) {
      a[2 * w] += bf_lo(p[w]);
      a[2 * w + 1] += bf_hi(p[w]);
    }
    return a;
  }
  __device__ static u32x4 pack(acc_t a) {
    u32x4 r;
#pragma unroll
    for (int w = 0; w < 4; w++) r[w] = bf_pack(a[2 * w], a[2 * w + 1]);
    return r;
  }
  typedef float sacc_t;
  __device__ static sacc_t szero() { return 0.0f; }
  __device__ static sacc_t sadd(sacc_t a, const char *p) {
    return a + __uint_as_float((uint32_t)(gld<uint16_t>(p)) << 16);
  }
  __device__ static void sstore(char *p, sacc_t a) { gst<uint16_t>(p, bf_round(a)); }
};

// fp16 (IEEE half), reference semantics: acc is half and every add is a half
// add.  gfx950 has that add natively -- one v_pk_add_f16 adds two elements,
// rounded to nearest even, subnormals kept (the code object's 16-bit denorm
// mode) -- so the accumulator stays in the packet's own layout (4 VGPRs) and
// an add costs four instructions per packet, with no widen / round pair.
typedef _Float16 half_t;
__device__ __forceinline__ half_t f16_ld(const char *p) { return __builtin_bit_cast(half_t, gld<uint16_t>(p)); }
__device__ __forceinline__ float f16_widen(uint32_t w, int hi) {
  return (float)__builtin_bit_cast(f16x2, w)[hi];
}
// f32 -> half is round-to-nearest-even (v_cvt_f16_f32); overflow gives Inf
// and a NaN stays a NaN.
__device__ __forceinline__ uint16_t f16_round(float f) { return __builtin_bit_cast(uint16_t, (half_t)f); }

struct OpF16 {
  static constexpr bool kWidens = false;
  static constexpr int kEsz = 2;
  typedef f16x8 acc_t;
  __device__ static acc_t zero() { return (f16x8)((half_t)0.0f); }  // +0
  __device__ static acc_t add(acc_t a, u32x4 p) { return a + __builtin_bit_cast(f16x8, p); }
  __device__ static u32x4 pack(acc_t a) { return __builtin_bit_cast(u32x4, a); }
  typedef half_t sacc_t;
  __device__ static sacc_t szero() { return (half_t)0.0f; }
  __device__ static sacc_t sadd(sacc_t a, const char *p) { return a + f16_ld(p); }
  __device__ static void sstore(char *p, sacc_t a) { gst<uint16_t>(p, __builtin_bit_cast(uint16_t, a)); }
};

// fp16 inputs, f32 accumulator, one rounding at the end (HICCL_ACC_WIDE): a
// sequential f32 sum in input order from +0, NOT reference-bitwise.
struct OpF16Wide {
  static constexpr bool kWidens = true;
  static constexpr int kEsz = 2;
  typedef f32x8 acc_t;
  __device__ static acc_t zero() { return (f32x8)(0.0f); }
  __device__ static acc_t add(acc_t a, u32x4 p) {
#pragma unroll
    for (int w = 0; w < 4; w++) {
      a[2 * w] += f16_widen(p[w], 0);
      a[2 * w + 1] += f16_widen(p[w], 1);
    }
    return a;
  }
  __device__ static u32x4 pack(acc_t a) {
    u32x4 r;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      f16x2 v = {(half_t)a[2 * w], (half_t)a[2 * w + 1]};
      r[w] = __builtin_bit_cast(uint32_t, v);
    }
    return r;
  }
  typedef float sacc_t;
  __device__ static sacc_t szero() { return 0.0f; }
  __device__ static sacc_t sadd(sacc_t a, const char *p) { return a + (float)f16_ld(p); }
  __device__ static void sstore(char *p, sacc_t a) { gst<uint16_t>(p, f16_round(a)); }
};

// Exact byte copy (HICCL_BYTES): one input, out = in[0] bit for bit.  The
// transport's batched data movement runs on the same tile engine.
struct OpRaw {
  static constexpr bool kWidens = false;
  static constexpr int kEsz = 1;
  typedef u32x4 acc_t;
  __device__ static acc_t zero() { return (u32x4)(0u); }
  __device__ static acc_t add(acc_t, u32x4 p) { return p; }
  __device__ static u32x4 pack(acc_t a) { return a; }
  typedef uint8_t sacc_t;
  __device__ static sacc_t szero() { return 0; }
  __device__ static sacc_t sadd(sacc_t, const char *p) { return gld<uint8_t>(p); }
  __device__ static void sstore(char *p, sacc_t a) { gst<uint8_t>(p, a); }
};

// --------------------------------------------------------- MAX / MIN ops --
// The same struct shape as the SUM ops; zero() is the operator's identity
// (-Inf / +Inf, INT32_MIN / INT32_MAX, 0 / UINT64_MAX) and add() the
// operator, so the engines fold `acc = id; acc = op(acc, in[k])` in list
// order.  The floating types follow IEEE 754-2019 maximum / minimum: a NaN
// operand gives NaN, -0 < +0, subnormals are kept, nothing is rounded.
// gfx950 has these as three-operand instructions (v_maximum3_f32,
// v_pk_maximum3_f16 and the minimum forms): two chained add()s of a group
// become one instruction per register.  Every accumulator is a packet
// (4 VGPRs).
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

template <bool MAX, class V>
__device__ __forceinline__ V fmm(V a, V b) {  // floating, scalar or vector
  if constexpr (MAX) return __builtin_elementwise_maximum(a, b);
  else return __builtin_elementwise_minimum(a, b);
}
template <bool MAX, class V>
__device__ __forceinline__ V imm(V a, V b) {  // integer, scalar or vector
  if constexpr (MAX) return __builtin_elementwise_max(a, b);
  else return __builtin_elementwise_min(a, b);
}

// f32, f64, f16: the packet is a vector of T and so is the accumulator.
template <bool MAX, class T, class VT>
struct OpFloatMM {
  static constexpr bool kWidens = false;
  static constexpr bool kPinAcc = true;  // exact, so re-associable: chunk_body
  static constexpr int kEsz = sizeof(T);
  static constexpr T kId = MAX ? -__builtin_huge_val() : __builtin_huge_val();
  typedef VT acc_t;
  __device__ static acc_t zero() { return (VT)(kId); }
  __device__ static acc_t add(acc_t a, u32x4 p) { return fmm<MAX>(a, __builtin_bit_cast(VT, p)); }
  __device__ static u32x4 pack(acc_t a) { return __builtin_bit_cast(u32x4, a); }
  typedef T sacc_t;
  __device__ static sacc_t szero() { return kId; }
  __device__ static sacc_t sadd(sacc_t a, const char *p) { return fmm<MAX>(a, gld<T>(p)); }
  __device__ static void sstore(char *p, sacc_t a) { gst<T>(p, a); }
};

// bf16: a bf16 is the top half of an f32, so both halves of a word are
// widened (exact), compared in f32 and the winners' top halves put back
// together -- nothing rounds.  The accumulator is kept PACKED, as OpBF16's:
// the repack is an opaque v_perm_b32, so the compiler cannot see through
// pack -> widen and carry 8 VGPRs per packet from add to add.
__device__ __forceinline__ uint32_t bf_join_opaque(float lo, float hi) {
  uint32_t r;  // bytes {hi.3, hi.2, lo.3, lo.2}
  asm("v_perm_b32 %0, %1, %2, %3" : "=v"(r) : "v"(hi), "v"(lo), "s"(0x07060302u));
  return r;
}

template <bool MAX>
struct OpBF16MM {
  static constexpr bool kWidens = true;
  static constexpr int kEsz = 2;
  static constexpr uint32_t kIdBits = MAX ? 0xff80u : 0x7f80u;  // -Inf / +Inf
  typedef u32x4 acc_t;
  __device__ static acc_t zero() { return (u32x4)(kIdBits << 16 | kIdBits); }
  // The tile engine's accumulators start from a scalar register instead (see
  // tile_zero): a literal that is not an inline constant gets hoisted out of
  // the unit loop into a VGPR that then lives through every tile -- one VGPR
  // more than OpBF16, whose +0 is an inline constant.
  __device__ static acc_t tile_zero() {
    uint32_t k;
    asm("s_mov_b32 %0, %1" : "=s"(k) : "i"(kIdBits << 16 | kIdBits));
    return (u32x4)(k);
  }
  __device__ static acc_t add(acc_t a, u32x4 p) {
    acc_t r;
#pragma unroll
    for (int w = 0; w < 4; w++)
      r[w] = bf_join_opaque(fmm<MAX>(bf_lo(a[w]), bf_lo(p[w])), fmm<MAX>(bf_hi(a[w]), bf_hi(p[w])));
    return r;
  }
  __device__ static u32x4 pack(acc_t a) { return a; }
  typedef float sacc_t;  // a widened bf16: the low half stays zero
  __device__ static sacc_t szero() { return __uint_as_float(kIdBits << 16); }
  __device__ static sacc_t sadd(sacc_t a, const char *p) {
    return fmm<MAX>(a, __uint_as_float((uint32_t)(gld<uint16_t>(p)) << 16));
  }
  __device__ static void sstore(char *p, sacc_t a) { gst<uint16_t>(p, (uint16_t)(__float_as_uint(a) >> 16)); }
};

// int32 (signed compare) and uint64 (unsigned compare).
template <bool MAX, class T, class VT>
struct OpIntMM {
  static constexpr bool kWidens = false;
  static constexpr bool kHalfChunk = sizeof(T) == 4;  // phase_p_of
  static constexpr int kEsz = sizeof(T);
  static constexpr T kId = MAX ? std::numeric_limits<T>::min() : std::numeric_limits<T>::max();
  typedef VT acc_t;
  __device__ static acc_t zero() { return (VT)(kId); }
  __device__ static acc_t add(acc_t a, u32x4 p) { return imm<MAX>(a, __builtin_bit_cast(VT, p)); }
  __device__ static u32x4 pack(acc_t a) { return __builtin_bit_cast(u32x4, a); }
  typedef T sacc_t;
  __device__ static sacc_t szero() { return kId; }
  __device__ static sacc_t sadd(sacc_t a, const char *p) { return imm<MAX>(a, gld<T>(p)); }
  __device__ static void sstore(char *p, sacc_t a) { gst<T>(p, a); }
};

template <bool MAX> using OpF32MM = OpFloatMM<MAX, float, f32x4>;
template <bool MAX> using OpF64MM = OpFloatMM<MAX, double, f64x2>;
template <bool MAX> using OpF16MM = OpFloatMM<MAX, half_t, f16x8>;
template <bool MAX> using OpI32MM = OpIntMM<MAX, int32_t, i32x4>;
template <bool MAX> using OpU64MM = OpIntMM<MAX, uint64_t, u64x2>;

// -------------------------------------------------- PROD and bitwise ops --
// PROD: zero() is 1 and add() one multiply, rounded to T (nearest even,
// subnormals kept) -- the second arithmetic under the parity contract: one
// rounding per step, strictly in list order.  There are only multiplies, so
// nothing can fuse, and a floating multiply is not re-associable, so the
// floating ops need no kPinAcc.  1 * x is x for every x but a signalling NaN
// (NaNs compare by NaN-ness), so the compiler may drop the first multiply.

// f32, f64, f16: the packet is a vector of T and so is the accumulator (f16:
// one v_pk_mul_f16 per two elements, no conversion).
template <class T, class VT>
struct OpFloatProd {
  static constexpr bool kWidens = false;
  static constexpr int kEsz = sizeof(T);
  typedef VT acc_t;
  __device__ static acc_t zero() { return (VT)((T)1.0f); }
  __device__ static acc_t add(acc_t a, u32x4 p) { return a * __builtin_bit_cast(VT, p); }
  __device__ static u32x4 pack(acc_t a) { return __builtin_bit_cast(u32x4, a); }
  typedef T sacc_t;
  __device__ static sacc_t szero() { return (T)1.0f; }
  __device__ static sacc_t sadd(sacc_t a, const char *p) { return a * gld<T>(p); }
  __device__ static void sstore(char *p, sacc_t a) { gst<T>(p, a); }
};

// bf16: OpBF16's shape with a multiply in place of the add -- widen both
// halves (exact), multiply in f32, round to nearest even back to bf16 after
// EVERY multiply, the accumulator kept packed.  The f32 product of two bf16
// values is exact (16 significand bits) except below 2^-134, half of bf16's
// smallest subnormal, where f32's own subnormals run out of bits: there the
// f32 rounding gives at most 2^-134 and the bf16 rounding (a tie at most, to
// even) gives zero, as one rounding of the exact product does.
struct OpBF16Prod {
  static constexpr bool kWidens = true;
  static constexpr int kEsz = 2;
  static constexpr uint32_t kOne = 0x3f803f80u;  // 1.0 | 1.0
  typedef u32x4 acc_t;
  __device__ static acc_t zero() { return (u32x4)(kOne); }
  // not an inline constant: from a scalar register, as OpBF16MM's
  __device__ static acc_t tile_zero() {
    uint32_t k;
    asm("s_mov_b32 %0, %1" : "=s"(k) : "i"(kOne));
    return (u32x4)(k);
  }
  __device__ static acc_t add(acc_t a, u32x4 p) {
    acc_t r;
#pragma unroll
    for (int w = 0; w < 4; w++)
      r[w] = bf_pack_opaque(bf_lo(a[w]) * bf_lo(p[w]), bf_hi(a[w]) * bf_hi(p[w]));
    return r;
  }
  __device__ static u32x4 pack(acc_t a) { return a; }
  typedef float sacc_t;  // a widened bf16
  __device__ static sacc_t szero() { return 1.0f; }
  __device__ static sacc_t sadd(sacc_t a, const char *p) {
    float s = a * __uint_as_float((uint32_t)(gld<uint16_t>(p)) << 16);
    return __uint_as_float((uint32_t)bf_round(s) << 16);
  }
  __device__ static void sstore(char *p, sacc_t a) { gst<uint16_t>(p, bf_round(a)); }
};

// int32 and uint64, PROD and the three bitwise operators: wrap-around
// multiply (the low bits, the same for either signedness) and AND / OR / XOR,
// all done in unsigned.  Exact, so re-associable across inputs: kPinAcc.
constexpr int kIntProd = 0, kIntAnd = 1, kIntOr = 2, kIntXor = 3;

template <int OP, class V>
__device__ __forceinline__ V int_fold(V a, V b) {  // unsigned, scalar or vector
  if constexpr (OP == kIntProd) return a * b;
  else if constexpr (OP == kIntAnd) return a & b;
  else if constexpr (OP == kIntOr) return a | b;
  else return a ^ b;
}

template <int OP, class T, class VT>
struct OpIntFold {
  static constexpr bool kWidens = false;
  static constexpr bool kPinAcc = true;
  static constexpr bool kHalfChunk = sizeof(T) == 4;  // phase_p_of
  static constexpr int kEsz = sizeof(T);
  static constexpr T kId = OP == kIntProd ? (T)1 : OP == kIntAnd ? (T)~(T)0 : (T)0;
  typedef VT acc_t;
  __device__ static acc_t zero() { return (VT)(kId); }
  __device__ static acc_t add(acc_t a, u32x4 p) { return int_fold<OP>(a, __builtin_bit_cast(VT, p)); }
  __device__ static u32x4 pack(acc_t a) { return __builtin_bit_cast(u32x4, a); }
  typedef T sacc_t;
  __device__ static sacc_t szero() { return kId; }
  __device__ static sacc_t sadd(sacc_t a, const char *p) { return int_fold<OP>(a, gld<T>(p)); }
  __device__ static void sstore(char *p, sacc_t a) { gst<T>(p, a); }
};

typedef OpFloatProd<float, f32x4> OpF32Prod;
typedef OpFloatProd<double, f64x2> OpF64Prod;
typedef OpFloatProd<half_t, f16x8> OpF16Prod;
template <int OP> using OpI32Fold = OpIntFold<OP, uint32_t, u32x4>;
template <int OP> using OpU64Fold = OpIntFold<OP, uint64_t, u64x2>;

// ------------------------------------------------------------ scaled sums --
// out = finish(sum, alpha): the SUM op of the same dtype and accumulator with a
// FINISHING step at store time -- pack() and sstore() take the wave-uniform
// alpha of the launch (Scale, kernels.h; it arrives in the kernel arguments
// of k_reduce_single_scaled / k_reduce_plan_scaled, so it stays in SGPRs) and multiply once, after the last add.  zero() and
// add() are the SUM op's own, so the sum is SUM's, bit for bit.
//   f64           fl64(s * alpha)
//   f32           fl32(s * a32), a32 = (float)alpha
//   bf16 / f16    round_T(fl32(widen(s) * a32)): the f32 product is ROUNDED TO
//                 F32 and then rounded to nearest even to T -- two roundings,
//                 which is the definition (a single rounding of the exact
//                 product differs, and so does a half multiply)
//   ... wide      round_T(fl32(s32 * a32)), s32 the f32 accumulator
// A multiply that follows an add cannot fuse with it.  Widen, multiply and
// narrow stay three instructions: the product passes through an empty asm
// (opaque_f32), so no pattern can fold the multiply into the conversion (a
// v_fma_mixlo_f16 in place of v_mul_f32 + v_cvt_f16_f32).
// An op without a finishing step has fin_t = NoFin (fin_of), an empty struct
// that the engines pass along and pack_fin / sstore_fin drop: the other ops'
// kernels do not change.
struct NoFin {};

template <class Op, class = void>
struct fin_of {
  typedef NoFin type;
};
template <class Op>
struct fin_of<Op, std::void_t<typename Op::fin_t>> {
  typedef typename Op::fin_t type;
};
template <class Op> using fin_t = typename fin_of<Op>::type;

template <class Op>
__device__ __forceinline__ u32x4 pack_fin(typename Op::acc_t a, fin_t<Op> f) {
  if constexpr (std::is_same<fin_t<Op>, NoFin>::value) return Op::pack(a);
  else return Op::pack(a, f);
}
template <class Op>
__device__ __forceinline__ void sstore_fin(char *p, typename Op::sacc_t a, fin_t<Op> f) {
  if constexpr (std::is_same<fin_t<Op>, NoFin>::value) Op::sstore(p, a);
  else Op::sstore(p, a, f);
}

__device__ __forceinline__ float opaque_f32(float x) {
  asm("" : "+v"(x));
  return x;
}
// one element's finishing multiply of the 2-byte types: an f32 product,
// rounded to f32, that the narrowing conversion cannot be merged with
__device__ __forceinline__ float scale_f32(float s, float a32) { return opaque_f32(s * a32); }

// f32, f64: one IEEE multiply of the packet by alpha.
template <class Base, class T>
struct OpFloatScaled : Base {
  typedef T fin_t;
  __device__ static T fin(const Scale &s) {
    if constexpr (sizeof(T) == 8) return s.a64;
    else return s.a32;
  }
  __device__ static u32x4 pack(typename Base::acc_t a, T alpha) { return __builtin_bit_cast(u32x4, a * alpha); }
  __device__ static void sstore(char *p, T a, T alpha) { gst<T>(p, a * alpha); }
};

// bf16: BF16 = OpBF16 (the packed bf16 accumulator is widened, exactly) or
// OpBF16Wide (the f32 accumulator as it is).
template <class Base>
struct OpBF16Scaled : Base {
  typedef float fin_t;
  __device__ static float fin(const Scale &s) { return s.a32; }
  __device__ static u32x4 pack(typename Base::acc_t a, float a32) {
    u32x4 r;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      if constexpr (sizeof(typename Base::acc_t) > kPacket)
        r[w] = bf_pack(scale_f32(a[2 * w], a32), scale_f32(a[2 * w + 1], a32));
      else
        r[w] = bf_pack(scale_f32(bf_lo(a[w]), a32), scale_f32(bf_hi(a[w]), a32));
    }
    return r;
  }
  // the scalar accumulator of both is a float (native: a widened bf16)
  __device__ static void sstore(char *p, float a, float a32) { gst<uint16_t>(p, bf_round(scale_f32(a, a32))); }
};

// f16: Base = OpF16 (the half accumulator is widened, exactly) or OpF16Wide.
template <class Base>
struct OpF16Scaled : Base {
  typedef float fin_t;
  __device__ static float fin(const Scale &s) { return s.a32; }
  __device__ static u32x4 pack(typename Base::acc_t a, float a32) {
    u32x4 r;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      const float lo = scale_f32((float)a[2 * w], a32), hi = scale_f32((float)a[2 * w + 1], a32);
      r[w] = (uint32_t)f16_round(lo) | (uint32_t)f16_round(hi) << 16;
    }
    return r;
  }
  __device__ static void sstore(char *p, typename Base::sacc_t a, float a32) {
    gst<uint16_t>(p, f16_round(scale_f32((float)a, a32)));
  }
};

typedef OpFloatScaled<OpF32, float> OpF32Scaled;
typedef OpFloatScaled<OpF64, double> OpF64Scaled;
typedef OpBF16Scaled<OpBF16> OpBF16NatScaled;
typedef OpBF16Scaled<OpBF16Wide> OpBF16WideScaled;
typedef OpF16Scaled<OpF16> OpF16NatScaled;
typedef OpF16Scaled<OpF16Wide> OpF16WideScaled;

// -------------------------------------------------------------- OCP FP8 ops --
// HICCL_FLOAT8_E4M3 (e4m3fn) and HICCL_FLOAT8_E5M2, 16 elements per packet.
// The arithmetic is defined through f32 (hiccl_reduce.h): widen(b) is exact,
// round_F(x) clamps a FINITE x to [-max, +max] (saturate-to-finite) and rounds
// to nearest even, subnormals kept; a NaN stays a NaN, +-Inf stays +-Inf in
// e5m2 and becomes a NaN in e4m3.
// gfx950 converts two elements per instruction: v_cvt_pk_f32_fp8 / _bf8 widen
// the low or the high half of a word, v_cvt_pk_fp8_f32 / _bf8_f32 round two
// f32 into one half of a word and keep the other.  The clamp comes FIRST and
// is this code's own, so nothing rests on what the conversion does with a
// finite value out of range; Inf and NaN reach it unclamped.
// The native ops keep the accumulator PACKED (16 elements in a u32x4, the
// packet's own layout, 4 VGPRs), as OpBF16 does and for its reason: the phased
// engine then runs FP8 at the same 128 KiB chunk as f32.  Per packet a native
// add is 16 widens (8 of the accumulator, 8 of the input), 16 f32 adds, the
// clamp (e4m3: 32 instructions, e5m2: 48) and 8 rounds.
constexpr int kE4M3 = 0, kE5M2 = 1;
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int FMT>
struct F8 {
  static constexpr float kMax = FMT == kE4M3 ? 448.0f : 57344.0f;
  // the operator identities: e5m2 -Inf / +Inf, e4m3 (no infinity) -448 / +448
  static constexpr uint32_t kMaxId = FMT == kE4M3 ? 0xfeu : 0xfcu;
  static constexpr uint32_t kMinId = FMT == kE4M3 ? 0x7eu : 0x7cu;
  // bytes {0, 1} (hi = false) or {2, 3} of w, exact
  template <bool HI>
  __device__ static f32x2 widen2(uint32_t w) {
    if constexpr (FMT == kE4M3) return __builtin_amdgcn_cvt_pk_f32_fp8((int)w, HI);
    else return __builtin_amdgcn_cvt_pk_f32_bf8((int)w, HI);
  }
  // The clamp of round_F.  INF = false: the caller knows x is finite or NaN
  // (a sum of two e4m3 values: the format has no infinity) -- the IEEE
  // 754-2019 maximum / minimum pair, which passes a NaN on.  Otherwise the
  // median of a finite x, and a non-finite x as it is.
  template <bool INF>
  __device__ static float clamp(float x) {
    if constexpr (!INF) return fmm<false>(fmm<true>(x, -kMax), kMax);
    else return __builtin_isfinite(x) ? __builtin_amdgcn_fmed3f(x, -kMax, kMax) : x;
  }
  // round_F(lo), round_F(hi) into the low or the high half of `old`
  template <bool HI, bool INF>
  __device__ static uint32_t round2(float lo, float hi, uint32_t old) {
    lo = clamp<INF>(lo);
    hi = clamp<INF>(hi);
    if constexpr (FMT == kE4M3) return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(lo, hi, (int)old, HI);
    else return (uint32_t)__builtin_amdgcn_cvt_pk_bf8_f32(lo, hi, (int)old, HI);
  }
  // one element (the peeled head / tail)
  __device__ static float widen1(uint8_t b) { return widen2<false>(b)[0]; }
  template <bool INF>
  __device__ static uint8_t round1(float x) { return (uint8_t)round2<false, INF>(x, x, 0u); }
  __device__ static float ld(const char *p) { return widen1(gld<uint8_t>(p)); }
};

// the 16 elements of a packet <-> f32, four per word
template <int FMT>
__device__ __forceinline__ void f8_widen4(uint32_t w, float (&v)[4]) {
  const f32x2 lo = F8<FMT>::template widen2<false>(w), hi = F8<FMT>::template widen2<true>(w);
  v[0] = lo[0], v[1] = lo[1], v[2] = hi[0], v[3] = hi[1];
}
template <int FMT, bool INF>
__device__ __forceinline__ uint32_t f8_round4(const float (&v)[4]) {
  const uint32_t r = F8<FMT>::template round2<false, INF>(v[0], v[1], 0u);
  return F8<FMT>::template round2<true, INF>(v[2], v[3], r);
}

// Native SUM: acc = round_F(fl32(widen(acc) + widen(x))) after every input.
// Both operands of e4m3 are finite or NaN, so is their f32 sum: no Inf select.
template <int FMT>
struct OpF8 {
  static constexpr bool kWidens = true;
  static constexpr int kEsz = 1;
  static constexpr bool kInf = FMT == kE5M2;
  typedef u32x4 acc_t;
  __device__ static acc_t zero() { return (u32x4)(0u); }  // +0
  __device__ static acc_t add(acc_t a, u32x4 p) {
    acc_t r;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      float x[4], y[4];
      f8_widen4<FMT>(a[w], x);
      f8_widen4<FMT>(p[w], y);
#pragma unroll
      for (int i = 0; i < 4; i++) x[i] += y[i];
      r[w] = f8_round4<FMT, kInf>(x);
    }
    return r;
  }
  __device__ static u32x4 pack(acc_t a) { return a; }
  typedef float sacc_t;  // a widened element
  __device__ static sacc_t szero() { return 0.0f; }
  __device__ static sacc_t sadd(sacc_t a, const char *p) {
    return F8<FMT>::widen1(F8<FMT>::template round1<kInf>(a + F8<FMT>::ld(p)));
  }
  __device__ static void sstore(char *p, sacc_t a) { gst<uint8_t>(p, F8<FMT>::template round1<true>(a)); }
};

// HICCL_ACC_WIDE: an f32 accumulator per element (16 VGPRs per packet), one
// f32 add per input in list order from +0, round_F once at the end.
template <int FMT>
struct OpF8Wide {
  static constexpr bool kWidens = true;
  static constexpr int kEsz = 1;
  // sixteen floats, not a 16-wide vector: one 512-bit register tuple per packet
  // made the tile kernels spill (copies of whole tuples around the group loop)
  struct acc_t {
    float v[16];
    __device__ float &operator[](int i) { return v[i]; }
  };
  __device__ static acc_t zero() {
    acc_t a;
#pragma unroll
    for (int i = 0; i < 16; i++) a.v[i] = 0.0f;
    return a;
  }
  __device__ static acc_t add(acc_t a, u32x4 p) {
#pragma unroll
    for (int w = 0; w < 4; w++) {
      float y[4];
      f8_widen4<FMT>(p[w], y);
#pragma unroll
      for (int i = 0; i < 4; i++) a[4 * w + i] += y[i];
    }
    return a;
  }
  __device__ static u32x4 pack(acc_t a) {
    u32x4 r;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      const float x[4] = {a[4 * w], a[4 * w + 1], a[4 * w + 2], a[4 * w + 3]};
      r[w] = f8_round4<FMT, true>(x);
    }
    return r;
  }
  typedef float sacc_t;
  __device__ static sacc_t szero() { return 0.0f; }
  __device__ static sacc_t sadd(sacc_t a, const char *p) { return a + F8<FMT>::ld(p); }
  __device__ static void sstore(char *p, sacc_t a) { gst<uint8_t>(p, F8<FMT>::template round1<true>(a)); }
};

// MAX / MIN: IEEE 754-2019 maximum / minimum of the widened values, packed
// again by the rounding conversion -- the winner is an FP8 value, so nothing
// rounds and nothing needs the clamp (e5m2's infinities pass the conversion as
// they are).  A NaN operand gives a NaN, -0 < +0.
template <bool MAX, int FMT>
struct OpF8MM {
  static constexpr bool kWidens = true;
  static constexpr int kEsz = 1;
  static constexpr uint32_t kIdByte = MAX ? F8<FMT>::kMaxId : F8<FMT>::kMinId;
  static constexpr uint32_t kIdBits = kIdByte * 0x01010101u;
  typedef u32x4 acc_t;
  __device__ static acc_t zero() { return (u32x4)(kIdBits); }
  // not an inline constant: from a scalar register, as OpBF16MM's
  __device__ static acc_t tile_zero() {
    uint32_t k;
    asm("s_mov_b32 %0, %1" : "=s"(k) : "i"(kIdBits));
    return (u32x4)(k);
  }
  __device__ static uint32_t join(const float (&v)[4]) {
    uint32_t r;
    if constexpr (FMT == kE4M3) {
      r = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0, false);
      r = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], (int)r, true);
    } else {
      r = (uint32_t)__builtin_amdgcn_cvt_pk_bf8_f32(v[0], v[1], 0, false);
      r = (uint32_t)__builtin_amdgcn_cvt_pk_bf8_f32(v[2], v[3], (int)r, true);
    }
    return r;
  }
  __device__ static acc_t add(acc_t a, u32x4 p) {
    acc_t r;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      float x[4], y[4];
      f8_widen4<FMT>(a[w], x);
      f8_widen4<FMT>(p[w], y);
#pragma unroll
      for (int i = 0; i < 4; i++) x[i] = fmm<MAX>(x[i], y[i]);
      r[w] = join(x);
    }
    return r;
  }
  __device__ static u32x4 pack(acc_t a) { return a; }
  typedef float sacc_t;  // a widened element
  __device__ static sacc_t szero() { return F8<FMT>::widen1((uint8_t)kIdByte); }
  __device__ static sacc_t sadd(sacc_t a, const char *p) { return fmm<MAX>(a, F8<FMT>::ld(p)); }
  __device__ static void sstore(char *p, sacc_t a) {
    const float v[4] = {a, a, a, a};
    gst<uint8_t>(p, (uint8_t)join(v));
  }
};

// Scaled sums: Base = OpF8 (round_F(fl32(widen(s) * a32))) or OpF8Wide
// (round_F(fl32(s32 * a32))).  The f32 product may overflow to Inf, so the
// rounding takes the full clamp.
template <class Base, int FMT>
struct OpF8Scaled : Base {
  typedef float fin_t;
  __device__ static float fin(const Scale &s) { return s.a32; }
  __device__ static u32x4 pack(typename Base::acc_t a, float a32) {
    u32x4 r;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      float x[4];
      if constexpr (sizeof(typename Base::acc_t) > kPacket) {
#pragma unroll
        for (int i = 0; i < 4; i++) x[i] = a[4 * w + i];
      } else {
        f8_widen4<FMT>(a[w], x);
      }
#pragma unroll
      for (int i = 0; i < 4; i++) x[i] = scale_f32(x[i], a32);
      r[w] = f8_round4<FMT, true>(x);
    }
    return r;
  }
  // the scalar accumulator of both is a float (native: a widened element)
  __device__ static void sstore(char *p, float a, float a32) {
    gst<uint8_t>(p, F8<FMT>::template round1<true>(scale_f32(a, a32)));
  }
};

// ------------------------------------------------------------ widened sums --
// bf16, f16 or FP8 inputs summed into an f32 OUTPUT (hiccl_reduce_widened): the
// arithmetic of the f32-accumulating ops above -- widen (exact), one f32 add per
// input in list order from +0 -- whose accumulator is stored as it is instead of
// being rounded back.  The one op family with two element sizes: kEsz is the
// inputs', kOutEsz the output's, and a packet is FOUR elements -- 16 B of the
// output (one f32x4 accumulator, one buffer_store_dwordx4) and 4 * kEsz bytes
// of every input (in_t: one buffer_load_dwordx2 of a 2-byte type, one
// buffer_load_dword of FP8).  Every byte quantity the engines pass along is the
// output's; the inputs' are those times kEsz / kOutEsz (in_bytes).
// There is one kernel for the plain and the scaled form: the store multiplies
// by a32, and the plain form passes 1.0f (fl32(s * 1.0f) is s for every s that
// is not a NaN, and NaNs compare by NaN-ness).
// An op of this family is told by kOutEsz, which no other op has.
template <class Op, class = void>
struct widens_out : std::false_type {};
template <class Op>
struct widens_out<Op, std::enable_if_t<(Op::kOutEsz > 0)>> : std::true_type {};

// bytes per output element, and an input's byte quantity from the output's
template <class Op>
constexpr int out_esz() {
  if constexpr (widens_out<Op>::value) return Op::kOutEsz;
  else return Op::kEsz;
}
template <class Op, class V>
__device__ __forceinline__ V in_bytes(V out_bytes) {
  if constexpr (widens_out<Op>::value) return out_bytes / (V)(Op::kOutEsz / Op::kEsz);
  else return out_bytes;
}

// what one lane loads of one input per packet
template <class Op, class = void>
struct in_pkt {
  typedef u32x4 type;
};
template <class Op>
struct in_pkt<Op, std::void_t<typename Op::in_t>> {
  typedef typename Op::in_t type;
};
template <class Op> using in_pkt_t = typename in_pkt<Op>::type;

template <class Op, int POL>
__device__ __forceinline__ in_pkt_t<Op> load_in(rsrc_t r, uint32_t voff) {
  if constexpr (widens_out<Op>::value) return Op::template load<POL>(r, in_bytes<Op>(voff));
  else return load_pkt<POL>(r, voff);
}

// The widening of one input packet (W of OpWiden): four elements -> f32x4.
struct WidenBF16 {
  static constexpr int kEsz = 2;
  typedef u32x2 in_t;
  template <int POL>
  __device__ static in_t load(rsrc_t r, uint32_t voff) { return load_pkt_b64<POL>(r, voff); }
  __device__ static f32x4 widen4(in_t p) { return f32x4{bf_lo(p[0]), bf_hi(p[0]), bf_lo(p[1]), bf_hi(p[1])}; }
  __device__ static float ld(const char *p) { return __uint_as_float((uint32_t)(gld<uint16_t>(p)) << 16); }
};

struct WidenF16 {
  static constexpr int kEsz = 2;
  typedef u32x2 in_t;
  template <int POL>
  __device__ static in_t load(rsrc_t r, uint32_t voff) { return load_pkt_b64<POL>(r, voff); }
  __device__ static f32x4 widen4(in_t p) {
    return f32x4{f16_widen(p[0], 0), f16_widen(p[0], 1), f16_widen(p[1], 0), f16_widen(p[1], 1)};
  }
  __device__ static float ld(const char *p) { return (float)f16_ld(p); }
};

template <int FMT>
struct WidenF8 {
  static constexpr int kEsz = 1;
  typedef uint32_t in_t;
  template <int POL>
  __device__ static in_t load(rsrc_t r, uint32_t voff) { return load_pkt_b32<POL>(r, voff); }
  __device__ static f32x4 widen4(in_t p) {
    float v[4];
    f8_widen4<FMT>(p, v);
    return f32x4{v[0], v[1], v[2], v[3]};
  }
  __device__ static float ld(const char *p) { return F8<FMT>::ld(p); }
};

template <class W>
struct OpWiden {
  static constexpr bool kWidens = true;
  static constexpr int kEsz = W::kEsz;
  static constexpr int kOutEsz = 4;
  typedef typename W::in_t in_t;
  template <int POL>
  __device__ static in_t load(rsrc_t r, uint32_t voff) { return W::template load<POL>(r, voff); }
  typedef f32x4 acc_t;
  __device__ static acc_t zero() { return (f32x4)(0.0f); }
  __device__ static acc_t add(acc_t a, in_t p) { return a + W::widen4(p); }
  typedef float fin_t;
  __device__ static float fin(const Scale &s) { return s.a32; }
  __device__ static u32x4 pack(acc_t a, float a32) { return __builtin_bit_cast(u32x4, a * a32); }
  typedef float sacc_t;
  __device__ static sacc_t szero() { return 0.0f; }
  __device__ static sacc_t sadd(sacc_t a, const char *p) { return a + W::ld(p); }
  __device__ static void sstore(char *p, float a, float a32) { gst<float>(p, a * a32); }
};

typedef OpWiden<WidenBF16> OpBF16ToF32;
typedef OpWiden<WidenF16> OpF16ToF32;
template <int FMT> using OpF8ToF32 = OpWiden<WidenF8<FMT>>;

// ------------------------------------------------ accumulating widened sums --
// out = fl32(p + fl32(s32 * a32)), p the OUTPUT as it was before the launch
// (hiccl_reduce_accumulate, hiccl_reduce_plan_set_accumulate): OpWiden's sum,
// bit for bit, finished first; then the scale, on the new contribution alone;
// then ONE add of the old output -- three separately rounded f32 operations.
// The product passes through opaque_f32 as the scaled sums' does, so the
// multiply and the add that follows it cannot contract into v_fma_f32 /
// v_pk_fma_f32 (a different word: one rounding less).  p is not addend 0 of
// the fold (fl32(fl32(p + x0) + x1) differs from fl32(p + fl32(x0 + x1))).
// An op of this family sets kAccum: the engines then read the old packet
// through the OUTPUT's own descriptor (the range check of the store, one
// buffer_load_dwordx4 per packet) and hand it to pack(); sstore() reads the
// scalar head / tail element it is about to overwrite.  A unit is read,
// modified and written once per launch: head, body units and tail are
// disjoint, and both schedules hand every unit out once.
// A family of its own, not a flag of OpWiden: the widened kernels stay
// instruction for instruction what they are, and the kernels' names differ.
template <class Op, class = void>
struct accumulates : std::false_type {};
template <class Op>
struct accumulates<Op, std::enable_if_t<Op::kAccum>> : std::true_type {};

template <class W>
struct OpWidenAccum : OpWiden<W> {
  static constexpr bool kAccum = true;
  static constexpr bool kHalfChunk = true;  // phase_p_of: the old packets are held over the sweep (chunk_body)
  __device__ static u32x4 pack(f32x4 a, float a32, u32x4 old) {
    f32x4 r;
#pragma unroll
    for (int i = 0; i < 4; i++) r[i] = opaque_f32(a[i] * a32);
    return __builtin_bit_cast(u32x4, __builtin_bit_cast(f32x4, old) + r);
  }
  __device__ static void sstore(char *p, float a, float a32) {
    const float r = opaque_f32(a * a32);
    gst<float>(p, gld<float>(p) + r);
  }
};

typedef OpWidenAccum<WidenBF16> OpBF16AccF32;
typedef OpWidenAccum<WidenF16> OpF16AccF32;
template <int FMT> using OpF8AccF32 = OpWidenAccum<WidenF8<FMT>>;

// --------------------------------------------------- weighted widened sums --
// out = finish(((+0 + fl32(w[0] * widen(x[0]))) + fl32(w[1] * widen(x[1]))) + ...)
// (hiccl_reduce_weighted, hiccl_reduce_plan_set_weighted): the widened sum, or
// the accumulating one, of inputs that each count with an f32 weight of their
// own -- NCCL's PreMulSum.  The weights live in DEVICE memory and are read when
// the kernel runs (weight_of: scalar loads through the constant address space,
// so a weight stays in an SGPR and is one operand of the lanes' multiplies).
// The multiply and the add are TWO separately rounded f32 operations: the
// products pass through an empty asm (opaque_f32x4 / opaque_f32), so they cannot
// contract with the add that follows into v_fma_f32 / v_pk_fma_f32 (a
// different word: one rounding less).  A weight of exactly 1.0f gives
// t = widen(x) bit for bit, so all-ones weights give the widened sum's words.
// zero(), pack() and sstore() are the base family's: alpha, the old output and
// n = 0 behave as they do there.
// An op of this family sets kWeighted; its add() and sadd() take the weight,
// which the engines fetch from the Inputs functor (w(k)) behind if constexpr.
// Families of their own, with kernels of their own (k_reduce_single_weighted,
// k_reduce_plan_weighted): every other kernel stays what it is.
template <class Op, class = void>
struct weighted : std::false_type {};
template <class Op>
struct weighted<Op, std::enable_if_t<Op::kWeighted>> : std::true_type {};

// what the engines carry per input next to its packets: the weight, or nothing
struct NoWeight {};
template <class Op> using w_t = std::conditional_t<weighted<Op>::value, float, NoWeight>;

template <class Op, class Inputs>
__device__ __forceinline__ w_t<Op> weight_of(const Inputs &in, uint32_t k) {
  if constexpr (weighted<Op>::value) return in.w(k);
  else return {};
}
template <class Op>
__device__ __forceinline__ typename Op::acc_t add_in(typename Op::acc_t a, in_pkt_t<Op> x, w_t<Op> w) {
  if constexpr (weighted<Op>::value) return Op::add(a, x, w);
  else return Op::add(a, x);
}

__device__ __forceinline__ f32x4 opaque_f32x4(f32x4 x) {
  asm("" : "+v"(x));
  return x;
}

template <class W>
struct OpWeighted : OpWiden<W> {
  static constexpr bool kWeighted = true;
  __device__ static f32x4 add(f32x4 a, typename W::in_t p, float w) { return a + opaque_f32x4(W::widen4(p) * w); }
  __device__ static float sadd(float a, const char *p, float w) { return a + opaque_f32(W::ld(p) * w); }
};

template <class W>
struct OpWeightedAccum : OpWidenAccum<W> {
  static constexpr bool kWeighted = true;
  __device__ static f32x4 add(f32x4 a, typename W::in_t p, float w) { return a + opaque_f32x4(W::widen4(p) * w); }
  __device__ static float sadd(float a, const char *p, float w) { return a + opaque_f32(W::ld(p) * w); }
};

// The old output packets of a unit, one buffer_load_dwordx4 each (kAccum ops).
template <class Op, int U, int POL>
__device__ __forceinline__ void load_old(u32x4 (&old)[U], rsrc_t w, const uint32_t (&voff)[U]) {
#pragma unroll
  for (int u = 0; u < U; u++) old[u] = load_pkt<POL>(w, voff[u]);
}

// ----------------------------------------------------------- tile engine --
//
// A compute is split as [head scalars | npkt 16-B packets | tail scalars],
// the packets 16-B aligned on the OUTPUT.  A tile = BLOCK*U packets; lane t
// of the workgroup owns packets u*BLOCK + t (u < U), so every load
// instruction of a wave covers 1 KiB contiguous bytes of one input.
// (SingleArgs, PlanDesc, PlanArgs: kernels.h.)

// Input pointer source: kernarg array or device table.
struct ArgInputs {
  const char *const *p;
  __device__ const char *operator()(int k) const { return p[k]; }
};

// The weights of a weighted op (engine.h's weighted sums): n consecutive floats
// in device memory, read through the constant address space (4) as the plan's
// pointer table is (TableInputs) -- scalar loads, the value known uniform.  Only
// a weighted op's kernels build these functors and only its add()s call w().
typedef const float __attribute__((address_space(4))) ConstF32;

struct ArgInputsWeighted : ArgInputs {
  const float *wp;
  __device__ float w(int k) const { return ((ConstF32 *)wp)[k]; }
};

// Under the peer policies the plain scalar accesses are bracketed by
// system-scope fences instead (an acquire before the loads: this XCD's L2
// drops lines of peer memory; a release after the stores: its dirty lines
// are written back) -- only the workgroup owning a compute's first unit,
// and only when the compute has a head or a tail.
template <class Op, int POL = 11, class Inputs>
__device__ __forceinline__ void scalar_part(char *out, Inputs in, uint32_t n, uint32_t head,
                                            uint64_t npkt, uint32_t tail, int tid, fin_t<Op> fin = {}) {
  constexpr int V = kPacket / out_esz<Op>();
  if (tid >= (int)(head + tail)) return;
  if constexpr (POL % 10 == kPolLoadSys) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
  uint64_t e = (tid < (int)head) ? (uint64_t)tid : (uint64_t)head + npkt * V + (tid - head);
  uint64_t off = e * Op::kEsz;
  typename Op::sacc_t acc = Op::szero();
  for (uint32_t k = 0; k < n; k++) {
    if constexpr (weighted<Op>::value) acc = Op::sadd(acc, in(k) + off, in.w(k));
    else acc = Op::sadd(acc, in(k) + off);
  }
  if constexpr (widens_out<Op>::value) sstore_fin<Op>(out + e * Op::kOutEsz, acc, fin);
  else sstore_fin<Op>(out + off, acc, fin);
  if constexpr (POL / 10 == kPolStoreSys) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
}

// One group of G inputs (G static): G descriptor builds (scalar), then G*U
// independent 16-B buffer loads, then the G in-order adds per packet.
//
// PACED: a pause of kPaceSleep x 64 clocks between one input's U loads and the
// next input's.  With scalar descriptors the G*U loads of a wave issue back to
// back, and on the one launch that is bound by HBM alone -- config 2's
// one-shot tiles on the ticket counter, 256 workgroups x 4 waves bursting 32
// KiB each -- that burst measured 1.1-1.6 % SLOWER than the waterfall loops
// it replaced, which had spread the same loads over about a microsecond.
// Spreading them on purpose gives that back, and on 7/8 of the grid
// (policy.cpp launch_shape) runs 2.4 % ahead.  The
// pauses hide under the tile's memory time; a latency-bound launch (static
// schedule, plans, programs) would pay for them, so only the one-shot
// kernel's dynamic schedule asks for them.
constexpr int kPaceSleep = 4;

template <class Op, int U, int G, int POL, bool PACED, class Inputs>
__device__ __forceinline__ void group_at(typename Op::acc_t (&acc)[U], Inputs in, uint32_t g,
                                         uint64_t tile_off, uint32_t tile_bytes,
                                         const uint32_t (&voff)[U]) {
  rsrc_t r[G];
#pragma unroll
  for (int j = 0; j < G; j++) r[j] = make_rsrc(in(g + j) + in_bytes<Op>(tile_off), in_bytes<Op>(tile_bytes));
  // a weighted op's G weights, indexed in the input LIST (g + j): scalar loads
  [[maybe_unused]] float wt[weighted<Op>::value ? G : 1];
  if constexpr (weighted<Op>::value) {
#pragma unroll
    for (int j = 0; j < G; j++) wt[j] = in.w(g + j);
  }
  in_pkt_t<Op> x[G][U];
  // Every load of the group is issued before the first add, input by input
  // (the barriers pin that order, so the adds -- input 0 first -- wait with
  // a vmcnt staircase instead of one vmcnt(0)).  Without them the scheduler
  // of the plan kernel (pointer table in memory) split an 8-input group into
  // 24 + 8 (f32) or 16 + 16 (bf16) loads with an s_waitcnt vmcnt(0) in
  // between: two memory round trips per tile.
#pragma unroll
  for (int j = 0; j < G; j++) {
#pragma unroll
    for (int u = 0; u < U; u++) x[j][u] = load_in<Op, POL>(r[j], voff[u]);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (PACED) {
      if (j + 1 < G) {
        __builtin_amdgcn_s_sleep(kPaceSleep);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < G; j++) {
#pragma unroll
    for (int u = 0; u < U; u++) {
      if constexpr (weighted<Op>::value) acc[u] = Op::add(acc[u], x[j][u], wt[j]);
      else acc[u] = Op::add(acc[u], x[j][u]);
    }
  }
}

// One tile: packets pkt0 + u*BLOCK + tid, tile_bytes = valid bytes of the
// tile (< the full tile only for the last one).  Inputs are consumed as full
// groups of 8 followed by one statically sized remainder group, so the adds
// happen in exactly the order k = 0, 1, ..., n-1.
// `before_store()` runs after the last add, before the stores (the unit
// scheduler publishes its next ticket there: every load has been waited for
// and no store is pending yet, so reading the atomic's result costs nothing).
struct NoHook {
  static constexpr bool kDynamic = false;
  __device__ void operator()() const {}
};

// The accumulator a tile starts from: Op::zero(), or Op::tile_zero() where an
// op has one (the same value, made in a way that suits this engine's unit
// loop; the phased engine's chunks take zero(), which the compiler
// rematerialises at the first add instead of holding a chunk of accumulators
// across the first loads).
template <class Op, class = void>
struct has_tile_zero : std::false_type {};
template <class Op>
struct has_tile_zero<Op, std::void_t<decltype(&Op::tile_zero)>> : std::true_type {};

template <class Op>
__device__ __forceinline__ typename Op::acc_t tile_zero() {
  if constexpr (has_tile_zero<Op>::value) return Op::tile_zero();
  else return Op::zero();
}

template <class Op, int U, int POL, bool PACED = false, class Inputs, class Hook = NoHook>
__device__ __forceinline__ void tile_body(char *outb, Inputs in, uint32_t n, uint64_t tile_off,
                                          uint32_t tile_bytes, const uint32_t (&voff)[U],
                                          Hook before_store = Hook(), fin_t<Op> fin = {}) {
  typename Op::acc_t acc[U];
#pragma unroll
  for (int u = 0; u < U; u++) acc[u] = tile_zero<Op>();
  // The output's descriptor is built here, ahead of the input groups, and not
  // next to the stores: built behind the switch below, the u64 kernels got it
  // as a VGPR copy joined over the switch's cases, and with it a waterfall
  // loop around each of their stores (4 SGPRs held over the tile instead).
  const rsrc_t w = make_rsrc(outb + tile_off, tile_bytes);
  // An accumulating op's old output packets are asked for here, ahead of the
  // first group's loads, so they come back under the inputs' latency: with up
  // to 8 inputs that group is the tile's last, with more the 4 * U VGPRs are
  // held over the earlier groups (no spill at 256 x 4).
  [[maybe_unused]] u32x4 old[accumulates<Op>::value ? U : 1];
  if constexpr (accumulates<Op>::value) {
    load_old<Op, U, POL>(old, w, voff);
    __builtin_amdgcn_sched_barrier(0);
  }
  // groups of GM inputs: at most 32 packets per lane in flight (U = 8: 4
  // inputs, U = 16: 2), so wide tiles stay within the register file
  constexpr uint32_t GM = U >= 8 ? 32 / U : 8;
  uint32_t g = 0;
  for (; g + GM <= n; g += GM) group_at<Op, U, GM, POL, PACED>(acc, in, g, tile_off, tile_bytes, voff);
  switch (n - g) {  // wave-uniform
    case 1: group_at<Op, U, 1, POL, PACED>(acc, in, g, tile_off, tile_bytes, voff); break;
    case 2: if constexpr (GM > 2) group_at<Op, U, 2, POL, PACED>(acc, in, g, tile_off, tile_bytes, voff); break;
    case 3: if constexpr (GM > 3) group_at<Op, U, 3, POL, PACED>(acc, in, g, tile_off, tile_bytes, voff); break;
    case 4: if constexpr (GM > 4) group_at<Op, U, 4, POL, PACED>(acc, in, g, tile_off, tile_bytes, voff); break;
    case 5: if constexpr (GM > 5) group_at<Op, U, 5, POL, PACED>(acc, in, g, tile_off, tile_bytes, voff); break;
    case 6: if constexpr (GM > 6) group_at<Op, U, 6, POL, PACED>(acc, in, g, tile_off, tile_bytes, voff); break;
    case 7: if constexpr (GM > 7) group_at<Op, U, 7, POL, PACED>(acc, in, g, tile_off, tile_bytes, voff); break;
    default: break;
  }
  before_store();
#pragma unroll
  for (int u = 0; u < U; u++) {
    if constexpr (accumulates<Op>::value) store_pkt<POL>(w, voff[u], Op::pack(acc[u], fin, old[u]));
    else store_pkt<POL>(w, voff[u], pack_fin<Op>(acc[u], fin));
  }
}

// Input-phased chunk (the default engine for large buckets).  A chunk =
// BLOCK*P packets; lane t owns packets p*BLOCK + t.  The workgroup sweeps
// input 0 of the chunk, then input 1, ...: input j+1's P loads are in flight
// while input j is added, so chip-wide only ~2 input streams are open at a
// time and each is read as long contiguous runs (BLOCK*P*16 B per workgroup;
// 128 KiB at the default 512 x 16).  The per-element add order is unchanged
// (k = 0, 1, ..., n-1 from a zero accumulator).  Measured: the nine-stream
// tile order runs at 5.5-5.8 TB/s and depends on the physical placement of
// the buckets; the phased order at 6.0-6.4 TB/s.
// n is runtime: inputs are taken in pairs; the load that would read past
// input n-1 gets a zero-range descriptor (no memory traffic, reads 0, never
// added).
// An op whose add is exact may be re-associated by the compiler: MAX / MIN of
// input j and of input j + 1 merge into one three-operand instruction placed
// at the second add, which keeps input j's P packets alive over the next
// input's loads (64 more VGPRs at P = 16: the kernel spills).  Such an op sets
// kPinAcc, and the phased engine then closes each add with an empty asm on the
// accumulator, which the merge cannot cross.  (int32 SUM has the same trouble
// and a smaller chunk instead: phase_p_of.)
template <class Op, class = void>
struct pins_acc : std::false_type {};
template <class Op>
struct pins_acc<Op, std::enable_if_t<Op::kPinAcc>> : std::true_type {};

template <class Op>
__device__ __forceinline__ void pin_acc(typename Op::acc_t &a) {
  if constexpr (pins_acc<Op>::value) asm volatile("" : "+v"(a));
}

template <class Op, int P, int POL, class Inputs, class Hook = NoHook>
__device__ __forceinline__ void chunk_body(char *outb, Inputs in, uint32_t n, uint64_t off,
                                           uint32_t nbytes, const uint32_t (&voff)[P],
                                           Hook before_store = Hook(), fin_t<Op> fin = {}) {
  typename Op::acc_t acc[P];
#pragma unroll
  for (int p = 0; p < P; p++) acc[p] = Op::zero();
  // An accumulating op reads the old output through the store's descriptor,
  // which it therefore builds here.  The loads go out in the sweep's LAST pass,
  // behind the x loads -- the slot that holds the zero-range load when n is
  // even -- so the old packets are one more stream of the ping-pong: in flight
  // while the last one or two inputs are added.  They are a loop-carried value
  // (4 VGPRs per packet over every pass), which is why these ops take the half
  // chunk (kHalfChunk): at P = 16 the bf16 kernel came out at 256 VGPRs with 24
  // B of scratch, and a peeled last pass did worse (184 B).
  [[maybe_unused]] u32x4 old[accumulates<Op>::value ? P : 1];
  [[maybe_unused]] rsrc_t wo;
  if constexpr (accumulates<Op>::value) wo = make_rsrc(outb + off, nbytes);
  if (n > 0) {
    in_pkt_t<Op> x[P], y[P];
    const uint64_t ioff = in_bytes<Op>(off);
    const uint32_t ibytes = in_bytes<Op>(nbytes);
    // a weighted op's weights travel with the packets they belong to (wx with
    // x, wy with y): scalar loads, indexed in the input list like the pointers
    [[maybe_unused]] w_t<Op> wx = weight_of<Op>(in, 0), wy = {};
    {
      rsrc_t r = make_rsrc(in(0) + ioff, ibytes);
#pragma unroll
      for (int p = 0; p < P; p++) x[p] = load_in<Op, POL>(r, voff[p]);
    }
    if constexpr (accumulates<Op>::value) {
      if (n == 1) load_old<Op, P, POL>(old, wo, voff);
    }
    uint32_t j = 0;
    for (; j + 2 <= n; j += 2) {  // x: input j in flight
      rsrc_t ry = make_rsrc(in(j + 1) + ioff, ibytes);
      wy = weight_of<Op>(in, j + 1);
#pragma unroll
      for (int p = 0; p < P; p++) y[p] = load_in<Op, POL>(ry, voff[p]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int p = 0; p < P; p++) {
        acc[p] = add_in<Op>(acc[p], x[p], wx);
        pin_acc<Op>(acc[p]);
        if constexpr (Op::kWidens) __builtin_amdgcn_sched_barrier(0);
      }
      __builtin_amdgcn_sched_barrier(0);
      const bool more = j + 2 < n;
      rsrc_t rx = make_rsrc(in(more ? j + 2 : j + 1) + ioff, more ? ibytes : 0u);
      wx = weight_of<Op>(in, more ? j + 2 : j + 1);
#pragma unroll
      for (int p = 0; p < P; p++) x[p] = load_in<Op, POL>(rx, voff[p]);
      if constexpr (accumulates<Op>::value) {
        if (j + 4 > n) load_old<Op, P, POL>(old, wo, voff);  // the last pass: input n-1 is y, or the x just asked for
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int p = 0; p < P; p++) {
        acc[p] = add_in<Op>(acc[p], y[p], wy);
        pin_acc<Op>(acc[p]);
        if constexpr (Op::kWidens) __builtin_amdgcn_sched_barrier(0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if (n & 1) {
#pragma unroll
      for (int p = 0; p < P; p++) acc[p] = add_in<Op>(acc[p], x[p], wx);
    }
  } else if constexpr (accumulates<Op>::value) {
    load_old<Op, P, POL>(old, wo, voff);  // n == 0: out = p + (+0), or p + a zero of alpha's sign
  }
  before_store();
  if constexpr (accumulates<Op>::value) {
#pragma unroll
    for (int p = 0; p < P; p++) store_pkt<POL>(wo, voff[p], Op::pack(acc[p], fin, old[p]));
  } else {
    rsrc_t w = make_rsrc(outb + off, nbytes);
#pragma unroll
    for (int p = 0; p < P; p++) store_pkt<POL>(w, voff[p], pack_fin<Op>(acc[p], fin));
  }
}

// Engines: kTile = all n inputs of a BLOCK*U tile loaded together (small
// computes, many tiles); kPhase = chunk_body (large buckets).
constexpr int kTile = 0;
constexpr int kPhase = 1;

// A value every lane of the workgroup holds alike, moved to SGPRs.
__device__ __forceinline__ uint32_t uniform32(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
  return (uint64_t)uniform32((uint32_t)(v >> 32)) << 32 | uniform32((uint32_t)v);
}

// One unit of either engine.  Every kernel's units come through here, and
// this is where a unit's two descriptor inputs -- its byte offset and its
// valid byte count -- are made scalar, once per unit: the bodies' make_rsrc
// then add them to kernarg / constant-memory pointers and every descriptor
// stays in SGPRs.  Left alone they reach the bodies in VGPRs (the unit index
// comes out of LDS on the dynamic schedule and through tile_order's branch;
// the byte count out of a 64-bit compare/select, which gfx9 has on the VALU
// only), and the compiler then wraps EACH buffer load and store in a
// readfirstlane waterfall loop: ~12 instructions per memory op, one loop
// finished before the next op issues.
// Both values are workgroup-uniform on every path: they are functions of the
// unit index and of kernel arguments / descriptor words read at uniform
// addresses, and the unit index is blockIdx.x + k * gridDim.x (static
// schedule, k_program) or a ticket that thread 0 stored to s_next[] before
// the barrier every lane read it behind (for_each_unit).  tile_order (any
// `order`) and the clamp of the last, partial unit are pure functions of
// those; a scalar-only compute returns before it gets here, on a uniform
// branch.
template <class Op, int U, int POL, int ENG, bool PACED = false, class Inputs, class Hook = NoHook>
__device__ __forceinline__ void unit_body(char *outb, Inputs in, uint32_t n, uint64_t off,
                                          uint32_t nbytes, const uint32_t (&voff)[U], Hook hook = Hook(),
                                          fin_t<Op> fin = {}) {
  const uint64_t uoff = uniform64(off);
  const uint32_t ubytes = uniform32(nbytes);
  if constexpr (ENG == kPhase)
    chunk_body<Op, U, POL>(outb, in, n, uoff, ubytes, voff, hook, fin);
  else
    tile_body<Op, U, POL, PACED>(outb, in, n, uoff, ubytes, voff, hook, fin);
}

// Body inputs shifted by the head: base(k) = in[k] + head*esz.
template <class Inner>
struct Shifted {
  Inner in;
  uint64_t shift;
  __device__ const char *operator()(int k) const { return in(k) + shift; }
  __device__ float w(int k) const { return in.w(k); }  // a weight belongs to its input, wherever the body starts
};

// ---------------------------------------------------- unit scheduling ----
//
// Static: workgroup b takes units b, b + grid, ...  Dynamic (sched != NULL):
// every workgroup takes its next unit from a device counter, so the
// workgroups the memory system serves faster do more units and the launch's
// tail is one unit instead of the slowest workgroup's share (+1.6-2.1 % on
// C2: profiles/r01_phase_probe_dyn.jsonl).  The next ticket is fetched one
// unit ahead so the atomic's latency hides under the current unit.  The
// counter pair {ticket, done} is zero on entry; the last workgroup to finish
// resets it, so consecutive launches on one stream (or replays of a graph)
// reuse it without a memset.  The host gives every (device, stream) its own
// pair and never uses it during stream capture (ticket_counter(), runtime.cpp).
__device__ __forceinline__ void drain_stores(uint32_t drain) {
  if (drain) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// The hook a unit of the dynamic schedule gets.  kDynamic lets a kernel tell
// the two schedules apart at compile time (NoHook: the static one).
template <class F>
struct TicketHook {
  static constexpr bool kDynamic = true;
  F f;
  __device__ void operator()() const { f(); }
};

template <class Body>
__device__ __forceinline__ void for_each_unit(uint32_t *sched, uint32_t grab, uint64_t t0, uint64_t t1,
                                              Body body, uint32_t drain = 0) {
  if (!sched) {
    for (uint64_t t = t0 + blockIdx.x; t < t1; t += gridDim.x) {
      body(t, NoHook());
      drain_stores(drain);
    }
    return;
  }
  // a ticket k covers units [t0 + k*grab, t0 + (k+1)*grab)
  __shared__ uint32_t s_next[2];
  if (threadIdx.x == 0)
    s_next[0] = __hip_atomic_fetch_add(&sched[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  uint64_t t = t0 + (uint64_t)s_next[0] * grab;
  int slot = 1;
  while (t < t1) {
    // the next ticket is grabbed before this one's loads; its value is
    // published after the last unit's last add and before that unit's stores
    // (the body's hook), where every load has been waited for, so the wait
    // costs little (a wait with stores pending is vmcnt(0))
    uint32_t nxt;  // meaningful in lane 0 only; no merge value, so no wait at the branch join
    if (threadIdx.x == 0)
      nxt = __hip_atomic_fetch_add(&sched[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t tend = (t + grab < t1) ? t + grab : t1;
    for (uint64_t u = t; u < tend; u++) {
      const bool last = u + 1 == tend;
      auto publish = [&]() {
        if (last && threadIdx.x == 0) s_next[slot] = nxt;
      };
      body(u, TicketHook<decltype(publish)>{publish});
      drain_stores(drain);
    }
    __syncthreads();
    t = t0 + (uint64_t)s_next[slot] * grab;
    slot ^= 1;
  }
  if (threadIdx.x == 0) {
    // every ticket grab of this workgroup precedes its done increment
    const uint32_t prev = __hip_atomic_fetch_add(&sched[1], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == gridDim.x - 1) {  // last workgroup: no grab is outstanding
      __hip_atomic_store(&sched[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&sched[1], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// Tile order: unit t of a launch of n units runs tile tile_order(t).  With
// 2^L segments the order interleaves them -- consecutive units (the ones in
// flight together across the chip) spread over 2^L equal stretches of every
// input instead of one contiguous window -- a bijection on [0, n) for any n
// (segment s holds q + (s < r) tiles, q = n >> L, r = n mod 2^L; the last r
// units are the long segments' extra tiles).  L = 0: linear.
__device__ __forceinline__ uint64_t tile_order(uint64_t t, uint64_t n, uint32_t L) {
  if (!L) return t;
  const uint64_t S = 1ull << L, q = n >> L, r = n & (S - 1);
  uint64_t seg, idx;
  if (t < (q << L)) {
    seg = t & (S - 1);
    idx = t >> L;
  } else {
    seg = t - (q << L);
    idx = q;
  }
  return seg * q + (seg < r ? seg : r) + idx;
}

// ------------------------------------------------------------ kernels ------

// The one-shot kernel's body; `fin`: the scale of a scaled sum (NoFin otherwise).
template <class Op, int BLOCK, int U, int POL, int ENG>
__device__ __forceinline__ void single_kernel(const SingleArgs &a, fin_t<Op> fin) {
  const int tid = threadIdx.x;
  uint32_t voff[U];
#pragma unroll
  for (int u = 0; u < U; u++) voff[u] = (uint32_t)((u * BLOCK + tid) * kPacket);
  ArgInputs raw{a.in};
  if (blockIdx.x == 0) scalar_part<Op>(a.out, raw, a.n, a.head, a.npkt, a.tail, tid, fin);
  if (a.npkt == 0) return;  // (the host never passes a sched counter then)
  const uint64_t shift = (uint64_t)a.head * Op::kEsz;
  Shifted<ArgInputs> in{raw, shift};
  char *outb = a.out + (uint64_t)a.head * out_esz<Op>();
  constexpr uint64_t TILE = (uint64_t)BLOCK * U;
  for_each_unit(a.sched, a.grab, 0, a.ntiles, [&](uint64_t u, auto hook) {
    const uint64_t t = tile_order(u, a.ntiles, a.order);
    const uint64_t pkt0 = t * TILE;
    const uint64_t left = a.npkt - pkt0;
    const uint32_t tile_bytes = (uint32_t)((left < TILE ? left : TILE) * kPacket);
    // the dynamic schedule's tiles pace their load burst (group_at)
    unit_body<Op, U, POL, ENG, decltype(hook)::kDynamic>(outb, in, a.n, pkt0 * kPacket, tile_bytes, voff, hook, fin);
  }, a.drain);
}

template <class Op, int BLOCK, int U, int POL, int ENG>
__global__ __launch_bounds__(BLOCK) void k_reduce_single(SingleArgs a) {
  single_kernel<Op, BLOCK, U, POL, ENG>(a, NoFin());
}

// The scaled sums' kernel: the same body with the op's alpha, which arrives in
// the kernel arguments (scalar loads: it stays in SGPRs).
template <class Op, int BLOCK, int U, int POL, int ENG>
__global__ __launch_bounds__(BLOCK) void k_reduce_single_scaled(SingleArgsScaled a) {
  single_kernel<Op, BLOCK, U, POL, ENG>(a, Op::fin(a.scale));
}

// The plan's device pointer table is read through the constant address space
// (4): the loads are then scalar (s_load) and the pointers known uniform.
// Through a generic pointer the compiler emits a flat load -- whose
// s_waitcnt vmcnt(0) drains every buffer load in flight -- and a
// readfirstlane waterfall loop around every buffer load using the pointer.
typedef const char *const __attribute__((address_space(4))) ConstPtr;

struct TableInputs {
  const char *const *p;
  __device__ const char *operator()(int k) const { return ((ConstPtr *)p)[k]; }
};

struct TableInputsWeighted : TableInputs {
  const float *wp;
  __device__ float w(int k) const { return ((ConstF32 *)wp)[k]; }
};

typedef const PlanDesc __attribute__((address_space(4))) ConstDesc;
typedef const uint32_t __attribute__((address_space(4))) ConstU32;

__device__ __forceinline__ PlanDesc load_desc(const PlanDesc *desc, uint32_t c) {
  const ConstDesc *q = (const ConstDesc *)desc + c;  // scalar loads
  PlanDesc d;
  d.out = q->out;
  d.npkt = q->npkt;
  d.tile_begin = q->tile_begin;
  d.n = q->n;
  d.head = q->head;
  d.tail = q->tail;
  d.pad = 0;
  return d;
}

// All computes of a plan in one launch.  Global unit t belongs to compute
// unit_comp[t] (the host's table: one scalar load, instead of a search over
// the computes' first units whose dependent probes cost several
// microseconds in the first unit of every workgroup of a small plan).
template <class Op, int BLOCK, int U, int POL, int ENG>
__global__ __launch_bounds__(BLOCK) void k_reduce_plan(PlanArgs a) {
  const int tid = threadIdx.x;
  uint32_t voff[U];
#pragma unroll
  for (int u = 0; u < U; u++) voff[u] = (uint32_t)((u * BLOCK + tid) * kPacket);
  constexpr uint64_t TILE = (uint64_t)BLOCK * U;
  for_each_unit(a.sched, a.grab, a.t_begin, a.t_end, [&](uint64_t t, auto hook) {
    const uint32_t c = a.unit_comp ? ((ConstU32 *)a.unit_comp)[t] : 0u;
    const PlanDesc d = load_desc(a.desc, c);
    const uint64_t lt = t - d.tile_begin;
    TableInputs raw{a.ptrs + (uint64_t)c * a.stride};
    if (lt == 0) scalar_part<Op, POL>(d.out, raw, d.n, d.head, d.npkt, d.tail, tid);
    const uint64_t pkt0 = lt * TILE;
    if (pkt0 >= d.npkt) {  // a scalar-only compute: nothing to load or store
      hook();
      return;
    }
    const uint64_t shift = (uint64_t)d.head * Op::kEsz;
    Shifted<TableInputs> in{raw, shift};
    const uint64_t left = d.npkt - pkt0;
    const uint32_t tile_bytes = (uint32_t)((left < TILE ? left : TILE) * kPacket);
    unit_body<Op, U, POL, ENG>(d.out + shift, in, d.n, pkt0 * kPacket, tile_bytes, voff, hook);
  });
}

// The scaled sums' plan kernel: k_reduce_plan (above) with the op's alpha from
// the kernel arguments.  The two bodies are kept apart on purpose: moved into
// one shared function, k_reduce_plan's instantiations came out with another
// register allocation (and 3-4 instructions fewer), and the kernels of the
// existing code objects are to stay instruction for instruction what they were.
template <class Op, int BLOCK, int U, int POL, int ENG>
__global__ __launch_bounds__(BLOCK) void k_reduce_plan_scaled(PlanArgsScaled a) {
  const fin_t<Op> fin = Op::fin(a.scale);
  const int tid = threadIdx.x;
  uint32_t voff[U];
#pragma unroll
  for (int u = 0; u < U; u++) voff[u] = (uint32_t)((u * BLOCK + tid) * kPacket);
  constexpr uint64_t TILE = (uint64_t)BLOCK * U;
  for_each_unit(a.sched, a.grab, a.t_begin, a.t_end, [&](uint64_t t, auto hook) {
    const uint32_t c = a.unit_comp ? ((ConstU32 *)a.unit_comp)[t] : 0u;
    const PlanDesc d = load_desc(a.desc, c);
    const uint64_t lt = t - d.tile_begin;
    TableInputs raw{a.ptrs + (uint64_t)c * a.stride};
    if (lt == 0) scalar_part<Op, POL>(d.out, raw, d.n, d.head, d.npkt, d.tail, tid, fin);
    const uint64_t pkt0 = lt * TILE;
    if (pkt0 >= d.npkt) {  // a scalar-only compute: nothing to load or store
      hook();
      return;
    }
    const uint64_t shift = (uint64_t)d.head * Op::kEsz;
    Shifted<TableInputs> in{raw, shift};
    const uint64_t left = d.npkt - pkt0;
    const uint32_t tile_bytes = (uint32_t)((left < TILE ? left : TILE) * kPacket);
    unit_body<Op, U, POL, ENG>(d.out + (uint64_t)d.head * out_esz<Op>(), in, d.n, pkt0 * kPacket, tile_bytes, voff, hook,
                               fin);
  });
}

// The MIXED plan kernel (kOpMixedSum): k_reduce_plan_scaled whose computes are
// scaled or not one by one -- PlanDesc.pad bit 3 (kDescUnscaled) set: this
// compute writes the plain sum.  A step of an averaging Comm<T> holds final
// computes (scaled) next to intermediate ones (plain) and stays one launch.
// The unit's finishing factor is alpha or ONE: the descriptor word is a scalar
// load and the choice a scalar select, so no lane diverges and the unit's code
// is the scaled kernel's.  Multiplying by one gives the plain sum's word for
// every non-NaN sum (fl(s * 1) = s, subnormals and signed zeros included;
// round_T(fl32(widen(s) * 1)) = s because widen is exact and s is in T's
// range; with an f32 accumulator round_T(s32), the WIDE sum), and a NaN stays
// a NaN.  A third body of its own, like the two above and for their reason.
template <class Op, int BLOCK, int U, int POL, int ENG>
__global__ __launch_bounds__(BLOCK) void k_reduce_plan_mixed(PlanArgsScaled a) {
  const fin_t<Op> fin_alpha = Op::fin(a.scale);
  const fin_t<Op> fin_one = Op::fin(Scale{1.0, 1.0f, 0u});
  const int tid = threadIdx.x;
  uint32_t voff[U];
#pragma unroll
  for (int u = 0; u < U; u++) voff[u] = (uint32_t)((u * BLOCK + tid) * kPacket);
  constexpr uint64_t TILE = (uint64_t)BLOCK * U;
  for_each_unit(a.sched, a.grab, a.t_begin, a.t_end, [&](uint64_t t, auto hook) {
    const uint32_t c = a.unit_comp ? ((ConstU32 *)a.unit_comp)[t] : 0u;
    const PlanDesc d = load_desc(a.desc, c);
    const uint32_t flags = ((const ConstDesc *)a.desc + c)->pad;  // scalar load, with the descriptor's other words
    const fin_t<Op> fin = (flags & kDescUnscaled) ? fin_one : fin_alpha;
    const uint64_t lt = t - d.tile_begin;
    TableInputs raw{a.ptrs + (uint64_t)c * a.stride};
    if (lt == 0) scalar_part<Op, POL>(d.out, raw, d.n, d.head, d.npkt, d.tail, tid, fin);
    const uint64_t pkt0 = lt * TILE;
    if (pkt0 >= d.npkt) {  // a scalar-only compute: nothing to load or store
      hook();
      return;
    }
    const uint64_t shift = (uint64_t)d.head * Op::kEsz;
    Shifted<TableInputs> in{raw, shift};
    const uint64_t left = d.npkt - pkt0;
    const uint32_t tile_bytes = (uint32_t)((left < TILE ? left : TILE) * kPacket);
    unit_body<Op, U, POL, ENG>(d.out + (uint64_t)d.head * out_esz<Op>(), in, d.n, pkt0 * kPacket, tile_bytes, voff, hook,
                               fin);
  });
}

// The weighted sums' kernels (OpWeighted, OpWeightedAccum): the scaled kernels'
// bodies over inputs that carry their weights -- the one-shot kernel takes the
// weight pointer behind the scaled kernel's arguments, the plan kernel a device
// table of one weight pointer per compute (read with the compute's descriptor:
// scalar loads).  Head, body and tail of a compute read the same n floats.
// Bodies of their own, as the three above and for their reason.
template <class Op, int BLOCK, int U, int POL, int ENG>
__global__ __launch_bounds__(BLOCK) void k_reduce_single_weighted(SingleArgsWeighted a) {
  const fin_t<Op> fin = Op::fin(a.scale);
  const int tid = threadIdx.x;
  uint32_t voff[U];
#pragma unroll
  for (int u = 0; u < U; u++) voff[u] = (uint32_t)((u * BLOCK + tid) * kPacket);
  ArgInputsWeighted raw{{a.in}, a.weights};
  if (blockIdx.x == 0) scalar_part<Op>(a.out, raw, a.n, a.head, a.npkt, a.tail, tid, fin);
  if (a.npkt == 0) return;  // (the host never passes a sched counter then)
  const uint64_t shift = (uint64_t)a.head * Op::kEsz;
  Shifted<ArgInputsWeighted> in{raw, shift};
  char *outb = a.out + (uint64_t)a.head * out_esz<Op>();
  constexpr uint64_t TILE = (uint64_t)BLOCK * U;
  for_each_unit(a.sched, a.grab, 0, a.ntiles, [&](uint64_t u, auto hook) {
    const uint64_t t = tile_order(u, a.ntiles, a.order);
    const uint64_t pkt0 = t * TILE;
    const uint64_t left = a.npkt - pkt0;
    const uint32_t tile_bytes = (uint32_t)((left < TILE ? left : TILE) * kPacket);
    unit_body<Op, U, POL, ENG, decltype(hook)::kDynamic>(outb, in, a.n, pkt0 * kPacket, tile_bytes, voff, hook, fin);
  }, a.drain);
}

typedef const float *const __attribute__((address_space(4))) ConstWeightPtr;

template <class Op, int BLOCK, int U, int POL, int ENG>
__global__ __launch_bounds__(BLOCK) void k_reduce_plan_weighted(PlanArgsWeighted a) {
  const fin_t<Op> fin = Op::fin(a.scale);
  const int tid = threadIdx.x;
  uint32_t voff[U];
#pragma unroll
  for (int u = 0; u < U; u++) voff[u] = (uint32_t)((u * BLOCK + tid) * kPacket);
  constexpr uint64_t TILE = (uint64_t)BLOCK * U;
  for_each_unit(a.sched, a.grab, a.t_begin, a.t_end, [&](uint64_t t, auto hook) {
    const uint32_t c = a.unit_comp ? ((ConstU32 *)a.unit_comp)[t] : 0u;
    const PlanDesc d = load_desc(a.desc, c);
    const uint64_t lt = t - d.tile_begin;
    TableInputsWeighted raw{{a.ptrs + (uint64_t)c * a.stride}, ((ConstWeightPtr *)a.weights)[c]};
    if (lt == 0) scalar_part<Op, POL>(d.out, raw, d.n, d.head, d.npkt, d.tail, tid, fin);
    const uint64_t pkt0 = lt * TILE;
    if (pkt0 >= d.npkt) {  // a scalar-only compute: nothing to load or store
      hook();
      return;
    }
    const uint64_t shift = (uint64_t)d.head * Op::kEsz;
    Shifted<TableInputsWeighted> in{raw, shift};
    const uint64_t left = d.npkt - pkt0;
    const uint32_t tile_bytes = (uint32_t)((left < TILE ? left : TILE) * kPacket);
    unit_body<Op, U, POL, ENG>(d.out + (uint64_t)d.head * out_esz<Op>(), in, d.n, pkt0 * kPacket, tile_bytes, voff, hook,
                               fin);
  });
}

// ------------------------------------------------------------ step programs --
//
// A stream-ordered pipeline step is a short ordered list: ready-token phases,
// the transport's batched copies, done-token phases, the step's reductions,
// the fused transfers' done tokens.  Launched one by one that is a
// k_sigwait_phases before every copy or reduction kernel.  A PROGRAM folds
// the signal/wait phases that precede a batch of units into that batch's
// kernel as a PROLOGUE: workgroup 0's first wave runs the phases in order
// (system-scope release stores of the epochs, bounded acquire spins -- as
// k_sigwait_phases), then publishes the launch's sequence number in the
// program's gate word; every other workgroup waits for that word before its
// first unit.  The units are the tiles of the batch's computes (reductions in
// the program's type, or exact byte copies), statically interleaved over the
// grid like the plan kernel.
//
// Measured alternative (round 3, profiles/r03f_progstep_*.jsonl): running a
// whole step -- several unit batches with completion gates between them --
// in one launch.  Completions then need grid-wide counting (atomics on one
// line from every workgroup) and, MI355X's L2 being per XCD, a system-scope
// L2 writeback per workgroup before each count and an invalidate after each
// gate: 40-170 us per step against 18-22 us for the separate launches.  A
// kernel boundary does that cache maintenance once per XCD.  So units that
// depend on other units stay in separate launches; only the token phases
// move into the kernels.
//
// Coherence of the prologue: no unit of the launch touches its data before
// the gate opens, so the data the phases waited for (peers' writes over
// xGMI) is read after it arrived, as it is by a kernel launched after a
// separate k_sigwait_phases; the launch's own stores are released at its
// end like any kernel's.

constexpr int kProgPol = kDefPol;  // nt loads, nt stores (the library's default policy)

// Phases [0, count) on one wave (lanes = flags), as k_sigwait_phases.
//
// `light` (opt-in, HICCL_PROG_FENCES=light): relaxed system-scope token stores
// and no fence after the waits.  A program's tokens never publish data of
// their own launch -- a done token follows the copies or reductions of an
// EARLIER launch (complete, and released, at that kernel's end; a peer's
// buffer written through with the peer policy), a ready token only says a
// buffer an earlier launch read is free -- and this launch's units start
// after the gate, on workgroups whose L1 holds none of their data (the
// kernel-start acquire invalidated it and nothing read it since).  The wave
// issues a phase's stores only after its polls of the previous phase have
// returned (the loop exits on the loaded value).  Fenced mode (the
// default: release stores, an acquire fence per phase after relaxed polls, a
// release gate store) orders workgroup 0 after the peers by the memory model,
// and the other workgroups after workgroup 0 by an agent-scope acquire after
// their gate polls (k_program); light mode leaves the gate hand-off relaxed.
__device__ __forceinline__ void prog_phases(const ProgArgs &a, uint32_t count, uint32_t lane, uint32_t add) {
  for (uint32_t p = 0; p < count; p++) {
    const ConstU32 *q = (const ConstU32 *)&a.phase[p];
    const uint32_t s0 = q[0], s1 = q[1], w0 = q[2], w1 = q[3];
    const uint32_t epoch = a.epoch[p] + add;
    for (uint32_t i = s0 + lane; i < s1; i += 64) {
      uint32_t *f = ((uint32_t *const __attribute__((address_space(4))) *)a.sig)[i];
      if (a.light)
        __hip_atomic_store(f, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      else
        __hip_atomic_store(f, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    for (uint32_t i = w0 + lane; i < w1; i += 64) {
      const uint32_t *f = ((const uint32_t *const __attribute__((address_space(4))) *)a.wait)[i];
      const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
      // relaxed polls (no cache invalidate per poll); the fence below acquires
      while ((int32_t)(__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) - epoch) < 0) {
        __builtin_amdgcn_s_sleep(2);
        if (a.err && __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) break;
        if (__builtin_amdgcn_s_memrealtime() - t0 > a.timeout_ticks) {
          if (a.err) __hip_atomic_store(a.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          break;
        }
      }
    }
    // fenced mode: each lane's acquire half of its polls, after its last
    // poll; then every lane's waits (and acquires) precede any store of the
    // next phase -- a wave-level barrier whose wavefront-scope fences carry
    // the ordering from lane to lane (only this wave runs the phases, so no
    // workgroup barrier is available here)
    if (!a.light) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

// Bounded wait of one lane until the gate word holds this launch's `seq`;
// on a time-out or an error recorded by anyone it gives up (the grid drains,
// the host reports the error).  Relaxed polls with backoff: hundreds of
// workgroups poll one line.  Equality, not >=: the word holds the previous
// launch's value until workgroup 0 stores ours, and no two launches of a
// program share a value (64-bit, hiccl_program_launch), so a later eager
// launch's value can never open a replay's gate early.
__device__ __forceinline__ void prog_gate_wait(const ProgArgs &a, uint64_t seq) {
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  uint32_t nap = 1;
  while (__hip_atomic_load(a.gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != seq) {
    for (uint32_t i = 0; i < nap; i++) __builtin_amdgcn_s_sleep(2);
    if (nap < 8) nap <<= 1;
    if (a.err && __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) return;
    if (__builtin_amdgcn_s_memrealtime() - t0 > a.timeout_ticks) {
      if (a.err) __hip_atomic_store(a.err, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      return;
    }
  }
}

template <class Op, int U, int POL>
__device__ __forceinline__ void prog_unit_of(const PlanDesc &d, TableInputs raw, uint64_t lt, int tid,
                                             const uint32_t (&voff)[U]) {
  constexpr uint64_t TILE = (uint64_t)kProgBlock * U;
  if (lt == 0) scalar_part<Op, POL>(d.out, raw, d.n, d.head, d.npkt, d.tail, tid);
  const uint64_t pkt0 = lt * TILE;
  if (pkt0 >= d.npkt) return;
  const uint64_t shift = (uint64_t)d.head * Op::kEsz;
  Shifted<TableInputs> in{raw, shift};
  const uint64_t left = d.npkt - pkt0;
  const uint32_t tile_bytes = (uint32_t)((left < TILE ? left : TILE) * kPacket);
  unit_body<Op, U, POL, kTile>(d.out + shift, in, d.n, pkt0 * kPacket, tile_bytes, voff);
}

// A unit under its compute's peer policy (the plan's hiccl_reduce_plan_set_peer
// flags, kept in the descriptor: bit 0 stores, bit 1 loads; workgroup-uniform).
template <class Op, int U>
__device__ __forceinline__ void prog_unit_peer(uint32_t peer, const PlanDesc &d, TableInputs raw, uint64_t lt,
                                               int tid, const uint32_t (&voff)[U]) {
  constexpr int L = kProgPol % 10, S = kProgPol / 10;
  switch (peer & 3u) {
    case 0: prog_unit_of<Op, U, kProgPol>(d, raw, lt, tid, voff); break;
    case 1: prog_unit_of<Op, U, 10 * kPolStoreSys + L>(d, raw, lt, tid, voff); break;
    case 2: prog_unit_of<Op, U, 10 * S + kPolLoadSys>(d, raw, lt, tid, voff); break;
    default: prog_unit_of<Op, U, 10 * kPolStoreSys + kPolLoadSys>(d, raw, lt, tid, voff); break;
  }
}

template <class Op, int U>
__global__ __launch_bounds__(kProgBlock) void k_program(ProgArgs a) {
  const int tid = threadIdx.x;
  uint32_t voff[U];
#pragma unroll
  for (int u = 0; u < U; u++) voff[u] = (uint32_t)((u * kProgBlock + tid) * kPacket);
  if (a.nphase) {
    const uint32_t add = a.epoch_dev ? __hip_atomic_load(a.epoch_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    const uint64_t seq = a.seq + add;
    if (blockIdx.x == 0) {
      if (tid < 64) {
        prog_phases(a, a.nphase, (uint32_t)tid, add);
        if (tid == 0) {
          if (a.light)
            __hip_atomic_store(a.gate, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          else
            __hip_atomic_store(a.gate, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    } else if (tid == 0) {
      prog_gate_wait(a, seq);
      // Fenced mode: an agent-scope acquire closes the relaxed gate polls,
      // pairing with workgroup 0's agent-scope release store of the gate,
      // which follows workgroup 0's system-scope acquire of the peers'
      // tokens.  That orders this workgroup after the tokens for writes made
      // on THIS GPU.  It is not a guarantee for a peer GPU's writes: on a
      // part with several XCDs workgroup 0's system-scope acquire
      // invalidates only its own XCD's L2, and an agent-scope acquire on
      // another XCD does not drop non-coherent L2 lines there.  Peer data
      // stays visible because no L2 holds a line of it (peer puts store
      // write-through, HICCL_PEER_STORES; fused reads load system-scope,
      // HICCL_PEER_LOADS; and the kernel-start invalidate) -- the same
      // cache argument `light` rests on, and unconfirmed until a run with
      // one GPU per rank.  Agent scope, not system: a system-scope acquire
      // per workgroup (1,024 L2 invalidations per launch) cost ~8 us per
      // C5 step (profiles/r04f_progstep.jsonl).  The workgroup barrier
      // below carries it to the other lanes.
      if (!a.light) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
  }
  for (uint64_t t = blockIdx.x; t < a.nunits; t += gridDim.x) {
    const uint32_t c = a.unit_comp ? ((ConstU32 *)a.unit_comp)[t] : 0u;
    const ConstDesc *q = (const ConstDesc *)a.desc + c;
    const PlanDesc d = load_desc(a.desc, c);
    const uint32_t flags = q->pad;  // bit 0: exact byte copy; bits 1-2: peer stores / peer loads
    TableInputs raw{a.ptrs + (uint64_t)c * a.stride};
    if (flags & 1u)
      prog_unit_peer<OpRaw, U>(flags >> 1, d, raw, t - d.tile_begin, tid, voff);
    else
      prog_unit_peer<Op, U>(flags >> 1, d, raw, t - d.tile_begin, tid, voff);
  }
}

// ------------------------------------------------------- kernel tables ----

// The one list of element types: (dtype, acc, op) -> (element op, tuned).  The
// headline types (f32, bf16 and f16 with the native accumulator) under SUM are
// TUNED: they get the full tuning table, the others -- every MAX / MIN, PROD
// and bitwise op among them -- every engine's default shape.  Every per-dtype
// lookup below goes through it.  PART names the part of the list a translation
// unit instantiates (engine.h's head): a key of another part answers `unknown`.
template <int DT, class O, bool TUNED>
struct Elem {
  static constexpr int dtype = DT;
  typedef O Op;
  static constexpr bool tuned = TUNED;
};

constexpr int kPartSum = 0;
constexpr int kPartMaxMin = 1;
constexpr int kPartProd = 2;  // PROD, BAND, BOR, BXOR
constexpr int kPartScale = 3;  // post-scaled sums (kOpScaledSum)
constexpr int kPartF8 = 4;  // the OCP FP8 types, every operator they have
constexpr int kPartWiden = 5;  // widened sums (kOpWidenSum): 2-byte and FP8 inputs, f32 output
constexpr int kPartAccum = 6;  // accumulating widened sums (kOpWidenAccum): out += alpha * sum
constexpr int kPartMixed = 7;  // mixed plans (kOpMixedSum): the scaled ops of all six floating types, plan kernels only

// MAX and MIN of the six arithmetic types; HICCL_BYTES has no operator.
template <bool MAX, class R, class F>
R with_elem_mm(int dtype, R unknown, F f) {
  switch (dtype) {
    case HICCL_FLOAT32: return f(Elem<HICCL_FLOAT32, OpF32MM<MAX>, false>());
    case HICCL_BFLOAT16: return f(Elem<HICCL_BFLOAT16, OpBF16MM<MAX>, false>());
    case HICCL_FLOAT16: return f(Elem<HICCL_FLOAT16, OpF16MM<MAX>, false>());
    case HICCL_FLOAT64: return f(Elem<HICCL_FLOAT64, OpF64MM<MAX>, false>());
    case HICCL_UINT64: return f(Elem<HICCL_UINT64, OpU64MM<MAX>, false>());
    case HICCL_INT32: return f(Elem<HICCL_INT32, OpI32MM<MAX>, false>());
    default: return unknown;
  }
}

template <class R, class F>
R with_elem_sum(int dtype, int acc, R unknown, F f) {
  switch (dtype) {
    case HICCL_FLOAT32: return f(Elem<HICCL_FLOAT32, OpF32, true>());
    case HICCL_BFLOAT16:
      return acc == HICCL_ACC_WIDE ? f(Elem<HICCL_BFLOAT16, OpBF16Wide, false>())
                                   : f(Elem<HICCL_BFLOAT16, OpBF16, true>());
    case HICCL_FLOAT16:
      return acc == HICCL_ACC_WIDE ? f(Elem<HICCL_FLOAT16, OpF16Wide, false>())
                                   : f(Elem<HICCL_FLOAT16, OpF16, true>());
    case HICCL_FLOAT64: return f(Elem<HICCL_FLOAT64, OpF64, false>());
    case HICCL_UINT64: return f(Elem<HICCL_UINT64, OpU64, false>());
    case HICCL_INT32: return f(Elem<HICCL_INT32, OpI32, false>());
    case HICCL_BYTES: return f(Elem<HICCL_BYTES, OpRaw, false>());
    default: return unknown;
  }
}

// PROD of the six arithmetic types.
template <class R, class F>
R with_elem_prod(int dtype, R unknown, F f) {
  switch (dtype) {
    case HICCL_FLOAT32: return f(Elem<HICCL_FLOAT32, OpF32Prod, false>());
    case HICCL_BFLOAT16: return f(Elem<HICCL_BFLOAT16, OpBF16Prod, false>());
    case HICCL_FLOAT16: return f(Elem<HICCL_FLOAT16, OpF16Prod, false>());
    case HICCL_FLOAT64: return f(Elem<HICCL_FLOAT64, OpF64Prod, false>());
    case HICCL_UINT64: return f(Elem<HICCL_UINT64, OpU64Fold<kIntProd>, false>());
    case HICCL_INT32: return f(Elem<HICCL_INT32, OpI32Fold<kIntProd>, false>());
    default: return unknown;
  }
}

// BAND / BOR / BXOR: the two integer types only.
template <int OP, class R, class F>
R with_elem_bit(int dtype, R unknown, F f) {
  switch (dtype) {
    case HICCL_UINT64: return f(Elem<HICCL_UINT64, OpU64Fold<OP>, false>());
    case HICCL_INT32: return f(Elem<HICCL_INT32, OpI32Fold<OP>, false>());
    default: return unknown;
  }
}

// Scaled sums: the floating types, under either accumulator for the 2-byte
// ones.  Untuned, like every operator but SUM.
template <class R, class F>
R with_elem_scale(int dtype, int acc, R unknown, F f) {
  const bool wide = acc == HICCL_ACC_WIDE;
  switch (dtype) {
    case HICCL_FLOAT32: return f(Elem<HICCL_FLOAT32, OpF32Scaled, false>());
    case HICCL_FLOAT64: return f(Elem<HICCL_FLOAT64, OpF64Scaled, false>());
    case HICCL_BFLOAT16:
      return wide ? f(Elem<HICCL_BFLOAT16, OpBF16WideScaled, false>()) : f(Elem<HICCL_BFLOAT16, OpBF16NatScaled, false>());
    case HICCL_FLOAT16:
      return wide ? f(Elem<HICCL_FLOAT16, OpF16WideScaled, false>()) : f(Elem<HICCL_FLOAT16, OpF16NatScaled, false>());
    default: return unknown;
  }
}

// The two OCP FP8 types: every operator they have -- SUM under either
// accumulator, MAX, MIN and the scaled sums -- is one part (kPartF8,
// reduce_f8.hip), and the lists above do not know the types.  Untuned.
inline bool is_f8(int dtype) { return dtype == HICCL_FLOAT8_E4M3 || dtype == HICCL_FLOAT8_E5M2; }

template <int FMT, int DT, class R, class F>
R with_elem_f8_fmt(int acc, int op, R unknown, F f) {
  const bool wide = acc == HICCL_ACC_WIDE;
  switch (op) {
    case HICCL_OP_SUM: return wide ? f(Elem<DT, OpF8Wide<FMT>, false>()) : f(Elem<DT, OpF8<FMT>, false>());
    case kOpScaledSum:
      return wide ? f(Elem<DT, OpF8Scaled<OpF8Wide<FMT>, FMT>, false>())
                  : f(Elem<DT, OpF8Scaled<OpF8<FMT>, FMT>, false>());
    case HICCL_OP_MAX: return wide ? unknown : f(Elem<DT, OpF8MM<true, FMT>, false>());
    case HICCL_OP_MIN: return wide ? unknown : f(Elem<DT, OpF8MM<false, FMT>, false>());
    default: return unknown;  // no PROD and no bitwise operator on FP8
  }
}

template <class R, class F>
R with_elem_f8(int dtype, int acc, int op, R unknown, F f) {
  switch (dtype) {
    case HICCL_FLOAT8_E4M3: return with_elem_f8_fmt<kE4M3, HICCL_FLOAT8_E4M3>(acc, op, unknown, f);
    case HICCL_FLOAT8_E5M2: return with_elem_f8_fmt<kE5M2, HICCL_FLOAT8_E5M2>(acc, op, unknown, f);
    default: return unknown;
  }
}

// Widened sums: the dtype is the INPUTS' (the output is f32), the accumulator
// is the op's own (acc must be native: the host refuses HICCL_ACC_WIDE).
// Untuned, and FP8 inputs come here too, not to kPartF8.
template <class R, class F>
R with_elem_widen(int dtype, int acc, R unknown, F f) {
  if (acc != HICCL_ACC_NATIVE) return unknown;
  switch (dtype) {
    case HICCL_BFLOAT16: return f(Elem<HICCL_BFLOAT16, OpBF16ToF32, false>());
    case HICCL_FLOAT16: return f(Elem<HICCL_FLOAT16, OpF16ToF32, false>());
    case HICCL_FLOAT8_E4M3: return f(Elem<HICCL_FLOAT8_E4M3, OpF8ToF32<kE4M3>, false>());
    case HICCL_FLOAT8_E5M2: return f(Elem<HICCL_FLOAT8_E5M2, OpF8ToF32<kE5M2>, false>());
    default: return unknown;
  }
}

// Accumulating widened sums (kOpWidenAccum): the widened sums' list with the
// accumulating ops.  Untuned.
template <class R, class F>
R with_elem_accum(int dtype, int acc, R unknown, F f) {
  if (acc != HICCL_ACC_NATIVE) return unknown;
  switch (dtype) {
    case HICCL_BFLOAT16: return f(Elem<HICCL_BFLOAT16, OpBF16AccF32, false>());
    case HICCL_FLOAT16: return f(Elem<HICCL_FLOAT16, OpF16AccF32, false>());
    case HICCL_FLOAT8_E4M3: return f(Elem<HICCL_FLOAT8_E4M3, OpF8AccF32<kE4M3>, false>());
    case HICCL_FLOAT8_E5M2: return f(Elem<HICCL_FLOAT8_E5M2, OpF8AccF32<kE5M2>, false>());
    default: return unknown;
  }
}

// Weighted widened sums (kOpWeightedSum, kOpWeightedAccum): the same list with
// the weighted ops.  Untuned; a list of its own, not a part of with_elem -- its
// kernels have argument structs and launcher types of their own.
template <class R, class F>
R with_elem_weighted(int dtype, int acc, int op, R unknown, F f) {
  if (acc != HICCL_ACC_NATIVE) return unknown;
  if (op == kOpWeightedSum) {
    switch (dtype) {
      case HICCL_BFLOAT16: return f(Elem<HICCL_BFLOAT16, OpWeighted<WidenBF16>, false>());
      case HICCL_FLOAT16: return f(Elem<HICCL_FLOAT16, OpWeighted<WidenF16>, false>());
      case HICCL_FLOAT8_E4M3: return f(Elem<HICCL_FLOAT8_E4M3, OpWeighted<WidenF8<kE4M3>>, false>());
      case HICCL_FLOAT8_E5M2: return f(Elem<HICCL_FLOAT8_E5M2, OpWeighted<WidenF8<kE5M2>>, false>());
      default: return unknown;
    }
  }
  if (op == kOpWeightedAccum) {
    switch (dtype) {
      case HICCL_BFLOAT16: return f(Elem<HICCL_BFLOAT16, OpWeightedAccum<WidenBF16>, false>());
      case HICCL_FLOAT16: return f(Elem<HICCL_FLOAT16, OpWeightedAccum<WidenF16>, false>());
      case HICCL_FLOAT8_E4M3: return f(Elem<HICCL_FLOAT8_E4M3, OpWeightedAccum<WidenF8<kE4M3>>, false>());
      case HICCL_FLOAT8_E5M2: return f(Elem<HICCL_FLOAT8_E5M2, OpWeightedAccum<WidenF8<kE5M2>>, false>());
      default: return unknown;
    }
  }
  return unknown;
}

template <int PART, class R, class F>
R with_elem(int dtype, int acc, int op, R unknown, F f) {
  if constexpr (PART == kPartMixed) {  // the scaled ops themselves, FP8's included
    if (op != kOpMixedSum) return unknown;
    const bool wide = acc == HICCL_ACC_WIDE;
    switch (dtype) {  // (not through with_elem_f8: f would be instantiated for FP8's unscaled ops too)
      case HICCL_FLOAT8_E4M3:
        return wide ? f(Elem<HICCL_FLOAT8_E4M3, OpF8Scaled<OpF8Wide<kE4M3>, kE4M3>, false>())
                    : f(Elem<HICCL_FLOAT8_E4M3, OpF8Scaled<OpF8<kE4M3>, kE4M3>, false>());
      case HICCL_FLOAT8_E5M2:
        return wide ? f(Elem<HICCL_FLOAT8_E5M2, OpF8Scaled<OpF8Wide<kE5M2>, kE5M2>, false>())
                    : f(Elem<HICCL_FLOAT8_E5M2, OpF8Scaled<OpF8<kE5M2>, kE5M2>, false>());
      default: return with_elem_scale(dtype, acc, unknown, f);
    }
  } else if constexpr (PART == kPartAccum) {
    return op == kOpWidenAccum ? with_elem_accum(dtype, acc, unknown, f) : unknown;
  } else if constexpr (PART == kPartWiden) {
    return op == kOpWidenSum ? with_elem_widen(dtype, acc, unknown, f) : unknown;
  } else if constexpr (PART == kPartF8) {
    return with_elem_f8(dtype, acc, op, unknown, f);
  } else if constexpr (PART == kPartScale) {
    return op == kOpScaledSum ? with_elem_scale(dtype, acc, unknown, f) : unknown;
  } else if constexpr (PART == kPartProd) {
    if (acc != HICCL_ACC_NATIVE) return unknown;
    switch (op) {
      case HICCL_OP_PROD: return with_elem_prod(dtype, unknown, f);
      case HICCL_OP_BAND: return with_elem_bit<kIntAnd>(dtype, unknown, f);
      case HICCL_OP_BOR: return with_elem_bit<kIntOr>(dtype, unknown, f);
      case HICCL_OP_BXOR: return with_elem_bit<kIntXor>(dtype, unknown, f);
      default: return unknown;
    }
  } else if constexpr (PART == kPartMaxMin) {
    // the f32 accumulator of HICCL_ACC_WIDE belongs to SUM alone
    if (acc != HICCL_ACC_NATIVE) return unknown;
    if (op == HICCL_OP_MAX) return with_elem_mm<true>(dtype, unknown, f);
    if (op == HICCL_OP_MIN) return with_elem_mm<false>(dtype, unknown, f);
    return unknown;
  } else {
    if (op != HICCL_OP_SUM) return unknown;
    return with_elem_sum(dtype, acc, unknown, f);
  }
}

// P of the phased engine: 16 packets per lane (acc + two in-flight loads =
// 3 x 64 VGPRs at 512 lanes) unless the accumulator is wider than a packet
// (bf16 / f16 wide: 8 floats; FP8 wide: 16 floats -- 128 VGPRs of accumulators
// and two loads of 32 in flight, 222 VGPRs as compiled) or the compiler reassociates the adds and holds more
// registers (int32: exact, so it may) -- then 8.  The chunk is a property of
// (dtype, acc): int32 takes 8 under every operator, so the host sizes a plan's
// units without asking for the operator.
// An int32 op says so itself (kHalfChunk), and so does an accumulating widened
// op (OpWidenAccum: the old output's packets are live next to the accumulators),
// the one case where the chunk depends on the operator: phase_p takes it.
template <class Op, class = void>
struct half_chunk : std::false_type {};
template <class Op>
struct half_chunk<Op, std::enable_if_t<Op::kHalfChunk>> : std::true_type {};

template <class Op>
constexpr int phase_p_of() {
  return (sizeof(typename Op::acc_t) > 16 || half_chunk<Op>::value) ? 8 : 16;
}

// ---- single-compute dispatch (template instantiation table)

template <class Op, int B, int U, int POL, int ENG = kTile>
void launch_single_t(const SingleArgsScaled &a, dim3 grid, hipStream_t s) {
  if constexpr (std::is_same<fin_t<Op>, NoFin>::value)
    hipLaunchKernelGGL((k_reduce_single<Op, B, U, POL, ENG>), grid, dim3(B), 0, s, (const SingleArgs &)a);
  else
    hipLaunchKernelGGL((k_reduce_single_scaled<Op, B, U, POL, ENG>), grid, dim3(B), 0, s, a);
}

template <class Op, int B, int U>
single_fn pick_nt(int pol) {
  switch (pol) {
    case 0: return launch_single_t<Op, B, U, 0>;
    case 1: return launch_single_t<Op, B, U, 1>;
    case 10: return launch_single_t<Op, B, U, 10>;
    case 11: return launch_single_t<Op, B, U, 11>;
    case 20: return launch_single_t<Op, B, U, 20>;
    case 21: return launch_single_t<Op, B, U, 21>;
    case 10 * kPolStoreSys + 1: return launch_single_t<Op, B, U, 10 * kPolStoreSys + 1>;
    default: return nullptr;
  }
}

template <class Op, int B>
single_fn pick_u(int u, int pol) {
  switch (u) {
    case 1: return pick_nt<Op, B, 1>(pol);
    case 2: return pick_nt<Op, B, 2>(pol);
    case 4: return pick_nt<Op, B, 4>(pol);
    // wide tiles for few inputs (32 packets per lane in flight at n = 4 / 2)
    case 8: return pol == kDefPol && B == 256 ? launch_single_t<Op, B, 8, kDefPol> : nullptr;
    case 16: return pol == kDefPol && B == 256 ? launch_single_t<Op, B, 16, kDefPol> : nullptr;
    default: return nullptr;
  }
}

// Phased engine: the default shape for every type; the headline types also
// get the sweep shapes (chunk 64-128 KiB) and cache-policy variants.
template <class Op, bool TUNED>
single_fn pick_phase(int block, int unroll, int pol) {
  constexpr int PD = phase_p_of<Op>();
  if (block == kPhBlock && unroll == PD) {
    switch (pol) {
      case 11: return launch_single_t<Op, kPhBlock, PD, 11, kPhase>;
      case 10 * kPolStoreSys + 1: return launch_single_t<Op, kPhBlock, PD, 10 * kPolStoreSys + 1, kPhase>;
      case 1: if constexpr (TUNED) return launch_single_t<Op, kPhBlock, PD, 1, kPhase>; break;
      case 10: if constexpr (TUNED) return launch_single_t<Op, kPhBlock, PD, 10, kPhase>; break;
      case 21: if constexpr (TUNED) return launch_single_t<Op, kPhBlock, PD, 21, kPhase>; break;
      case 0: if constexpr (TUNED) return launch_single_t<Op, kPhBlock, PD, 0, kPhase>; break;
      default: break;
    }
    return nullptr;
  }
  if constexpr (TUNED) {
    if (pol != kDefPol) return nullptr;
    if (block == 1024 && unroll == 4) return launch_single_t<Op, 1024, 4, 11, kPhase>;
    if constexpr (PD == 16) {
      if (block == 512 && unroll == 8) return launch_single_t<Op, 512, 8, 11, kPhase>;
      if (block == 1024 && unroll == 8) return launch_single_t<Op, 1024, 8, 11, kPhase>;
      if (block == 256 && unroll == 16) return launch_single_t<Op, 256, 16, 11, kPhase>;
    } else {
      if (block == 512 && unroll == 4) return launch_single_t<Op, 512, 4, 11, kPhase>;
    }
  }
  return nullptr;
}

// Full tuning table for the headline types; default shape for the rest.
template <class Op, bool TUNED>
single_fn pick_single_op(int engine, int block, int unroll, int pol) {
  if (engine == HICCL_ENGINE_PHASE) return pick_phase<Op, TUNED>(block, unroll, pol);
  if constexpr (TUNED) {
    if (block == 256) return pick_u<Op, 256>(unroll, pol);
    if (block == 512) return pick_u<Op, 512>(unroll, pol);
    return nullptr;
  } else {
    if (block != kDefBlock || unroll != kDefUnroll) return nullptr;
    if (pol == 10 * kPolStoreSys + 1) return launch_single_t<Op, kDefBlock, kDefUnroll, 10 * kPolStoreSys + 1>;
    return pol == kDefPol ? launch_single_t<Op, kDefBlock, kDefUnroll, kDefPol> : nullptr;
  }
}

// ---- plan dispatch
//
// Plan kernels (and one-shot calls with > 64 inputs, which run as a
// one-compute plan) come in the PHASE engine's default shape and the TILE
// engine at 256 lanes x U packets, U = 4 for every type and also 1 or 2 for
// the headline types (f32, bf16 / f16 native).  Cache policy: nt loads and stores.

template <class Op, int ENG, int U, int POL = kDefPol>
void launch_plan_t(const PlanArgsScaled &a, dim3 grid, hipStream_t s) {
  constexpr int B = ENG == kPhase ? kPhBlock : kDefBlock;
  if constexpr (std::is_same<fin_t<Op>, NoFin>::value)
    hipLaunchKernelGGL((k_reduce_plan<Op, B, U, POL, ENG>), grid, dim3(B), 0, s, (const PlanArgs &)a);
  else
    hipLaunchKernelGGL((k_reduce_plan_scaled<Op, B, U, POL, ENG>), grid, dim3(B), 0, s, a);
}

// The plan kernels' cache policy: nt loads and stores, or a plan's peer
// policy (hiccl_reduce_plan_set_peer: system-scope stores and/or loads) --
// those in the PHASE engine's default shape and TILE at U = 4 (and 2 for the
// headline types: a pipeline step's small batches).
template <class Op, bool TUNED, int POL>
plan_fn pick_plan_pol(int engine, int unroll) {
  constexpr bool DEF = POL == kDefPol;
  if (engine == HICCL_ENGINE_PHASE) return launch_plan_t<Op, kPhase, phase_p_of<Op>(), POL>;
  switch (unroll) {
    case 0:
    case 4: return launch_plan_t<Op, kTile, 4, POL>;
    case 2: if constexpr (TUNED) return launch_plan_t<Op, kTile, 2, POL>; break;
    case 8: if constexpr (TUNED && DEF) return launch_plan_t<Op, kTile, 8>; break;
    case 16: if constexpr (TUNED && DEF) return launch_plan_t<Op, kTile, 16>; break;
    case 1: if constexpr (TUNED && DEF) return launch_plan_t<Op, kTile, 1>; break;
    default: break;
  }
  return nullptr;
}

template <class Op, bool TUNED>
plan_fn pick_plan_eng(int engine, int unroll, int pol) {
  constexpr int L = kDefPol % 10, S = kDefPol / 10;
  switch (pol) {
    case kDefPol: return pick_plan_pol<Op, TUNED, kDefPol>(engine, unroll);
    case 10 * kPolStoreSys + L: return pick_plan_pol<Op, TUNED, 10 * kPolStoreSys + L>(engine, unroll);
    case 10 * S + kPolLoadSys: return pick_plan_pol<Op, TUNED, 10 * S + kPolLoadSys>(engine, unroll);
    case 10 * kPolStoreSys + kPolLoadSys:
      return pick_plan_pol<Op, TUNED, 10 * kPolStoreSys + kPolLoadSys>(engine, unroll);
    default: return nullptr;
  }
}

// The mixed plan kernels (k_reduce_plan_mixed): the shapes the scaled plan
// kernels have -- either engine's default shape under the four plan policies
// (default, write-through stores, peer loads, both) -- and no tuning table.
template <class Op, int ENG, int U, int POL>
void launch_plan_mixed_t(const PlanArgsScaled &a, dim3 grid, hipStream_t s) {
  constexpr int B = ENG == kPhase ? kPhBlock : kDefBlock;
  hipLaunchKernelGGL((k_reduce_plan_mixed<Op, B, U, POL, ENG>), grid, dim3(B), 0, s, a);
}

template <class Op, int POL>
plan_fn pick_plan_mixed_pol(int engine, int unroll) {
  if (engine == HICCL_ENGINE_PHASE) return launch_plan_mixed_t<Op, kPhase, phase_p_of<Op>(), POL>;
  return unroll == 0 || unroll == kDefUnroll ? launch_plan_mixed_t<Op, kTile, kDefUnroll, POL> : nullptr;
}

template <class Op>
plan_fn pick_plan_mixed_eng(int engine, int unroll, int pol) {
  constexpr int L = kDefPol % 10, S = kDefPol / 10;
  switch (pol) {
    case kDefPol: return pick_plan_mixed_pol<Op, kDefPol>(engine, unroll);
    case 10 * kPolStoreSys + L: return pick_plan_mixed_pol<Op, 10 * kPolStoreSys + L>(engine, unroll);
    case 10 * S + kPolLoadSys: return pick_plan_mixed_pol<Op, 10 * S + kPolLoadSys>(engine, unroll);
    case 10 * kPolStoreSys + kPolLoadSys: return pick_plan_mixed_pol<Op, 10 * kPolStoreSys + kPolLoadSys>(engine, unroll);
    default: return nullptr;
  }
}

// The weighted kernels (k_reduce_single_weighted, k_reduce_plan_weighted): the
// shapes the widened and accumulating families have -- one-shot: either
// engine's default shape with nt or write-through stores; plan: either engine's
// default shape under the four plan policies -- and no tuning table.
template <class Op, int B, int U, int POL, int ENG>
void launch_single_weighted_t(const SingleArgsWeighted &a, dim3 grid, hipStream_t s) {
  hipLaunchKernelGGL((k_reduce_single_weighted<Op, B, U, POL, ENG>), grid, dim3(B), 0, s, a);
}

template <class Op>
single_w_fn pick_single_weighted_op(int engine, int block, int unroll, int pol) {
  constexpr int WT = 10 * kPolStoreSys + 1;
  if (engine == HICCL_ENGINE_PHASE) {
    constexpr int PD = phase_p_of<Op>();
    if (block != kPhBlock || unroll != PD) return nullptr;
    if (pol == WT) return launch_single_weighted_t<Op, kPhBlock, PD, WT, kPhase>;
    return pol == kDefPol ? launch_single_weighted_t<Op, kPhBlock, PD, kDefPol, kPhase> : nullptr;
  }
  if (block != kDefBlock || unroll != kDefUnroll) return nullptr;
  if (pol == WT) return launch_single_weighted_t<Op, kDefBlock, kDefUnroll, WT, kTile>;
  return pol == kDefPol ? launch_single_weighted_t<Op, kDefBlock, kDefUnroll, kDefPol, kTile> : nullptr;
}

template <class Op, int ENG, int U, int POL>
void launch_plan_weighted_t(const PlanArgsWeighted &a, dim3 grid, hipStream_t s) {
  constexpr int B = ENG == kPhase ? kPhBlock : kDefBlock;
  hipLaunchKernelGGL((k_reduce_plan_weighted<Op, B, U, POL, ENG>), grid, dim3(B), 0, s, a);
}

template <class Op, int POL>
plan_w_fn pick_plan_weighted_pol(int engine, int unroll) {
  if (engine == HICCL_ENGINE_PHASE) return launch_plan_weighted_t<Op, kPhase, phase_p_of<Op>(), POL>;
  return unroll == 0 || unroll == kDefUnroll ? launch_plan_weighted_t<Op, kTile, kDefUnroll, POL> : nullptr;
}

template <class Op>
plan_w_fn pick_plan_weighted_eng(int engine, int unroll, int pol) {
  constexpr int L = kDefPol % 10, S = kDefPol / 10;
  switch (pol) {
    case kDefPol: return pick_plan_weighted_pol<Op, kDefPol>(engine, unroll);
    case 10 * kPolStoreSys + L: return pick_plan_weighted_pol<Op, 10 * kPolStoreSys + L>(engine, unroll);
    case 10 * S + kPolLoadSys: return pick_plan_weighted_pol<Op, 10 * S + kPolLoadSys>(engine, unroll);
    case 10 * kPolStoreSys + kPolLoadSys: return pick_plan_weighted_pol<Op, 10 * kPolStoreSys + kPolLoadSys>(engine, unroll);
    default: return nullptr;
  }
}

// ---- program dispatch: TILE at 256 lanes x 4 packets, the headline types
// also x 2 (a pipeline step's small batches)

template <class Op, int U>
void launch_prog_t(const ProgArgs &a, dim3 grid, hipStream_t s) {
  hipLaunchKernelGGL((k_program<Op, U>), grid, dim3(kProgBlock), 0, s, a);
}

// ---- the lookups of one half of the list (kernels.h's pick_* for its ops)

template <int PART>
bool part_tuned(int dtype, int acc, int op) {
  return with_elem<PART>(dtype, acc, op, false, [](auto e) { return decltype(e)::tuned; });
}

template <int PART>
single_fn part_single(int dtype, int acc, int op, int engine, int block, int unroll, int pol) {
  return with_elem<PART>(dtype, acc, op, (single_fn) nullptr, [&](auto e) {
    typedef decltype(e) E;
    return pick_single_op<typename E::Op, E::tuned>(engine, block, unroll, pol);
  });
}

template <int PART>
plan_fn part_plan(int dtype, int acc, int op, int engine, int unroll, int pol) {
  return with_elem<PART>(dtype, acc, op, (plan_fn) nullptr, [&](auto e) {
    typedef decltype(e) E;
    return pick_plan_eng<typename E::Op, E::tuned>(engine, unroll, pol);
  });
}

template <int PART>
prog_fn part_prog(int dtype, int op, int unroll) {
  // programs accumulate natively only (hiccl_program_add_plan)
  return with_elem<PART>(dtype, HICCL_ACC_NATIVE, op, (prog_fn) nullptr, [&](auto e) -> prog_fn {
    typedef decltype(e) E;
    if constexpr (sizeof(typename E::Op::acc_t) > kPacket) return nullptr;  // the f32-accumulating ops
    else if (unroll != 2) return launch_prog_t<typename E::Op, 4>;
    else if constexpr (E::tuned) return launch_prog_t<typename E::Op, 2>;
    else return nullptr;
  });
}

}  // namespace
