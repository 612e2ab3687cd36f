// tests/cpp/ops_add.cpp -- `+=` of HiCCL::maxof<U> / minof<U> (host only).
//
//   ops_add table OUT
//       For U = f16 and U = bf16, op = max and min, each of the type's 16 fixed
//       addends a (tests/hostile_f16.py ADDENDS; tests/ops_expected.py
//       BF16_ADDENDS: +-0, the smallest subnormal and normal of either sign,
//       +-1, 1 + ulp, -2048, +-max, 16, +-Inf, one NaN) and each of the 65,536
//       patterns x:  T acc = x; acc += a;  the bits go to OUT as
//       uint16[2 types][2 ops][16][65536].  Where the compiler has _Float16,
//       maxof<_Float16> is checked against maxof<f16> on the same pairs.
//   ops_add fold KIND OP IN OUT n count
//       KIND f32 | f64 | i32 | u64, OP max | min: IN holds n x count elements
//       (row k = input k);  T acc = 0; acc += in[k][i]  in list order goes to
//       OUT -- the reference's reduce_kernel loop on the wrapper type.
//
// tests/test_ops_cpu.py compares both with tests/ops_expected.py.  The static
// checks below are the wrappers' contract (include/hiccl/ops.h).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hiccl/compute.h"  // built with -DHICCL_PORT_HOST: no HIP

using HiCCL::bf16;
using HiCCL::f16;
using HiCCL::maxof;
using HiCCL::minof;

static_assert(sizeof(maxof<float>) == 4 && sizeof(minof<double>) == 8, "wrapper size");
static_assert(sizeof(maxof<bf16>) == 2 && sizeof(minof<f16>) == 2, "wrapper size");
static_assert(sizeof(maxof<int32_t>) == 4 && sizeof(minof<uint64_t>) == 8, "wrapper size");
static_assert(HiCCL::dtype_of<maxof<float>>() == 0 && HiCCL::dtype_of<minof<double>>() == 1, "dtype of a wrapper");
static_assert(HiCCL::dtype_of<maxof<bf16>>() == 2 && HiCCL::dtype_of<minof<f16>>() == 6, "dtype of a wrapper");
static_assert(HiCCL::dtype_of<maxof<int32_t>>() == 4 && HiCCL::dtype_of<minof<uint64_t>>() == 3, "dtype of a wrapper");
static_assert(HiCCL::dtype_of<minof<unsigned long>>() == 3 && HiCCL::dtype_of<maxof<int>>() == 4, "dtype of a wrapper");
static_assert(HiCCL::op_of<float>() == 0 && HiCCL::op_of<bf16>() == 0, "plain types sum");
static_assert(HiCCL::op_of<maxof<float>>() == 1 && HiCCL::op_of<minof<f16>>() == 2, "op of a wrapper");
#ifdef __FLT16_MANT_DIG__
static_assert(sizeof(maxof<_Float16>) == 2 && HiCCL::dtype_of<minof<_Float16>>() == 6, "_Float16 wrapper");
#endif

static const uint16_t kF16Addends[16] = {0x0000, 0x8000, 0x0001, 0x8001, 0x0400, 0x8400, 0x3C00, 0xBC00,
                                         0x3C01, 0xE800, 0x7BFF, 0xFBFF, 0x4C00, 0x7C00, 0xFC00, 0x7E01};
static const uint16_t kBF16Addends[16] = {0x0000, 0x8000, 0x0001, 0x8001, 0x0080, 0x8080, 0x3F80, 0xBF80,
                                          0x3F81, 0xC500, 0x7F7F, 0xFF7F, 0x4180, 0x7F80, 0xFF80, 0x7FC1};

static void fail(const std::string &what) {
  std::fprintf(stderr, "ops_add: %s\n", what.c_str());
  std::exit(1);
}

template <class W, class U>
static void table_of(const uint16_t *addends, uint16_t *out) {
  for (int a = 0; a < 16; a++) {
    U add;
    add.bits = addends[a];
    for (uint32_t b = 0; b < 65536; b++) {
      U x;
      x.bits = (uint16_t)b;
      W acc, other;
      acc.v = x;
      other.v = add;
      acc += other;
      out[(size_t)a * 65536 + b] = acc.v.bits;
    }
  }
}

#ifdef __FLT16_MANT_DIG__
static bool f16_nan(uint16_t b) { return (b & 0x7C00) == 0x7C00 && (b & 0x03FF); }

template <class W>
static void check_float16(const uint16_t *expect) {
  for (int a = 0; a < 16; a++) {
    _Float16 add;
    std::memcpy(&add, &kF16Addends[a], 2);
    for (uint32_t b = 0; b < 65536; b++) {
      const uint16_t bits = (uint16_t)b;
      _Float16 x;
      std::memcpy(&x, &bits, 2);
      W acc, other;
      acc.v = x;
      other.v = add;
      acc += other;
      const _Float16 r = acc.v;
      uint16_t got;
      std::memcpy(&got, &r, 2);
      const uint16_t want = expect[(size_t)a * 65536 + b];
      if (f16_nan(want) ? !f16_nan(got) : got != want)
        fail("_Float16 wrapper differs from the f16 wrapper at addend " + std::to_string(a) + ", pattern " +
             std::to_string(b));
    }
  }
}
#endif

template <class W>
static void check_identity(uint64_t want_bits, const char *name) {
  W acc = 0;  // T acc = 0
  uint64_t got = 0;
  std::memcpy(&got, &acc, sizeof(W));
  if (got != want_bits) fail(std::string("identity of ") + name);
  W one = 0, other = 0;
  if (!(one == other) || one != other) fail(std::string("== / != of ") + name);
}

template <class W, class U>
static void fold_file(const char *in_path, const char *out_path, int n, size_t count) {
  std::vector<U> in((size_t)n * count), out(count);
  FILE *fh = std::fopen(in_path, "rb");
  if (!fh || std::fread(in.data(), sizeof(U), in.size(), fh) != in.size()) fail("cannot read IN");
  std::fclose(fh);
  std::vector<W *> rows(n);
  for (int k = 0; k < n; k++) rows[k] = reinterpret_cast<W *>(in.data() + (size_t)k * count);
  for (size_t i = 0; i < count; i++) {  // the reference's loop (reduce_kernel, CPU branch)
    W acc = 0;
    for (int k = 0; k < n; k++) acc += rows[k][i];
    out[i] = acc.v;
  }
  fh = std::fopen(out_path, "wb");
  if (!fh || std::fwrite(out.data(), sizeof(U), count, fh) != count || std::fclose(fh)) fail("cannot write OUT");
  std::printf("ops_add: folded %d x %zu\n", n, count);
}

int main(int argc, char **argv) {
  check_identity<maxof<float>>(0xff800000u, "maxof<float>");
  check_identity<minof<float>>(0x7f800000u, "minof<float>");
  check_identity<maxof<double>>(0xfff0000000000000ull, "maxof<double>");
  check_identity<minof<double>>(0x7ff0000000000000ull, "minof<double>");
  check_identity<maxof<bf16>>(0xff80u, "maxof<bf16>");
  check_identity<minof<bf16>>(0x7f80u, "minof<bf16>");
  check_identity<maxof<f16>>(0xfc00u, "maxof<f16>");
  check_identity<minof<f16>>(0x7c00u, "minof<f16>");
  check_identity<maxof<int32_t>>(0x80000000u, "maxof<int32_t>");
  check_identity<minof<int32_t>>(0x7fffffffu, "minof<int32_t>");
  check_identity<maxof<uint64_t>>(0, "maxof<uint64_t>");
  check_identity<minof<uint64_t>>(~0ull, "minof<uint64_t>");
  if (argc == 3 && std::string(argv[1]) == "table") {
    const size_t block = 16u * 65536u;
    std::vector<uint16_t> out(4 * block);
    table_of<maxof<f16>, f16>(kF16Addends, out.data());
    table_of<minof<f16>, f16>(kF16Addends, out.data() + block);
    table_of<maxof<bf16>, bf16>(kBF16Addends, out.data() + 2 * block);
    table_of<minof<bf16>, bf16>(kBF16Addends, out.data() + 3 * block);
#ifdef __FLT16_MANT_DIG__
    check_float16<maxof<_Float16>>(out.data());
    check_float16<minof<_Float16>>(out.data() + block);
#endif
    FILE *fh = std::fopen(argv[2], "wb");
    if (!fh || std::fwrite(out.data(), 2, out.size(), fh) != out.size() || std::fclose(fh)) fail("cannot write OUT");
    std::printf("ops_add: wrote %zu results\n", out.size());
    return 0;
  }
  if (argc == 8 && std::string(argv[1]) == "fold") {
    const std::string kind = argv[2], op = argv[3];
    const int n = std::atoi(argv[6]);
    const size_t count = (size_t)std::atoll(argv[7]);
    if (n < 0 || n > 64 || count < 1 || count > (1u << 24)) fail("n or count out of range");
    const bool mx = op == "max";
    if (!mx && op != "min") fail("OP must be max or min");
    if (kind == "f32") mx ? fold_file<maxof<float>, float>(argv[4], argv[5], n, count)
                          : fold_file<minof<float>, float>(argv[4], argv[5], n, count);
    else if (kind == "f64") mx ? fold_file<maxof<double>, double>(argv[4], argv[5], n, count)
                               : fold_file<minof<double>, double>(argv[4], argv[5], n, count);
    else if (kind == "i32") mx ? fold_file<maxof<int32_t>, int32_t>(argv[4], argv[5], n, count)
                               : fold_file<minof<int32_t>, int32_t>(argv[4], argv[5], n, count);
    else if (kind == "u64") mx ? fold_file<maxof<uint64_t>, uint64_t>(argv[4], argv[5], n, count)
                               : fold_file<minof<uint64_t>, uint64_t>(argv[4], argv[5], n, count);
    else fail("KIND must be f32, f64, i32 or u64");
    return 0;
  }
  fail("usage: ops_add table OUT | ops_add fold KIND OP IN OUT n count");
  return 2;
}
