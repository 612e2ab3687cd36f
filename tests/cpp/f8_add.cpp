// tests/cpp/f8_add.cpp -- HiCCL::f8e4m3 and HiCCL::f8e5m2
// (include/hiccl/elem_types.h, include/hiccl/ops.h) on the host: a stand-alone
// program that writes what the types compute, for tests/test_f8_cpu.py to
// compare with torch's conversions bit for bit.
//
//   f8_add <outdir>
//
// For F in {e4m3, e5m2} it writes into <outdir>:
//   add_F.bin     65,536 bytes: `acc = a; acc += b` for a = i >> 8, b = i & 255
//   round_F.bin   2,097,152 bytes: F::round of the f32 patterns i << 12
//                 (i < 2^20), then of (i << 12) | 1
//   widen_F.bin   256 floats: `operator float` of every byte
//   ident_F.bin   5 bytes: maxof<F>(0), minof<F>(0), F(0), and maxof / minof
//                 folded over {-0, +0}
// The test builds it plainly and with -fsanitize=address,undefined and runs both.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "hiccl/ops.h"

using namespace HiCCL;

static bool dump(const std::string &path, const void *p, size_t n) {
  FILE *f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = std::fwrite(p, 1, n, f) == n;
  return std::fclose(f) == 0 && ok;
}

template <class F>
static bool tables(const std::string &dir, const char *name) {
  std::vector<uint8_t> add(65536);
  for (uint32_t i = 0; i < 65536; i++) {
    F acc, b;
    acc.bits = (uint8_t)(i >> 8);
    b.bits = (uint8_t)(i & 255);
    acc += b;
    add[i] = acc.bits;
  }
  const uint32_t n = 1u << 20;
  std::vector<uint8_t> rnd(2 * (size_t)n);
  for (uint32_t low = 0; low < 2; low++) {
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t w = (i << 12) | low;
      float f;
      std::memcpy(&f, &w, 4);
      rnd[(size_t)low * n + i] = F::round(f);
    }
  }
  float wid[256];
  for (int b = 0; b < 256; b++) {
    F x;
    x.bits = (uint8_t)b;
    wid[b] = (float)x;
  }
  maxof<F> mx = 0;
  minof<F> mn = 0;
  F zero = 0;
  // -0 < +0: a maximum over {-0, +0} is +0 (0x00), a minimum -0 (0x80)
  maxof<F> fm = 0, a, b;
  minof<F> fn = 0, c, d;
  a.v.bits = c.v.bits = 0x80;
  b.v.bits = d.v.bits = 0x00;
  fm += a, fm += b, fm += a;
  fn += d, fn += c, fn += d;
  const uint8_t ident[5] = {mx.v.bits, mn.v.bits, zero.bits, fm.v.bits, fn.v.bits};
  const std::string s(name);
  return dump(dir + "/add_" + s + ".bin", add.data(), add.size()) &&
         dump(dir + "/round_" + s + ".bin", rnd.data(), rnd.size()) &&
         dump(dir + "/widen_" + s + ".bin", wid, sizeof(wid)) && dump(dir + "/ident_" + s + ".bin", ident, 5);
}

int main(int argc, char **argv) {
  static_assert(sizeof(f8e4m3) == 1 && sizeof(f8e5m2) == 1 && sizeof(maxof<f8e4m3>) == 1 && sizeof(minof<f8e5m2>) == 1,
                "a wrapper is its value");
  static_assert(op_of<maxof<f8e4m3>>() == 1 && op_of<minof<f8e5m2>>() == 2 && op_of<f8e4m3>() == 0, "op_of");
  if (argc != 2) {
    std::printf("usage: f8_add <outdir>\n");
    return 2;
  }
  const bool ok = tables<f8e4m3>(argv[1], "e4m3") && tables<f8e5m2>(argv[1], "e5m2");
  std::printf("f8_add: %s\n", ok ? "WROTE" : "FAILED");
  return ok ? 0 : 1;
}
