// tests/cpp/f8_compute.cpp -- HiCCL::Compute<f8e4m3> and Compute<f8e5m2>: add /
// start / wait on one compute each, unscaled and with set_scale, in a single
// process.
//
//   f8_compute IN_E4M3 OUT_E4M3 IN_E5M2 OUT_E5M2 n count alpha
//
// IN_* holds n x count FP8 bytes (row k = input k).  Each compute is started
// twice: as a plain sum (output OUT_*.plain) and, after set_scale(alpha) on
// the launched compute, scaled (OUT_*).  Built twice from this file: with
// HICCL_PORT_HOST the computes run the host port (the types' own `+=`, then
// scale_finish), without it the batched plan kernel on the GPU.  Input k
// starts (k + 2) mod 16 bytes and the output 1 byte past a 16-byte boundary,
// so the GPU computes have a scalar head and tail and mutually misaligned
// inputs.  tests/test_f8_cpu.py and tests/test_f8_gpu.py compare the outputs
// with the torch restatement (tests/f8_expected.py).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hiccl/compute.h"

static void fail(const char *what) {
  std::fprintf(stderr, "f8_compute: %s\n", what);
  std::exit(1);
}

template <class T>
static void run(const char *in_path, const std::string &out_path, int n, size_t count, double alpha) {
  static_assert(sizeof(T) == 1, "an FP8 storage type");
  std::vector<char> host((size_t)n * count), result(count);
  FILE *fh = std::fopen(in_path, "rb");
  if (!fh || std::fread(host.data(), 1, (size_t)n * count, fh) != (size_t)n * count) fail("cannot read an input file");
  std::fclose(fh);

  const size_t slot = (count + 2 * 16 + 8 + 15) / 16 * 16;  // bytes per buffer, offsets included
  const size_t bytes = (size_t)(n + 1) * slot;
  char *base = nullptr;
#ifdef HICCL_PORT_HOST
  base = (char *)std::aligned_alloc(64, (bytes + 63) / 64 * 64);
  if (!base) fail("aligned_alloc");
  std::memset(base, 0xA5, bytes);
#else
  CommBench::hip_check(hipSetDevice(0), "hipSetDevice");
  CommBench::hip_check(hipMalloc((void **)&base, bytes), "hipMalloc");
  CommBench::hip_check(hipMemset(base, 0xA5, bytes), "hipMemset");
#endif
  std::vector<T *> in(n);
  for (int k = 0; k < n; k++) {
    in[k] = (T *)(base + (size_t)k * slot + (k + 2) % 16);
#ifdef HICCL_PORT_HOST
    std::memcpy((void *)in[k], host.data() + (size_t)k * count, count);
#else
    CommBench::hip_check(hipMemcpy(in[k], host.data() + (size_t)k * count, count, hipMemcpyHostToDevice), "H2D");
#endif
  }
  T *out = (T *)(base + (size_t)n * slot + 1);

  auto save = [&](const std::string &path) {
#ifdef HICCL_PORT_HOST
    std::memcpy(result.data(), out, count);
#else
    CommBench::hip_check(hipMemcpy(result.data(), out, count, hipMemcpyDeviceToHost), "D2H");
#endif
    FILE *o = std::fopen(path.c_str(), "wb");
    if (!o || std::fwrite(result.data(), 1, count, o) != count || std::fclose(o)) fail("cannot write an output file");
  };
  {
    HiCCL::Compute<T> comp;
    comp.add(in, out, count, /*compid=*/0);
    if (comp.numcomp != 1) fail("the compute was not recorded");
    comp.start();
    comp.wait();
    save(out_path + ".plain");
    comp.set_scale(alpha);  // on the launched compute
    comp.start();
    comp.wait();
    save(out_path);
  }
#ifdef HICCL_PORT_HOST
  std::free(base);
#else
  CommBench::hip_check(hipFree(base), "hipFree");
#endif
}

int main(int argc, char **argv) {
  if (argc != 8) fail("usage: f8_compute IN_E4M3 OUT_E4M3 IN_E5M2 OUT_E5M2 n count alpha");
  const int n = std::atoi(argv[5]);
  const size_t count = (size_t)std::atoll(argv[6]);
  const double alpha = std::strtod(argv[7], nullptr);  // a hex float keeps every bit
  if (n < 1 || n > 64 || count < 1 || count > (1u << 24)) fail("n or count out of range");
  run<HiCCL::f8e4m3>(argv[1], argv[2], n, count, alpha);
  run<HiCCL::f8e5m2>(argv[3], argv[4], n, count, alpha);
  std::printf("f8_compute: PASSED (%d x %zu, f8e4m3 and f8e5m2, plain and scaled by %a)\n", n, count, alpha);
  return 0;
}
