// tests/cpp/prod_compute.cpp -- HiCCL::Compute<prodof<float>> and
// Compute<prodof<HiCCL::bf16>>: add / start / wait on one compute each, in a
// single process.
//
//   prod_compute IN_F32 OUT_F32 IN_BF16 OUT_BF16 n count
//
// IN_F32 holds n x count floats and IN_BF16 n x count bf16 bit patterns (row
// k = input k); the product of the floats goes to OUT_F32 and the product of
// the bf16 values to OUT_BF16.  Built twice from this file: with
// HICCL_PORT_HOST the computes run the host port (host_sum, `acc += x` on the
// wrapper types), without it the batched plan kernel on the GPU (HICCL_FLOAT32
// and HICCL_BFLOAT16 under HICCL_OP_PROD).  Input k starts k + 2 elements and
// the output 1 element past a 16-byte boundary, so the GPU computes have a
// scalar head and tail and mutually misaligned inputs.  tests/test_prod_cpu.py
// and tests/test_prod_gpu.py compare the outputs with the fixtures.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hiccl/compute.h"

static void fail(const char *what) {
  std::fprintf(stderr, "prod_compute: %s\n", what);
  std::exit(1);
}

template <class T>
static void run(const char *in_path, const char *out_path, int n, size_t count) {
  static_assert(sizeof(T) == sizeof(typename T::value_type), "a wrapper is its value");
  static_assert(HiCCL::op_of<T>() == 16, "prodof<U> runs under HICCL_OP_PROD");
  const size_t esz = sizeof(T), per = 16 / esz;
  std::vector<char> host((size_t)n * count * esz), result(count * esz);
  FILE *fh = std::fopen(in_path, "rb");
  if (!fh || std::fread(host.data(), esz, (size_t)n * count, fh) != (size_t)n * count) fail("cannot read an input file");
  std::fclose(fh);

  const size_t slot = count + 2 * per + 8;  // elements per buffer, offsets included
  const size_t bytes = (size_t)(n + 1) * slot * esz;
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
  auto aligned = [&](size_t k) {  // the 16-byte boundary at or after slot k's start
    const size_t off = (k * slot * esz + 15) / 16 * 16;
    return (T *)(base + off);
  };
  std::vector<T *> in(n);
  for (int k = 0; k < n; k++) {
    in[k] = aligned(k) + (k + 2) % per;
#ifdef HICCL_PORT_HOST
    std::memcpy((void *)in[k], host.data() + (size_t)k * count * esz, count * esz);
#else
    CommBench::hip_check(hipMemcpy(in[k], host.data() + (size_t)k * count * esz, count * esz, hipMemcpyHostToDevice),
                         "H2D");
#endif
  }
  T *out = aligned(n) + 1;

  {
    HiCCL::Compute<T> comp;
    comp.add(in, out, count, /*compid=*/0);
    if (comp.numcomp != 1) fail("the compute was not recorded");
    comp.start();
    comp.wait();
  }

#ifdef HICCL_PORT_HOST
  std::memcpy(result.data(), out, count * esz);
  std::free(base);
#else
  CommBench::hip_check(hipMemcpy(result.data(), out, count * esz, hipMemcpyDeviceToHost), "D2H");
  CommBench::hip_check(hipFree(base), "hipFree");
#endif
  fh = std::fopen(out_path, "wb");
  if (!fh || std::fwrite(result.data(), esz, count, fh) != count || std::fclose(fh)) fail("cannot write an output file");
}

int main(int argc, char **argv) {
  if (argc != 7) fail("usage: prod_compute IN_F32 OUT_F32 IN_BF16 OUT_BF16 n count");
  const int n = std::atoi(argv[5]);
  const size_t count = (size_t)std::atoll(argv[6]);
  if (n < 1 || n > 64 || count < 1 || count > (1u << 24)) fail("n or count out of range");
  run<HiCCL::prodof<float>>(argv[1], argv[2], n, count);
  run<HiCCL::prodof<HiCCL::bf16>>(argv[3], argv[4], n, count);
  std::printf("prod_compute: PASSED (%d x %zu, product of float and of bf16)\n", n, count);
  return 0;
}
