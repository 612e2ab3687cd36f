// tests/cpp/f16_compute.cpp -- HiCCL::Compute<HiCCL::f16>: add / start / wait
// on one compute, in a single process.
//
//   f16_compute IN OUT n count
//
// IN holds n x count half bit patterns (uint16, row k = input k); the sum
// goes to OUT (count x uint16).  Built twice from this file: with
// HICCL_PORT_HOST the compute runs the host port (host_sum, `acc += x` on
// HiCCL::f16), without it the batched plan kernel on the GPU (HICCL_FLOAT16).
// Input k starts k + 2 elements and the output 1 element past a 16-byte
// boundary, so the GPU compute has a scalar head and tail and mutually
// misaligned inputs.  tests/test_f16_gpu.py compares both outputs with
// NumPy's in-order half sum.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hiccl/compute.h"

typedef HiCCL::f16 T;

static void fail(const char *what) {
  std::fprintf(stderr, "f16_compute: %s\n", what);
  std::exit(1);
}

int main(int argc, char **argv) {
  if (argc != 5) fail("usage: f16_compute IN OUT n count");
  const int n = std::atoi(argv[3]);
  const size_t count = (size_t)std::atoll(argv[4]);
  if (n < 1 || n > 64 || count < 1 || count > (1u << 24)) fail("n or count out of range");
  std::vector<uint16_t> host((size_t)n * count), result(count);
  FILE *fh = std::fopen(argv[1], "rb");
  if (!fh || std::fread(host.data(), 2, host.size(), fh) != host.size()) fail("cannot read IN");
  std::fclose(fh);

  const size_t slot = count + 16;  // elements per buffer, offsets included
  const size_t bytes = (size_t)(n + 1) * slot * sizeof(T);
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
    in[k] = (T *)base + (size_t)k * slot + (k + 2) % 8;
#ifdef HICCL_PORT_HOST
    std::memcpy((void *)in[k], host.data() + (size_t)k * count, count * 2);
#else
    CommBench::hip_check(hipMemcpy(in[k], host.data() + (size_t)k * count, count * 2, hipMemcpyHostToDevice), "H2D");
#endif
  }
  T *out = (T *)base + (size_t)n * slot + 1;

  {
    HiCCL::Compute<T> comp;
    comp.add(in, out, count, /*compid=*/0);
    if (comp.numcomp != 1) fail("the compute was not recorded");
    comp.start();
    comp.wait();
  }

#ifdef HICCL_PORT_HOST
  std::memcpy(result.data(), out, count * 2);
  std::free(base);
#else
  CommBench::hip_check(hipMemcpy(result.data(), out, count * 2, hipMemcpyDeviceToHost), "D2H");
  CommBench::hip_check(hipFree(base), "hipFree");
#endif
  fh = std::fopen(argv[2], "wb");
  if (!fh || std::fwrite(result.data(), 2, count, fh) != count || std::fclose(fh)) fail("cannot write OUT");
  std::printf("f16_compute: PASSED (%d x %zu)\n", n, count);
  return 0;
}
