// tests/cpp/scale_compute.cpp -- HiCCL::Compute<float> and Compute<HiCCL::bf16>
// with set_scale / clear_scale: add / start / wait on one compute each, in a
// single process.
//
//   scale_compute IN_F32 OUT_F32 IN_BF16 OUT_BF16 n count alpha
//
// IN_F32 holds n x count floats and IN_BF16 n x count bf16 bit patterns (row
// k = input k).  Each compute is started three times: scaled by `alpha` (set
// BEFORE the first add), scaled by 2 * alpha (set_scale on the launched
// compute) and after clear_scale.  The outputs go to OUT_*, OUT_*.twice and
// OUT_*.plain.  Built twice from this file: with HICCL_PORT_HOST the computes
// run the host port (host_sum, then scale_finish), without it the batched plan
// kernel on the GPU (hiccl_reduce_plan_set_scale).  Input k starts k + 2
// elements and the output 1 element past a 16-byte boundary, so the GPU
// computes have a scalar head and tail and mutually misaligned inputs.
// tests/test_scale_cpu.py and tests/test_scale_gpu.py compare the outputs with
// the fixtures.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hiccl/compute.h"

static void fail(const char *what) {
  std::fprintf(stderr, "scale_compute: %s\n", what);
  std::exit(1);
}

template <class T>
static void run(const char *in_path, const std::string &out_path, int n, size_t count, double alpha) {
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

  auto save = [&](const std::string &path) {
#ifdef HICCL_PORT_HOST
    std::memcpy(result.data(), out, count * esz);
#else
    CommBench::hip_check(hipMemcpy(result.data(), out, count * esz, hipMemcpyDeviceToHost), "D2H");
#endif
    FILE *o = std::fopen(path.c_str(), "wb");
    if (!o || std::fwrite(result.data(), esz, count, o) != count || std::fclose(o)) fail("cannot write an output file");
  };
  {
    HiCCL::Compute<T> comp;
    comp.set_scale(alpha);  // before the first add: kept until the plan exists
    comp.add(in, out, count, /*compid=*/0);
    if (comp.numcomp != 1) fail("the compute was not recorded");
    comp.start();
    comp.wait();
    save(out_path);
    comp.set_scale(2.0 * alpha);  // on the launched compute
    comp.start();
    comp.wait();
    save(out_path + ".twice");
    comp.clear_scale();
    comp.start();
    comp.wait();
    save(out_path + ".plain");
  }
#ifdef HICCL_PORT_HOST
  std::free(base);
#else
  CommBench::hip_check(hipFree(base), "hipFree");
#endif
}

int main(int argc, char **argv) {
  if (argc != 8) fail("usage: scale_compute IN_F32 OUT_F32 IN_BF16 OUT_BF16 n count alpha");
  const int n = std::atoi(argv[5]);
  const size_t count = (size_t)std::atoll(argv[6]);
  const double alpha = std::strtod(argv[7], nullptr);  // a hex float keeps every bit
  if (n < 1 || n > 64 || count < 1 || count > (1u << 24)) fail("n or count out of range");
  run<float>(argv[1], argv[2], n, count, alpha);
  run<HiCCL::bf16>(argv[3], argv[4], n, count, alpha);
  std::printf("scale_compute: PASSED (%d x %zu, float and bf16 scaled by %a)\n", n, count, alpha);
  return 0;
}
