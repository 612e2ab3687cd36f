// tests/cpp/weighted_sum.cpp -- HiCCL::WidenCompute<T> with per-input weights:
// add(in, out, n, compid, weights) / start / wait on one compute, in a single
// process.
//
//   weighted_sum KIND IN WEIGHTS PRIOR OUT n count alpha   KIND: bf16, f16, e4m3 or e5m2
//
// IN holds n x count elements of KIND (row k = input k), WEIGHTS n floats,
// PRIOR the count f32 words the output holds before the accumulating launch.
// Written:
//   OUT         fl32(s32 * a32), s32 the in-order sum of fl32(w[k] * widen(x[k]))
//   OUT.accum   fl32(p + fl32(s32 * a32))            a second, accumulating object
// Built twice from this file: with HICCL_PORT_HOST the compute runs the host
// port (the weights in host memory) -- a stand-alone program that
// tests/test_weighted_cpu.py also builds with -fsanitize=address,undefined;
// without it the batched plan kernel on the GPU, the weights in device memory
// (tests/test_weighted_gpu.py).  Input k starts (k + 1) mod 8 elements and the
// output 1 element past a 16-byte boundary, so the GPU compute has a scalar
// head and tail and mutually misaligned inputs.  The tests compare the outputs
// with the fixtures (tests/golden/reduce_weighted_*.npz).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hiccl/compute.h"

static void fail(const char *what) {
  std::fprintf(stderr, "weighted_sum: %s\n", what);
  std::exit(1);
}

static void read_file(const char *path, void *dst, size_t bytes) {
  FILE *fh = std::fopen(path, "rb");
  if (!fh || std::fread(dst, 1, bytes, fh) != bytes) fail("cannot read an input file");
  std::fclose(fh);
}

template <class T>
static void run(const char *in_path, const char *w_path, const char *prior_path, const std::string &out_path, int n,
                size_t count, double alpha) {
  const size_t in_bytes = count * sizeof(T), out_bytes = count * sizeof(float), w_bytes = (size_t)n * sizeof(float);
  std::vector<char> host((size_t)n * in_bytes);
  std::vector<float> prior(count), result(count), wts(n);
  read_file(in_path, host.data(), host.size());
  read_file(w_path, wts.data(), w_bytes);
  read_file(prior_path, prior.data(), out_bytes);

  const size_t in_slot = (in_bytes + 8 * sizeof(T) + 63) / 64 * 64, out_slot = (out_bytes + 16 + 63) / 64 * 64;
  const size_t w_slot = (w_bytes + 63) / 64 * 64;
  const size_t bytes = (size_t)n * in_slot + out_slot + w_slot;
  char *base = nullptr;
#ifdef HICCL_PORT_HOST
  base = (char *)std::aligned_alloc(64, bytes);
  if (!base) fail("aligned_alloc");
  std::memset(base, 0xA5, bytes);
#else
  CommBench::hip_check(hipSetDevice(0), "hipSetDevice");
  CommBench::hip_check(hipMalloc((void **)&base, bytes), "hipMalloc");
  CommBench::hip_check(hipMemset(base, 0xA5, bytes), "hipMemset");
#endif
  auto upload = [&](void *dst, const void *src, size_t nbytes) {
#ifdef HICCL_PORT_HOST
    std::memcpy(dst, src, nbytes);
#else
    CommBench::hip_check(hipMemcpy(dst, src, nbytes, hipMemcpyHostToDevice), "H2D");
#endif
  };
  std::vector<T *> in(n);
  for (int k = 0; k < n; k++) {
    in[k] = (T *)(base + (size_t)k * in_slot) + (k + 1) % 8;
    upload((void *)in[k], host.data() + (size_t)k * in_bytes, in_bytes);
  }
  float *out = (float *)(base + (size_t)n * in_slot) + 1;
  float *w = (float *)(base + (size_t)n * in_slot + out_slot);
  upload(w, wts.data(), w_bytes);

  auto save = [&](const std::string &path) {
#ifdef HICCL_PORT_HOST
    std::memcpy(result.data(), out, out_bytes);
#else
    CommBench::hip_check(hipMemcpy(result.data(), out, out_bytes, hipMemcpyDeviceToHost), "D2H");
#endif
    FILE *o = std::fopen(path.c_str(), "wb");
    if (!o || std::fwrite(result.data(), 1, out_bytes, o) != out_bytes || std::fclose(o)) fail("cannot write an output file");
  };
  {
    HiCCL::WidenCompute<T> comp;
    comp.set_scale(alpha);
    comp.add(in, out, count, /*compid=*/0, w);
    if (comp.numcomp != 1) fail("the compute was not recorded");
    if (comp.bytes() != count * ((size_t)n * sizeof(T) + 4)) fail("bytes() is not count * (n * sizeof(T) + 4)");
    comp.start();
    comp.wait();
    save(out_path);
  }
  {
    HiCCL::WidenCompute<T> comp;
    comp.set_accumulate();
    comp.set_scale(alpha);
    comp.add(in, out, count, /*compid=*/0, w);
    upload(out, prior.data(), out_bytes);
    comp.start();
    comp.wait();
    save(out_path + ".accum");
  }
#ifdef HICCL_PORT_HOST
  std::free(base);
#else
  CommBench::hip_check(hipFree(base), "hipFree");
#endif
}

int main(int argc, char **argv) {
  if (argc != 9) fail("usage: weighted_sum KIND IN WEIGHTS PRIOR OUT n count alpha");
  const std::string kind(argv[1]);
  const int n = std::atoi(argv[6]);
  const size_t count = (size_t)std::atoll(argv[7]);
  const double alpha = std::strtod(argv[8], nullptr);  // a hex float keeps every bit
  if (n < 1 || n > 64 || count < 1 || count > (1u << 24)) fail("n or count out of range");
  if (kind == "bf16") run<HiCCL::bf16>(argv[2], argv[3], argv[4], argv[5], n, count, alpha);
  else if (kind == "f16") run<HiCCL::f16>(argv[2], argv[3], argv[4], argv[5], n, count, alpha);
  else if (kind == "e4m3") run<HiCCL::f8e4m3>(argv[2], argv[3], argv[4], argv[5], n, count, alpha);
  else if (kind == "e5m2") run<HiCCL::f8e5m2>(argv[2], argv[3], argv[4], argv[5], n, count, alpha);
  else fail("KIND must be bf16, f16, e4m3 or e5m2");
  std::printf("weighted_sum: PASSED (%s, %d x %zu, scaled by %a, overwriting and accumulating)\n", kind.c_str(), n, count,
              alpha);
  return 0;
}
