// hiccl_amd/csrc/util.cpp -- the small entry points: version, errors, device
// facts, synthetic inputs, stream copies, bucket allocations.
#include "runtime.h"

// 0.10.0 (0.2: HICCL_FLOAT16; 0.3: hiccl_op_t, MAX and MIN; 0.4: PROD, BAND, BOR, BXOR; 0.5: scaled sums;
// 0.6: HICCL_FLOAT8_E4M3, HICCL_FLOAT8_E5M2; 0.7: widened sums;
// 0.8: accumulating widened sums; 0.9: unscaled computes in a scaled plan, the mixed plan kernels;
// 0.10: weighted widened sums)
#define HICCL_VERSION_INT 1000

using namespace hiccl_impl;

extern "C" {

size_t hiccl_dtype_size(int dtype) { return esize(dtype); }

const char *hiccl_last_error(void) { return last_error(); }

int hiccl_version(void) { return HICCL_VERSION_INT; }

// ---------------------------------------------------------- measurement --

int hiccl_fill_uniform(int dtype, void *out, size_t count, uint64_t seed, uint32_t k, size_t first,
                       void *stream) {
  if (count == 0) return 0;
  if (!out) return fail(hipErrorInvalidValue, "fill_uniform: out is NULL");
  // Same key derivation as oracle/reduce_oracle.c hash3(): splitmix64(seed ^ k<<48) + i.
  uint64_t z = seed ^ ((uint64_t)k << 48);
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  const uint64_t key = z ^ (z >> 31);
  uint64_t blocks = (count + 255) / 256;
  const uint64_t cap = (uint64_t)device_cus(current_device()) * 16;
  if (blocks > cap) blocks = cap;
  if (!launch_fill(dtype, (unsigned)blocks, (hipStream_t)stream, (char *)out, (uint64_t)count, key, (uint64_t)first))
    return fail(hipErrorInvalidValue, "fill_uniform: dtype must be FLOAT32/FLOAT64/BFLOAT16/FLOAT16/FLOAT8_E4M3/FLOAT8_E5M2");
  return check_hip(hipGetLastError(), "fill_uniform: launch");
}

int hiccl_device_info(int device, int *cus, int *mem_clock_khz, int *bus_width_bits) {
  int v = 0;
  if (cus) {
    if (int e = check_hip(hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device), "device_info: CUs"))
      return e;
    *cus = v;
  }
  if (mem_clock_khz) {
    if (int e = check_hip(hipDeviceGetAttribute(&v, hipDeviceAttributeMemoryClockRate, device), "device_info: clock"))
      return e;
    *mem_clock_khz = v;
  }
  if (bus_width_bits) {
    if (int e = check_hip(hipDeviceGetAttribute(&v, hipDeviceAttributeMemoryBusWidth, device), "device_info: bus"))
      return e;
    *bus_width_bits = v;
  }
  return 0;
}

int hiccl_stream_copy(void *dst, const void *src, size_t bytes, void *stream) {
  if (bytes == 0) return 0;
  if (!dst || !src) return fail(hipErrorInvalidValue, "stream_copy: NULL pointer");
  // the packet loop needs aligned pointers; fewer than 16 bytes are the byte tail alone, at any address (the
  // transport's probe of an IPC mapping reads 8 bytes or fewer where a buffer of 1- or 2-byte elements starts)
  if (bytes >= 16 && ((uintptr_t)dst % 16 || (uintptr_t)src % 16))
    return fail(hipErrorInvalidValue, "stream_copy: pointers must be 16-B aligned");
  hipStream_t s = (hipStream_t)stream;
  const uint64_t npkt = bytes / 16;
  if (npkt) {
    uint64_t blocks = (npkt + 1023) / 1024;
    const uint64_t cap = (uint64_t)device_cus(current_device()) * 8;
    if (blocks > cap) blocks = cap;
    launch_copy((unsigned)blocks, s, dst, src, npkt);
  }
  if (bytes % 16)
    launch_copy_bytes(s, (char *)dst + npkt * 16, (const char *)src + npkt * 16, (uint64_t)(bytes % 16));
  return check_hip(hipGetLastError(), "stream_copy: launch");
}

// ---- bucket layout
//
// A reduction bucket -- n inputs and the output of one compute -- in ONE
// device allocation, buffer j (inputs 0..n-1, then the output) at
// j x stride, stride = the buffer rounded up to 64 KiB plus 64 KiB.  Measured
// on config 2 (tools/alloc_probe.py; profiles/r06d_alloc.jsonl, r06e_, r06f_,
// r06h_): the same kernel on nine separate hipMalloc'd buffers (torch.empty,
// hipMalloc, hipDeviceMallocContiguous) runs 1.43-1.56 ms depending on the
// allocation -- up to 9 % apart in one process, although every buffer alone
// reads and writes at the same rate -- while buckets in one allocation at
// 1 GiB + 0-4 MiB strides ran 1.424-1.462 ms, every one of 28 instances on
// fresh devices (the 64-128 KiB staggers fastest).  Separate allocations
// leave the streams' relative physical placement to chance; one allocation
// fixes it.  Which physical memory the allocation gets still matters: on a
// device whose free memory was fragmented first, later buckets can be as
// slow as separate buffers (r06l_alloc.jsonl).
static uint64_t bucket_stride(size_t bytes) {
  const uint64_t g = 64ull << 10;
  return (((uint64_t)bytes + g - 1) / g) * g + g;
}

size_t hiccl_bucket_stride(int dtype, size_t count) {
  const size_t esz = esize(dtype);
  return esz && count ? (size_t)bucket_stride(count * esz) : 0;
}

int hiccl_bucket_alloc(int dtype, int n, size_t count, int device, void **base, void **in, void **out) {
  const size_t esz = esize(dtype);
  if (!esz) return fail(hipErrorInvalidValue, "bucket_alloc: unknown dtype");
  if (n < 0 || n > (1 << 20)) return fail(hipErrorInvalidValue, "bucket_alloc: n out of range");
  if (!count) return fail(hipErrorInvalidValue, "bucket_alloc: count must be > 0");
  if (!base || !out || (n > 0 && !in)) return fail(hipErrorInvalidValue, "bucket_alloc: NULL output argument");
  *base = nullptr;
  int prev = 0;
  if (int e = check_hip(hipGetDevice(&prev), "bucket_alloc: hipGetDevice")) return e;
  if (int e = check_hip(hipSetDevice(device), "bucket_alloc: hipSetDevice")) return e;
  const uint64_t stride = bucket_stride(count * esz);
  char *b = nullptr;
  const int e = check_hip(hipMalloc((void **)&b, (size_t)(stride * (uint64_t)(n + 1))), "bucket_alloc: hipMalloc");
  (void)hipSetDevice(prev);  // the caller's current device is left as it was
  if (e) return e;
  for (int k = 0; k < n; k++) in[k] = b + (uint64_t)k * stride;
  *out = b + (uint64_t)n * stride;
  *base = b;
  return 0;
}

int hiccl_bucket_free(void *base) {
  if (!base) return 0;
  return check_hip(hipFree(base), "bucket_free: hipFree");
}

}  // extern "C"
