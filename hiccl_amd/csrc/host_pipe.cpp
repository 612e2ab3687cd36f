// hiccl_amd/csrc/host_pipe.cpp -- hiccl_host_pipe_*: host-resident buckets
// reduced on the GPU through a pipeline of staged chunks.
#include <vector>

#include "policy.h"

using namespace hiccl_impl;

struct hiccl_host_pipe {
  int dtype = 0;
  int device = 0;
  int op = HICCL_OP_SUM;  // hiccl_host_pipe_set_op
  bool scaled = false;    // hiccl_host_pipe_set_scale: out = alpha * sum (op stays SUM)
  Scale scale{0.0, 0.0f, 0u};
  size_t esz = 0;
  size_t chunk = 0;  // elements per input per chunk
  int depth = 0;
  int cap_n = 0;     // staging slots hold this many inputs
  std::vector<hipStream_t> streams;
  std::vector<char *> stage;  // per slot: max(cap_n, 1) x chunk elements
};

namespace {

constexpr size_t kPipeChunkBytes = 64ull << 20;
constexpr int kPipeDepth = 3;

int pipe_stage_for(hiccl_host_pipe *p, int n) {
  const int need = n > 0 ? n : 1;
  if (need <= p->cap_n) return 0;
  for (auto &b : p->stage)
    if (b) { (void)hipFree(b); b = nullptr; }
  p->cap_n = 0;
  for (auto &b : p->stage)
    if (int e = check_hip(hipMalloc((void **)&b, (size_t)need * p->chunk * p->esz), "host_pipe: hipMalloc staging"))
      return e;
  p->cap_n = need;
  return 0;
}

}  // namespace

extern "C" {

int hiccl_host_pipe_create(hiccl_host_pipe_t **pipe, int dtype, int device, size_t chunk_bytes,
                           int depth) {
  if (!pipe) return fail(hipErrorInvalidValue, "host_pipe_create: pipe is NULL");
  *pipe = nullptr;
  const size_t esz = esize(dtype);
  if (!esz) return fail(hipErrorInvalidValue, "host_pipe_create: unknown dtype");
  if (depth < 0 || depth > 8) return fail(hipErrorInvalidValue, "host_pipe_create: depth must be 0..8");
  if (!chunk_bytes) chunk_bytes = kPipeChunkBytes;
  if (chunk_bytes < esz) return fail(hipErrorInvalidValue, "host_pipe_create: chunk_bytes below one element");
  int ndev = 0;
  if (int e = check_hip(hipGetDeviceCount(&ndev), "host_pipe_create: hipGetDeviceCount")) return e;
  if (device < 0 || device >= ndev) return fail(hipErrorInvalidDevice, "host_pipe_create: bad device");
  if (int e = check_hip(hipSetDevice(device), "host_pipe_create: hipSetDevice")) return e;
  auto *p = new hiccl_host_pipe;
  p->dtype = dtype;
  p->device = device;
  p->esz = esz;
  p->chunk = chunk_bytes / esz;
  p->depth = depth ? depth : kPipeDepth;
  p->stage.assign(p->depth, nullptr);
  for (int i = 0; i < p->depth; i++) {
    hipStream_t s = nullptr;
    if (int e = check_hip(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "host_pipe_create: stream")) {
      hiccl_host_pipe_destroy(p);
      return e;
    }
    p->streams.push_back(s);
  }
  *pipe = p;
  return 0;
}

int hiccl_host_pipe_reduce(hiccl_host_pipe_t *p, void *out, const void *const *in, int n, size_t count) {
  if (!p) return fail(hipErrorInvalidValue, "host_pipe_reduce: pipe is NULL");
  if (p->dtype == HICCL_BYTES && n != 1) return fail(hipErrorInvalidValue, "host_pipe_reduce: HICCL_BYTES copies need n == 1");
  if (int e = check_buffers(out, in, n, count, p->esz)) return e;
  if (count == 0) return 0;
  if (int e = check_hip(hipSetDevice(p->device), "host_pipe_reduce: hipSetDevice")) return e;
  if (int e = pipe_stage_for(p, n)) return e;
  const size_t slot_in = p->chunk * p->esz;  // bytes between staged inputs
  std::vector<const void *> dev_in((size_t)(n > 0 ? n : 1));
  int err = 0;
  size_t c = 0;
  for (size_t lo = 0; lo < count && !err; lo += p->chunk, c++) {
    const size_t len = count - lo < p->chunk ? count - lo : p->chunk;
    const int slot = (int)(c % (size_t)p->depth);
    hipStream_t s = p->streams[slot];
    char *stage = p->stage[slot];
    for (int k = 0; k < n && !err; k++) {
      dev_in[k] = stage + (size_t)k * slot_in;
      err = check_hip(hipMemcpyAsync(stage + (size_t)k * slot_in, (const char *)in[k] + lo * p->esz,
                                     len * p->esz, hipMemcpyHostToDevice, s),
                      "host_pipe_reduce: H2D");
    }
    // in place into staged input 0 (exact aliasing is element-wise safe)
    if (!err)
      err = reduce_call(p->dtype, p->scaled ? kOpScaledSum : p->op, p->scaled ? &p->scale : nullptr, stage,
                        dev_in.data(), n, len, s, nullptr);
    if (!err)
      err = check_hip(hipMemcpyAsync((char *)out + lo * p->esz, stage, len * p->esz, hipMemcpyDeviceToHost, s),
                      "host_pipe_reduce: D2H");
  }
  for (hipStream_t s : p->streams) {  // drain every slot, even after an error
    int e = check_hip(hipStreamSynchronize(s), "host_pipe_reduce: sync");
    if (!err) err = e;
  }
  return err;
}

int hiccl_host_pipe_set_op(hiccl_host_pipe_t *p, int op) {
  if (!p) return fail(hipErrorInvalidValue, "host_pipe_set_op: pipe is NULL");
  if (int e = check_op(p->dtype, HICCL_ACC_NATIVE, op, "host_pipe_set_op")) return e;
  if (p->scaled && op != HICCL_OP_SUM)
    return fail(hipErrorInvalidValue, "host_pipe_set_op: a scaled pipe sums (HICCL_OP_SUM only): clear the scale first");
  p->op = op;
  return 0;
}

int hiccl_host_pipe_set_scale(hiccl_host_pipe_t *p, const double *alpha) {
  if (!p) return fail(hipErrorInvalidValue, "host_pipe_set_scale: pipe is NULL");
  Scale sc{0.0, 0.0f, 0u};
  if (alpha) {
    if (int e = check_scale(p->dtype, *alpha, "host_pipe_set_scale", &sc)) return e;
    if (p->op != HICCL_OP_SUM)
      return fail(hipErrorInvalidValue, "host_pipe_set_scale: only sums are scaled (the pipe's op is not HICCL_OP_SUM)");
  }
  p->scaled = alpha != nullptr;
  p->scale = sc;
  return 0;
}

void hiccl_host_pipe_destroy(hiccl_host_pipe_t *p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  for (hipStream_t s : p->streams) (void)hipStreamSynchronize(s);
  for (char *b : p->stage)
    if (b) (void)hipFree(b);
  for (hipStream_t s : p->streams) (void)hipStreamDestroy(s);
  delete p;
}

}  // extern "C"
