// hiccl_amd/csrc/runtime.cpp -- errors, device facts, ticket counters,
// buffer checks (runtime.h).
#include "runtime.h"

#include <cstdlib>
#include <map>
#include <mutex>

namespace hiccl_impl {

// ------------------------------------------------------------------ errors --

static thread_local std::string g_last_error;

int fail(int code, const std::string &msg) {
  g_last_error = msg;
  return code;
}

int check_hip(hipError_t e, const char *what) {
  if (e != hipSuccess) {
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    return (int)e;
  }
  return 0;
}

const char *last_error() { return g_last_error.c_str(); }

// -------------------------------------------------------- device and stream --

// Token protocol of programs and of k_sigwait_phases (hiccl_token_mode).
// Default FENCED: release token stores, relaxed polls then an acquire
// fence per phase, a release gate store and an agent-scope acquire after
// each workgroup's gate polls -- the memory model's own guarantee.
// HICCL_PROG_FENCES=light: relaxed stores and polls, no fences (prog_phases'
// argument rests on kernel-boundary cache behaviour that only a run with one
// GPU per rank can confirm, so it is opt-in until one has).  Read at every
// launch (a capture keeps the value it was recorded with).
bool prog_light() {
  const char *e = std::getenv("HICCL_PROG_FENCES");
  return e && std::string(e) == "light";
}

static std::mutex g_dev_mu;
static int g_dev_cus[64];

static thread_local int t_cus_override = 0;

CusOverride::CusOverride(int cus) { t_cus_override = cus; }
CusOverride::~CusOverride() { t_cus_override = 0; }

int device_cus(int dev) {
  if (t_cus_override > 0) return t_cus_override;
  if (dev < 0 || dev >= 64) return 256;
  std::lock_guard<std::mutex> lk(g_dev_mu);
  if (g_dev_cus[dev] == 0) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus <= 0)
      cus = 256;
    g_dev_cus[dev] = cus;
  }
  return g_dev_cus[dev];
}

int current_device() {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess) d = 0;
  return d;
}

bool capturing(hipStream_t s, bool if_unknown) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cap) != hipSuccess) {
    (void)hipGetLastError();
    return if_unknown;
  }
  return cap != hipStreamCaptureStatusNone;
}

// Dynamic-scheduling counter pairs, one per (device, stream), allocated on
// first use (64 B apart) and zeroed once; the kernels leave them zero.
namespace {
struct SchedKey {
  int dev;
  hipStream_t s;
  bool operator<(const SchedKey &o) const { return dev != o.dev ? dev < o.dev : s < o.s; }
};
std::mutex g_sched_mu;
std::map<SchedKey, uint32_t *> g_sched;
}  // namespace

// Never during stream capture (a replayed graph could run beside other work
// on the same stream's counter).  hipStreamPerThread is one handle value for
// a different stream on every host thread: two threads could run kernels on
// one counter at once (units skipped, wrong sums), so it takes the static
// schedule.  The null stream is the legacy stream here (this library is
// built without per-thread default streams): launches on it serialise, one
// counter is safe.
uint32_t *ticket_counter(int dev, hipStream_t s) {
  if (s == hipStreamPerThread || capturing(s, true)) return nullptr;
  std::lock_guard<std::mutex> lk(g_sched_mu);
  auto it = g_sched.find(SchedKey{dev, s});
  if (it != g_sched.end()) return it->second;
  uint32_t *p = nullptr;
  if (hipMalloc((void **)&p, 64) != hipSuccess) return nullptr;
  // zeroed in order on `s` (a null-stream memset does not order a
  // non-blocking stream's first kernel after it)
  if (hipMemsetAsync(p, 0, 64, s) != hipSuccess) {
    (void)hipFree(p);
    return nullptr;
  }
  g_sched.emplace(SchedKey{dev, s}, p);
  return p;
}

// ----------------------------------------------------------------- buffers --

Split split_on(const void *out, size_t count, size_t esz) {
  const size_t V = kPacket / esz;
  const uintptr_t mis = (uintptr_t)out % kPacket;
  size_t head = mis ? (kPacket - mis) / esz : 0;
  if (head > count) head = count;
  Split s;
  s.head = (uint32_t)head;
  s.npkt = (count - head) / V;
  s.tail = (uint32_t)(count - head - s.npkt * V);
  return s;
}

int check_buffers(void *out, const void *const *in, int n, size_t count, size_t esz) {
  if (!out) return fail(hipErrorInvalidValue, "hiccl_reduce: out is NULL");
  if ((uintptr_t)out % esz)
    return fail(hipErrorInvalidValue, "hiccl_reduce: out is not element-aligned");
  if (n < 0) return fail(hipErrorInvalidValue, "hiccl_reduce: n < 0");
  if (n > 0 && !in) return fail(hipErrorInvalidValue, "hiccl_reduce: in is NULL");
  const uintptr_t o0 = (uintptr_t)out, o1 = o0 + count * esz;
  for (int k = 0; k < n; k++) {
    const uintptr_t p = (uintptr_t)in[k];
    if (!p) return fail(hipErrorInvalidValue, "hiccl_reduce: in[" + std::to_string(k) + "] is NULL");
    if (p % esz)
      return fail(hipErrorInvalidValue,
                  "hiccl_reduce: in[" + std::to_string(k) + "] is not element-aligned");
    const uintptr_t p1 = p + count * esz;
    if (p != o0 && p < o1 && o0 < p1)
      return fail(hipErrorInvalidValue, "hiccl_reduce: in[" + std::to_string(k) +
                                            "] partially overlaps out (only exact aliasing is allowed)");
  }
  return 0;
}

int check_buffers_widened(void *out, const void *const *in, int n, size_t count, size_t esz, size_t osz) {
  if (!out) return fail(hipErrorInvalidValue, "hiccl_reduce_widened: out is NULL");
  if ((uintptr_t)out % osz)
    return fail(hipErrorInvalidValue, "hiccl_reduce_widened: out is not aligned to its element (4 bytes)");
  if (n < 0) return fail(hipErrorInvalidValue, "hiccl_reduce_widened: n < 0");
  if (n > 0 && !in) return fail(hipErrorInvalidValue, "hiccl_reduce_widened: in is NULL");
  if (count > SIZE_MAX / osz)
    return fail(hipErrorInvalidValue, "hiccl_reduce_widened: count overflows (4 * count does not fit a size_t)");
  const uintptr_t o0 = (uintptr_t)out, o1 = o0 + count * osz;
  for (int k = 0; k < n; k++) {
    const uintptr_t p = (uintptr_t)in[k];
    if (!p) return fail(hipErrorInvalidValue, "hiccl_reduce_widened: in[" + std::to_string(k) + "] is NULL");
    if (p % esz)
      return fail(hipErrorInvalidValue, "hiccl_reduce_widened: in[" + std::to_string(k) + "] is not element-aligned");
    const uintptr_t p1 = p + count * esz;
    if (p < o1 && o0 < p1)
      return fail(hipErrorInvalidValue, "hiccl_reduce_widened: in[" + std::to_string(k) +
                                            "] overlaps out (a widened sum cannot run in place: the element sizes differ)");
  }
  return 0;
}

}  // namespace hiccl_impl
