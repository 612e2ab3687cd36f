// hiccl_amd/csrc/runtime.h -- what every host file of the library shares:
// the last-error string, device facts, the dynamic schedule's ticket
// counters, and the split of a buffer into head / packets / tail.
#pragma once

#include <string>

#include "../../include/hiccl_reduce.h"
#include "kernels.h"

namespace hiccl_impl __attribute__((visibility("hidden"))) {

// ---- errors: hiccl_last_error() returns the calling thread's last message
int fail(int code, const std::string &msg);
int check_hip(hipError_t e, const char *what);
const char *last_error();

// ---- device and stream
int current_device();
// Compute units of `dev` (256 where the runtime cannot tell).
int device_cus(int dev);
// While one lives, device_cus() answers `cus` on this thread instead of
// asking a device (hiccl_reduce_auto_choice).
struct CusOverride {
  explicit CusOverride(int cus);
  ~CusOverride();
};
// Is `s` being captured into a graph?  `if_unknown` is the answer when the
// runtime cannot tell.
bool capturing(hipStream_t s, bool if_unknown);
// The {ticket, done} counter pair of the dynamic schedule for a launch on
// (dev, s), or NULL -- the launch then runs the static schedule: during
// stream capture, on hipStreamPerThread, and on any allocation failure.
uint32_t *ticket_counter(int dev, hipStream_t s);
// HICCL_PROG_FENCES=light (hiccl_token_mode), read at every launch.
bool prog_light();

// ---- buffers
struct Split {
  uint32_t head, tail;
  uint64_t npkt;
};
// [head | npkt packets | tail] with the packets 16-B aligned on `out`.
Split split_on(const void *out, size_t count, size_t esz);
// Work units of `npkt` packets at `unit` packets each; a compute with only
// scalars still owns one.
inline uint64_t tiles_for(uint64_t npkt, uint64_t unit) {
  const uint64_t t = (npkt + unit - 1) / unit;
  return t ? t : 1;
}
// Validate pointers: element alignment, no partial overlap with the output.
int check_buffers(void *out, const void *const *in, int n, size_t count, size_t esz);
// A widened sum's pointers (inputs of `esz` bytes per element, an output of
// `osz`): element alignment on either side, osz * count within a size_t, and
// NO overlap of the output with any input -- the element sizes differ, so
// nothing can be summed in place.
int check_buffers_widened(void *out, const void *const *in, int n, size_t count, size_t esz, size_t osz);

}  // namespace hiccl_impl
