// hiccl_amd/csrc/signal.cpp -- hiccl_signal_wait*, hiccl_counter_add:
// stream-ordered transport signalling (k_sigwait_phases).
#include <string.h>

#include "runtime.h"

using namespace hiccl_impl;

extern "C" {

int hiccl_signal_wait(uint32_t *const *sig, int nsig, const uint32_t *const *wait, int nwait,
                      uint32_t epoch, uint32_t *err, double timeout_s, void *stream) {
  return hiccl_signal_wait_dev(sig, nsig, wait, nwait, epoch, nullptr, err, timeout_s, stream);
}

int hiccl_counter_add(uint32_t *ctr, uint32_t v, void *stream) {
  if (!ctr) return fail(hipErrorInvalidValue, "counter_add: ctr is NULL");
  launch_counter_add(ctr, v, (hipStream_t)stream);
  return check_hip(hipGetLastError(), "counter_add: launch");
}

int hiccl_signal_wait_dev(uint32_t *const *sig, int nsig, const uint32_t *const *wait, int nwait,
                          uint32_t epoch, const uint32_t *epoch_dev, uint32_t *err, double timeout_s,
                          void *stream) {
  hiccl_signal_phase_t ph;
  ph.sig = sig;
  ph.nsig = nsig;
  ph.wait = wait;
  ph.nwait = nwait;
  ph.epoch = epoch;
  return hiccl_signal_wait_phases(&ph, 1, epoch_dev, err, timeout_s, stream);
}

int hiccl_signal_wait_phases(const hiccl_signal_phase_t *ph, int nph, const uint32_t *epoch_dev, uint32_t *err,
                             double timeout_s, void *stream) {
  if (nph < 0 || (nph && !ph)) return fail(hipErrorInvalidValue, "signal_wait: bad phase list");
  for (int p = 0; p < nph; p++) {
    const hiccl_signal_phase_t &q = ph[p];
    if (q.nsig < 0 || q.nwait < 0 || (q.nsig && !q.sig) || (q.nwait && !q.wait))
      return fail(hipErrorInvalidValue, "signal_wait: bad flag lists");
    for (int i = 0; i < q.nsig; i++)
      if (!q.sig[i]) return fail(hipErrorInvalidValue, "signal_wait: NULL signal flag");
    for (int i = 0; i < q.nwait; i++)
      if (!q.wait[i]) return fail(hipErrorInvalidValue, "signal_wait: NULL wait flag");
  }
  const uint64_t ticks = (uint64_t)((timeout_s > 0 ? timeout_s : 30.0) * 1e8);  // s_memrealtime: 100 MHz
  hipStream_t s = (hipStream_t)stream;
  SigPhaseArgs a;
  const uint32_t light = prog_light() ? 1u : 0u;
  auto reset = [&]() {
    memset(&a, 0, sizeof(a));
    a.err = err;
    a.epoch_dev = epoch_dev;
    a.timeout_ticks = ticks;
    a.light = light;
  };
  auto launch = [&]() -> int {
    if (!a.nphase) return 0;
    launch_sigwait_phases(a, s);
    int e = check_hip(hipGetLastError(), "signal_wait: launch");
    reset();
    return e;
  };
  // Append (sig[0..ns), wait[0..nw)) with `epoch` as one sub-phase, starting
  // a new launch when the kernel's arrays or phase slots are full.
  auto push = [&](uint32_t *const *sg, int ns, const uint32_t *const *wt, int nw, uint32_t epoch) -> int {
    if (a.nphase == (uint32_t)kMaxPhases ||
        (a.nphase ? a.sig_end[a.nphase - 1] : 0) + ns > (uint32_t)kMaxFlags ||
        (a.nphase ? a.wait_end[a.nphase - 1] : 0) + nw > (uint32_t)kMaxFlags)
      if (int e = launch()) return e;
    const uint32_t s0 = a.nphase ? a.sig_end[a.nphase - 1] : 0, w0 = a.nphase ? a.wait_end[a.nphase - 1] : 0;
    for (int i = 0; i < ns; i++) a.sig[s0 + i] = sg[i];
    for (int i = 0; i < nw; i++) a.wait[w0 + i] = wt[i];
    a.sig_end[a.nphase] = s0 + ns;
    a.wait_end[a.nphase] = w0 + nw;
    a.epoch[a.nphase] = epoch;
    a.nphase++;
    return 0;
  };
  reset();
  for (int p = 0; p < nph; p++) {
    const hiccl_signal_phase_t &q = ph[p];
    if (q.nsig + q.nwait == 0) continue;
    if (q.nsig <= kMaxFlags && q.nwait <= kMaxFlags) {
      if (int e = push(q.sig, q.nsig, q.wait, q.nwait, q.epoch)) return e;
      continue;
    }
    // a phase above kMaxFlags: every signal first, then the waits, in
    // kMaxFlags pieces (a wait must never precede a signal of its phase)
    for (int i = 0; i < q.nsig; i += kMaxFlags)
      if (int e = push(q.sig + i, q.nsig - i < kMaxFlags ? q.nsig - i : kMaxFlags, nullptr, 0, q.epoch)) return e;
    for (int i = 0; i < q.nwait; i += kMaxFlags)
      if (int e = push(nullptr, 0, q.wait + i, q.nwait - i < kMaxFlags ? q.nwait - i : kMaxFlags, q.epoch))
        return e;
  }
  return launch();
}

}  // extern "C"
