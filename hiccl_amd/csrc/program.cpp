// hiccl_amd/csrc/program.cpp -- hiccl_program_*: step programs (k_program:
// token phases folded into a unit batch's launch) and the stream-ordered
// protocol's defaults.
#include <string.h>

#include <cctype>
#include <cstdio>
#include <cstdlib>

#include "plan.h"

using namespace hiccl_impl;

struct hiccl_program {
  int dtype = 0;
  int device = 0;
  int op = HICCL_OP_SUM;  // the first reducing plan's (hiccl_program_add_plan)
  bool has_op = false;    // a reducing plan has been added
  struct Unit {
    void *out;
    std::vector<const void *> in;
    size_t count;
    bool bytes;  // exact byte copy (a HICCL_BYTES plan's compute)
    int peer;    // the plan's hiccl_reduce_plan_set_peer flags
  };
  std::vector<Unit> units;  // the unit batch (after the phases)
  struct Phase {
    std::vector<uint32_t *> sig;
    std::vector<const uint32_t *> wait;
  };
  std::vector<Phase> phases;  // the prologue
  bool dirty = true;
  char *d_block = nullptr;
  uint64_t *d_gate = nullptr;
  uint64_t seq = 0;  // last sequence number used (eager launches; captures reserve a range)
  ProgArgs args;
  int unroll = 4;
  uint32_t grid = 0;
  uint32_t max_wg = 0;  // hiccl_program_set_max_workgroups (0: default)
  std::atomic<bool> enqueued{false};
};

namespace {

// Workgroups per CU of a program launch: a small batch (under one 16 KiB
// tile per lane-group per CU, the C5 step) takes 4 like the plan kernel's
// small launches, larger ones 2.
constexpr int kProgSmallBpc = 4;
constexpr int kProgBpc = 2;

int prog_upload(hiccl_program *p, hipStream_t s) {
  if (!p->dirty) return 0;
  if (capturing(s, false))
    return fail(hipErrorStreamCaptureUnsupported,
                "program: the first launch after a change uploads the program and cannot be captured");
  sync_if_enqueued(p->enqueued);
  if (p->d_block) {
    (void)hipFree(p->d_block);
    p->d_block = nullptr;
  }
  if (!p->d_gate) {
    if (int e = check_hip(hipMalloc((void **)&p->d_gate, 256), "program: hipMalloc(gate)")) return e;
    if (int e = check_hip(hipMemset(p->d_gate, 0, 256), "program: hipMemset(gate)")) return e;
    p->seq = 0;
  }
  const int cus = device_cus(p->device);
  const size_t tesz = esize(p->dtype);
  auto esz_of = [&](const hiccl_program::Unit &u) { return u.bytes ? (size_t)1 : tesz; };
  uint64_t total_pkt = 0;
  size_t maxn = 1;
  for (auto &u : p->units) {
    total_pkt += split_on(u.out, u.count, esz_of(u)).npkt;
    if (u.in.size() > maxn) maxn = u.in.size();
  }
  // half-size tiles when the batch has under two 16 KiB tiles per CU (as a
  // plan's auto unroll)
  const bool small = total_pkt < 2ull * cus * kProgBlock * 4;
  p->unroll = pick_prog(p->dtype, p->op, 2) && small ? 2 : 4;
  DescTable t(maxn, (uint64_t)kProgBlock * p->unroll);
  for (auto &u : p->units)
    t.add(u.out, u.in.data(), u.in.size(), u.count, esz_of(u), (u.bytes ? 1u : 0u) | ((uint32_t)u.peer << 1));
  if (t.units > 0xffffffffull) return fail(hipErrorInvalidValue, "program: more than 2^32 tiles");
  ProgArgs &a = p->args;
  memset(&a, 0, sizeof(a));
  a.nunits = t.units;
  a.nphase = (uint32_t)p->phases.size();
  uint64_t grid = (uint64_t)cus * (small ? kProgSmallBpc : kProgBpc);
  if (p->max_wg && p->max_wg < grid) grid = p->max_wg;
  if (grid > a.nunits) grid = a.nunits;
  p->grid = (uint32_t)(grid ? grid : 1);  // a phases-only program: workgroup 0 alone
  // device block: [desc | ptrs | unit_comp] (the table) [| phases | sig | wait]
  size_t nsig = 0, nwait = 0;
  for (auto &ph : p->phases) {
    nsig += ph.sig.size();
    nwait += ph.wait.size();
  }
  auto al8 = [](size_t x) { return (x + 7) & ~(size_t)7; };
  const size_t o_ph = t.bytes();
  const size_t o_sig = al8(o_ph + p->phases.size() * sizeof(ProgPhase));
  const size_t o_wait = al8(o_sig + nsig * sizeof(void *));
  const size_t bytes = al8(o_wait + nwait * sizeof(void *)) + 8;
  std::vector<char> host = t.image(bytes - o_ph);
  {
    ProgPhase *hp = (ProgPhase *)(host.data() + o_ph);
    uint32_t **hs = (uint32_t **)(host.data() + o_sig);
    const uint32_t **hw = (const uint32_t **)(host.data() + o_wait);
    uint32_t si = 0, wi = 0;
    for (size_t i = 0; i < p->phases.size(); i++) {
      auto &ph = p->phases[i];
      hp[i].sig_begin = si;
      for (auto *f : ph.sig) hs[si++] = f;
      hp[i].sig_end = si;
      hp[i].wait_begin = wi;
      for (auto *f : ph.wait) hw[wi++] = f;
      hp[i].wait_end = wi;
    }
  }
  if (int e = check_hip(hipMalloc((void **)&p->d_block, bytes), "program: hipMalloc")) return e;
  if (int e = check_hip(hipMemcpy(p->d_block, host.data(), bytes, hipMemcpyHostToDevice), "program: upload"))
    return e;
  t.bind(a, p->d_block);
  a.phase = (const ProgPhase *)(p->d_block + o_ph);
  a.sig = (uint32_t *const *)(p->d_block + o_sig);
  a.wait = (const uint32_t *const *)(p->d_block + o_wait);
  a.gate = p->d_gate;
  p->dirty = false;
  return 0;
}

}  // namespace

extern "C" {

int hiccl_program_create(hiccl_program_t **prog, int dtype, int device) {
  if (!prog) return fail(hipErrorInvalidValue, "program_create: prog is NULL");
  *prog = nullptr;
  if (!pick_prog(dtype, HICCL_OP_SUM, 4)) return fail(hipErrorInvalidValue, "program_create: unsupported dtype");
  int ndev = 0;
  if (int e = check_hip(hipGetDeviceCount(&ndev), "program_create: hipGetDeviceCount")) return e;
  if (device < 0 || device >= ndev) return fail(hipErrorInvalidDevice, "program_create: bad device");
  auto *p = new hiccl_program;
  p->dtype = dtype;
  p->device = device;
  *prog = p;
  return 0;
}

int hiccl_program_add_signal(hiccl_program_t *p, uint32_t *const *sig, int nsig, const uint32_t *const *wait,
                             int nwait) {
  if (!p) return fail(hipErrorInvalidValue, "program_add_signal: prog is NULL");
  if (nsig < 0 || nwait < 0 || (nsig && !sig) || (nwait && !wait))
    return fail(hipErrorInvalidValue, "program_add_signal: bad flag lists");
  for (int i = 0; i < nsig; i++)
    if (!sig[i]) return fail(hipErrorInvalidValue, "program_add_signal: NULL signal flag");
  for (int i = 0; i < nwait; i++)
    if (!wait[i]) return fail(hipErrorInvalidValue, "program_add_signal: NULL wait flag");
  if (!p->units.empty())
    return fail(hipErrorInvalidValue, "program_add_signal: phases precede the program's units (start a new program)");
  if (p->phases.size() >= (size_t)kProgMaxPhases)
    return fail(hipErrorInvalidValue, "program_add_signal: more than 64 phases in one program");
  hiccl_program::Phase ph;
  ph.sig.assign(sig, sig + nsig);
  ph.wait.assign(wait, wait + nwait);
  p->phases.push_back(std::move(ph));
  p->dirty = true;
  return 0;
}

int hiccl_program_add_plan(hiccl_program_t *p, const hiccl_reduce_plan_t *plan) {
  if (!p || !plan) return fail(hipErrorInvalidValue, "program_add_plan: NULL argument");
  const bool bytes = plan->dtype == HICCL_BYTES;
  if (!bytes && plan->dtype != p->dtype)
    return fail(hipErrorInvalidValue, "program_add_plan: the plan's dtype is neither the program's nor HICCL_BYTES");
  if (plan->req.acc == HICCL_ACC_WIDE)
    return fail(hipErrorInvalidValue, "program_add_plan: programs accumulate natively (HICCL_ACC_NATIVE) only");
  if (plan->widened)
    return fail(hipErrorInvalidValue, "program_add_plan: programs take no widened plan (hiccl_reduce_plan_set_out_dtype): "
                                      "no program kernel changes type");
  if (plan->scaled)
    return fail(hipErrorInvalidValue, "program_add_plan: programs take no scaled plan (hiccl_reduce_plan_set_scale): "
                                      "they have no scale per compute");
  if (!bytes) {
    if (p->has_op && plan->op != p->op)
      return fail(hipErrorInvalidValue,
                  "program_add_plan: the plan's op differs from the op of the program's first reducing plan");
    if (!pick_prog(p->dtype, plan->op, 4))
      return fail(hipErrorInvalidValue, "program_add_plan: no program kernel for this dtype and op");
    p->op = plan->op;
    p->has_op = true;
  }
  const int peer = plan_eff_peer(plan);  // the plan's own store form (wt_by_size) carries over
  for (auto &c : plan->comps) p->units.push_back(hiccl_program::Unit{c.out, c.in, c.count, bytes, peer});
  p->dirty = true;
  return 0;
}

int hiccl_program_set_max_workgroups(hiccl_program_t *p, int max_wg) {
  if (!p) return fail(hipErrorInvalidValue, "program_set_max_workgroups: prog is NULL");
  if (max_wg < 0) return fail(hipErrorInvalidValue, "program_set_max_workgroups: max_wg < 0");
  p->max_wg = (uint32_t)max_wg;
  p->dirty = true;
  return 0;
}

int hiccl_program_num_units(const hiccl_program_t *p) { return p ? (int)p->units.size() : 0; }
int hiccl_program_num_phases(const hiccl_program_t *p) { return p ? (int)p->phases.size() : 0; }

int hiccl_program_launch(hiccl_program_t *p, const uint32_t *epochs, const uint32_t *epoch_dev, uint32_t *err,
                         double timeout_s, void *stream) {
  if (!p) return fail(hipErrorInvalidValue, "program_launch: prog is NULL");
  if (!p->phases.empty() && !epochs) return fail(hipErrorInvalidValue, "program_launch: epochs is NULL");
  if (int e = check_hip(hipSetDevice(p->device), "program_launch: hipSetDevice")) return e;
  if (p->phases.empty() && p->units.empty()) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (int e = prog_upload(p, s)) return e;
  prog_fn fn = pick_prog(p->dtype, p->op, p->unroll);
  if (!fn) return fail(hipErrorInvalidValue, "program_launch: no kernel for this dtype / shape");
  ProgArgs a = p->args;
  a.err = err;
  a.epoch_dev = epoch_dev;
  a.timeout_ticks = (uint64_t)((timeout_s > 0 ? timeout_s : 30.0) * 1e8);  // s_memrealtime: 100 MHz
  for (uint32_t i = 0; i < a.nphase; i++) a.epoch[i] = epochs[i];
  a.light = prog_light() ? 1u : 0u;
  // the gate's sequence number: one per eager launch; a captured launch
  // uses seq + *epoch_dev (replay r: seq + r) and reserves every value a
  // 32-bit *epoch_dev can add, so no later launch or re-capture of this
  // program reuses a value one of its replays stores (64-bit: no wrap)
  a.seq = ++p->seq;
  if (epoch_dev) p->seq += (1ull << 32);
  fn(a, dim3(p->grid), s);
  p->enqueued.store(true, std::memory_order_relaxed);
  return check_hip(hipGetLastError(), "program_launch: launch");
}

void hiccl_program_destroy(hiccl_program_t *p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  sync_if_enqueued(p->enqueued);
  if (p->d_block) (void)hipFree(p->d_block);
  if (p->d_gate) (void)hipFree(p->d_gate);
  delete p;
}

int hiccl_token_mode(void) { return prog_light() ? HICCL_TOKENS_LIGHT : HICCL_TOKENS_FENCED; }

// "1" / yes / on / true (any case) opt in; "0" / no / off / false / unset
// keep the default (off).  Round 3 read any value but "0" as on: a value
// that is neither spelling is read as off and named once on stderr, so a job
// script's protocol never changes without a word.
int hiccl_step_program_default(void) {
  const char *e = std::getenv("HICCL_STEP_PROGRAM");
  if (!e) return 0;
  std::string v(e);
  for (auto &ch : v) ch = (char)std::tolower((unsigned char)ch);
  if (v == "1" || v == "yes" || v == "on" || v == "true") return 1;
  if (!(v.empty() || v == "0" || v == "no" || v == "off" || v == "false")) {
    static std::atomic<bool> warned{false};
    if (!warned.exchange(true))
      std::fprintf(stderr, "HiCCL: HICCL_STEP_PROGRAM=%s not recognised (1/yes/on/true or 0/no/off/false); "
                           "step programs stay off\n", e);
  }
  return 0;
}

}  // extern "C"
