// hiccl_amd/csrc/plan.cpp -- hiccl_reduce_plan_*: every compute of a pipeline
// step in one launch from a device descriptor table.
#include "plan.h"

#include <string.h>

using namespace hiccl_impl;

namespace hiccl_impl {

void DescTable::add(void *out, const void *const *in, size_t n, size_t count, size_t esz, uint32_t flags) {
  const Split sp = split_on(out, count, esz);
  PlanDesc d;
  d.out = (char *)out;
  d.npkt = sp.npkt;
  d.tile_begin = units;
  d.n = (uint32_t)n;
  d.head = sp.head;
  d.tail = sp.tail;
  d.pad = flags;
  desc.push_back(d);
  for (size_t k = 0; k < stride; k++) ptrs.push_back(k < n ? in[k] : nullptr);
  units += tiles_for(sp.npkt, unit);
}

std::vector<char> DescTable::image(size_t extra) const {
  std::vector<char> host(bytes() + extra, 0);
  if (!desc.empty()) {
    memcpy(host.data(), desc.data(), ptrs_off());
    memcpy(host.data() + ptrs_off(), ptrs.data(), ptrs.size() * sizeof(void *));
  }
  if (desc.size() > 1) {
    uint32_t *uc = (uint32_t *)(host.data() + unit_comp_off());
    for (size_t c = 0; c < desc.size(); c++) {
      const uint64_t end = c + 1 < desc.size() ? desc[c + 1].tile_begin : units;
      for (uint64_t t = desc[c].tile_begin; t < end; t++) uc[t] = (uint32_t)c;
    }
  }
  return host;
}

bool sync_if_enqueued(std::atomic<bool> &enqueued) {
  if (!enqueued.load(std::memory_order_relaxed)) return false;
  (void)hipDeviceSynchronize();
  enqueued.store(false, std::memory_order_relaxed);
  return true;
}

int launch_plan(PlanArgsWeighted a, int dtype, const Cfg &c, double mean_n, int dev, hipStream_t s, int pol) {
  const bool weighted = is_weighted_op(c.op);
  const plan_fn fn = weighted ? nullptr : pick_plan(dtype, c.acc, c.op, c.engine, c.unroll, pol);
  const plan_w_fn wfn = weighted ? pick_plan_weighted(dtype, c.acc, c.op, c.engine, c.unroll, pol) : nullptr;
  if (!fn && !wfn)
    return fail(hipErrorInvalidValue, pol == kDefPol ? "plan: unsupported dtype / shape"
                                                     : "plan: no peer-policy kernel for this shape (PHASE default, "
                                                       "TILE unroll 4, f32 / bf16 / f16 also 2)");
  const LaunchShape L = launch_shape(c, mean_n, a.t_end - a.t_begin, device_cus(dev));
  a.grab = L.grab;
  a.sched = L.dynamic ? ticket_counter(dev, s) : nullptr;
  if (wfn) wfn(a, dim3((unsigned)L.grid), s);
  else fn(a, dim3((unsigned)L.grid), s);
  return check_hip(hipGetLastError(), "plan: launch");
}

// Store form of a plan's launches (see wt_by_size): write-through on request
// (store_policy 4) or by the bytes a launch writes and its packet-weighted
// inputs per output.
static int plan_store_peer(const hiccl_reduce_plan *p) {
  if (p->req.store_policy == kPolStoreSys + 1) return HICCL_PEER_STORES;
  uint64_t out = 0;
  double weighted_n = 0;
  for (auto &c : p->comps) {
    out += (uint64_t)c.count * p->osz;  // the bytes WRITTEN
    weighted_n += (double)c.count * (double)c.in.size();
  }
  const double n = out ? weighted_n * (double)p->osz / (double)out : 0.0;
  return wt_by_size(resolve(&p->req), p->dtype, n, out) ? HICCL_PEER_STORES : 0;
}

int plan_eff_peer(const hiccl_reduce_plan *p) { return p->peer | plan_store_peer(p); }

}  // namespace hiccl_impl

namespace {

// Before the plan's device block is freed: no launch may still read it.
void plan_quiesce(hiccl_reduce_plan *p) {
  if (!sync_if_enqueued(p->enqueued) && p->launched) (void)hipStreamSynchronize(p->last);
}

// The plan's configuration with its engine and shape resolved for `npkt`
// packets of packet-weighted mean `mean_n` inputs.
Cfg plan_cfg(const hiccl_reduce_plan *p, uint64_t npkt, double mean_n) {
  Cfg c = resolve(&p->req);
  c.op = p->kernel_op();
  const bool auto_unroll = !c.unroll;
  // AUTO's engine rules follow the store form the launches take by size
  c.wt = c.store_auto && plan_store_peer(p);
  finish_cfg(c, npkt, mean_n, p->dtype, p->device);
  // peer and write-through policies: wide tiles become U = 4
  if (p->eff_peer && c.engine == HICCL_ENGINE_TILE && auto_unroll && !wt_unroll(c.unroll)) c.unroll = kDefUnroll;
  return c;
}

int plan_upload(hiccl_reduce_plan *p, hipStream_t s) {
  if (!p->dirty) return 0;
  // synchronous allocation + copy: not allowed inside a stream capture
  // (capture a plan only after a launch outside the capture uploaded it)
  if (capturing(s, false))
    return fail(hipErrorStreamCaptureUnsupported,
                "plan: the first launch after an add or a config change uploads the plan and cannot be captured");
  if (p->d_block) {
    plan_quiesce(p);  // a running launch still reads it
    (void)hipFree(p->d_block);
    p->d_block = nullptr;
  }
  uint64_t total_pkt = 0;
  double weighted_n = 0;
  size_t maxn = 0;
  for (auto &c : p->comps) {
    const uint64_t k = split_on(c.out, c.count, p->osz).npkt;
    total_pkt += k;
    weighted_n += (double)k * c.in.size();
    if (c.in.size() > maxn) maxn = c.in.size();
  }
  p->mean_n = total_pkt ? weighted_n / total_pkt : 0;
  p->eff_peer = plan_eff_peer(p);
  const Cfg c = plan_cfg(p, total_pkt, p->mean_n);
  p->engine = c.engine;
  p->unroll = c.unroll;
  p->bpc = c.bpc;
  DescTable t(maxn, unit_pkts(p->engine, p->dtype, c.acc, p->unroll, c.op));
  // (the flag is read by the mixed kernels alone: every other plan kernel takes pad for zero)
  for (auto &cp : p->comps)
    t.add(cp.out, cp.in.data(), cp.in.size(), cp.count, p->osz, cp.unscaled ? kDescUnscaled : 0u);
  // a weighted plan: one weight pointer per compute behind the table
  std::vector<char> host = t.image(p->weighted ? p->comps.size() * sizeof(const float *) : 0);
  if (p->weighted) {
    const float **w = (const float **)(host.data() + t.bytes());
    for (size_t i = 0; i < p->comps.size(); i++) w[i] = p->comps[i].weights;
  }
  if (int e = check_hip(hipMalloc((void **)&p->d_block, host.size()), "plan: hipMalloc")) return e;
  if (int e = check_hip(hipMemcpy(p->d_block, host.data(), host.size(), hipMemcpyHostToDevice), "plan: upload"))
    return e;
  memset(&p->args, 0, sizeof(p->args));
  t.bind(p->args, p->d_block);
  p->args.t_begin = 0;
  p->args.t_end = t.units;
  p->d_weights = p->weighted ? (const float *const *)(p->d_block + t.bytes()) : nullptr;
  p->dirty = false;
  return 0;
}

int plan_kernel(hiccl_reduce_plan *p, hipStream_t s) {
  Cfg c = resolve(&p->req);
  c.op = p->kernel_op();
  c.engine = p->engine;
  c.unroll = p->unroll;
  c.block = p->engine == HICCL_ENGINE_PHASE ? kPhBlock : kDefBlock;
  c.bpc = p->bpc;
  PlanArgsWeighted a;  // the plan itself is only read (hiccl_reduce_plan_enqueue from several threads)
  (PlanArgs &)a = p->args;
  a.scale = p->kernel_scale();
  a.weights = p->d_weights;
  return launch_plan(a, p->dtype, c, p->mean_n, p->device, s, plan_pol(p->eff_peer));
}

// Upload (if needed) and launch, no bookkeeping of where the launch went.
int plan_enqueue_impl(hiccl_reduce_plan_t *p, hipStream_t s, const char *what) {
  if (!p) return fail(hipErrorInvalidValue, std::string(what) + ": plan is NULL");
  if (int e = check_hip(hipSetDevice(p->device), (std::string(what) + ": hipSetDevice").c_str())) return e;
  if (p->comps.empty()) return 0;
  if (int e = plan_upload(p, s)) return e;
  return plan_kernel(p, s);
}

// One field of the plan's config changed: validate the whole, then keep it.
int plan_set_field(hiccl_reduce_plan_t *p, int hiccl_reduce_config_t::*field, int value, const char *who) {
  if (!p) return fail(hipErrorInvalidValue, std::string(who) + ": plan is NULL");
  hiccl_reduce_config_t c = p->req;
  c.*field = value;
  if (int e = check_cfg(&c, who)) return e;
  if (int e = check_op(p->dtype, c.acc, p->op, who)) return e;
  if (p->widened && c.acc != HICCL_ACC_NATIVE)
    return fail(hipErrorInvalidValue, std::string(who) + ": a widened plan always accumulates in f32: leave acc at "
                                                         "HICCL_ACC_NATIVE");
  p->req = c;
  p->dirty = true;  // (the auto engine's chunk size depends on the accumulator, too)
  return 0;
}

// Does every engine config `c` may resolve to have a plan kernel of operator
// `op` (a hiccl_op_t, kOpScaledSum, kOpWidenSum or kOpWidenAccum) in the shape `c` names?  Empty string if
// so, else why not.  No device work.
std::string plan_config_error(const hiccl_reduce_plan *p, const hiccl_reduce_config_t &c, int op) {
  Cfg r = resolve(&c);
  r.op = op;
  const bool shape = c.block || c.unroll;
  if (shape && r.engine == HICCL_ENGINE_AUTO) r.engine = HICCL_ENGINE_TILE;
  const int engines[2] = {HICCL_ENGINE_TILE, HICCL_ENGINE_PHASE};
  for (int eng : engines) {
    if (r.engine != HICCL_ENGINE_AUTO && r.engine != eng) continue;
    Cfg t = r;
    t.engine = eng;
    if (!t.block) t.block = eng == HICCL_ENGINE_PHASE ? kPhBlock : kDefBlock;
    if (!t.unroll) t.unroll = eng == HICCL_ENGINE_PHASE ? phase_p(p->dtype, t.acc, t.op) : kDefUnroll;
    const std::string why = plan_shape_error(t, p->dtype);
    if (!why.empty()) return why;
  }
  return "";
}

}  // namespace

extern "C" {

int hiccl_reduce_plan_create(hiccl_reduce_plan_t **plan, int dtype, int device) {
  if (!plan) return fail(hipErrorInvalidValue, "plan_create: plan is NULL");
  *plan = nullptr;
  if (!esize(dtype)) return fail(hipErrorInvalidValue, "plan_create: unknown dtype");
  int ndev = 0;
  if (int e = check_hip(hipGetDeviceCount(&ndev), "plan_create: hipGetDeviceCount")) return e;
  if (device < 0 || device >= ndev) return fail(hipErrorInvalidDevice, "plan_create: bad device");
  if (int e = check_hip(hipSetDevice(device), "plan_create: hipSetDevice")) return e;
  auto *p = new hiccl_reduce_plan;
  memset(&p->req, 0, sizeof(p->req));
  p->dtype = dtype;
  p->device = device;
  p->esz = esize(dtype);
  p->osz = p->esz;
  // the plan's own stream is created on first request (hiccl_reduce_plan_stream):
  // callers that launch on a shared stream never pay for one
  *plan = p;
  return 0;
}

int hiccl_reduce_plan_set_acc(hiccl_reduce_plan_t *p, int acc) {
  return plan_set_field(p, &hiccl_reduce_config_t::acc, acc, "plan_set_acc");
}

int hiccl_reduce_plan_set_op(hiccl_reduce_plan_t *p, int op) {
  if (!p) return fail(hipErrorInvalidValue, "plan_set_op: plan is NULL");
  if (int e = check_op(p->dtype, p->req.acc, op, "plan_set_op")) return e;
  if (p->scaled && op != HICCL_OP_SUM)
    return fail(hipErrorInvalidValue, "plan_set_op: a scaled plan sums (HICCL_OP_SUM only): clear the scale first");
  if (p->widened && op != HICCL_OP_SUM)
    return fail(hipErrorInvalidValue, "plan_set_op: a widened plan sums (HICCL_OP_SUM only)");
  p->op = op;
  p->dirty = true;  // (AUTO's shape depends on the operator: MAX and MIN are untuned)
  return 0;
}

int hiccl_reduce_plan_op(const hiccl_reduce_plan_t *p) { return p ? p->op : -1; }

int hiccl_reduce_plan_set_scale(hiccl_reduce_plan_t *p, const double *alpha) {
  if (!p) return fail(hipErrorInvalidValue, "plan_set_scale: plan is NULL");
  Scale sc{0.0, 0.0f, 0u};
  if (alpha) {
    if (int e = check_scale(p->dtype, *alpha, "plan_set_scale", &sc)) return e;
    if (p->op != HICCL_OP_SUM)
      return fail(hipErrorInvalidValue, "plan_set_scale: only sums are scaled (the plan's op is not HICCL_OP_SUM)");
    // the scaled kernels are untuned: a config that names a shape only the
    // tuned sums have (TILE unroll 1, 2, 8, 16) is refused here, not at launch
    const std::string why = plan_config_error(p, p->req, p->widened ? p->kernel_op() : kOpScaledSum);
    if (!why.empty())
      return fail(hipErrorInvalidValue, "plan_set_scale: the plan's config names a shape the scaled kernels lack: " + why);
  }
  // a scaled sum is another kernel, untuned: AUTO's shape may differ.  A new
  // alpha alone travels in the kernel arguments and needs no upload (nor does
  // the scale of a widened plan, whose kernel is the same with and without).
  if (p->scaled != (alpha != nullptr) && !p->widened) p->dirty = true;
  p->scaled = alpha != nullptr;
  p->scale = sc;
  return 0;
}

int hiccl_reduce_plan_scale(const hiccl_reduce_plan_t *p, double *alpha) {
  if (!p) return -1;
  if (p->scaled && alpha) *alpha = p->scale.a64;
  return p->scaled ? 1 : 0;
}

int hiccl_reduce_plan_set_out_dtype(hiccl_reduce_plan_t *p, int out_dtype) {
  if (!p) return fail(hipErrorInvalidValue, "plan_set_out_dtype: plan is NULL");
  if (!p->comps.empty())
    return fail(hipErrorInvalidValue, "plan_set_out_dtype: the output dtype is set before the first add (the plan holds " +
                                          std::to_string(p->comps.size()) + " computes)");
  if (int e = check_widened(p->dtype, out_dtype, p->req.acc, nullptr, "plan_set_out_dtype", nullptr)) return e;
  if (p->op != HICCL_OP_SUM)
    return fail(hipErrorInvalidValue, "plan_set_out_dtype: only sums are widened (the plan's op is not HICCL_OP_SUM)");
  // the widened kernels are untuned: a config that names a shape only the
  // tuned sums have is refused here, not at launch
  const std::string why = plan_config_error(p, p->req, kOpWidenSum);
  if (!why.empty())
    return fail(hipErrorInvalidValue, "plan_set_out_dtype: the plan's config names a shape the widened kernels lack: " + why);
  p->widened = true;
  p->osz = esize(out_dtype);
  p->dirty = true;
  return 0;
}

int hiccl_reduce_plan_set_accumulate(hiccl_reduce_plan_t *p, int on) {
  if (!p) return fail(hipErrorInvalidValue, "plan_set_accumulate: plan is NULL");
  if (on) {
    if (!p->widened)
      return fail(hipErrorInvalidValue, "plan_set_accumulate: only a widened plan accumulates (hiccl_reduce_plan_set_out_dtype "
                                        "first): a same-type sum accumulates by passing out as input 0");
    if (p->peer & HICCL_PEER_STORES)
      return fail(hipErrorInvalidValue, "plan_set_accumulate: an accumulating plan takes no HICCL_PEER_STORES (the old output "
                                        "is read where it is written: keep it in local memory)");
    // the accumulating kernels are untuned, as the widened ones: the same shapes
    const std::string why = plan_config_error(p, p->req, p->weighted ? kOpWeightedAccum : kOpWidenAccum);
    if (!why.empty())
      return fail(hipErrorInvalidValue,
                  "plan_set_accumulate: the plan's config names a shape the accumulating kernels lack: " + why);
  } else if (p->accumulate) {
    // back to the widened kernels, whose PHASE shape is not the accumulating
    // ones': a config that names the latter is refused here, not replaced
    const std::string why = plan_config_error(p, p->req, p->weighted ? kOpWeightedSum : kOpWidenSum);
    if (!why.empty())
      return fail(hipErrorInvalidValue,
                  "plan_set_accumulate: the plan's config names a shape the widened kernels lack: " + why);
  }
  // another kernel: the next launch uploads again (a new alpha alone does not)
  if (p->accumulate != (on != 0)) p->dirty = true;
  p->accumulate = on != 0;
  return 0;
}

int hiccl_reduce_plan_accumulate(const hiccl_reduce_plan_t *p) { return !p ? -1 : p->accumulate ? 1 : 0; }

int hiccl_reduce_plan_set_weighted(hiccl_reduce_plan_t *p, int on) {
  if (!p) return fail(hipErrorInvalidValue, "plan_set_weighted: plan is NULL");
  if (!p->comps.empty())
    return fail(hipErrorInvalidValue, "plan_set_weighted: a plan is made weighted before the first add (the plan holds " +
                                          std::to_string(p->comps.size()) + " computes)");
  if (on && !p->widened)
    return fail(hipErrorInvalidValue, "plan_set_weighted: only a widened plan is weighted (hiccl_reduce_plan_set_out_dtype "
                                      "first): same-type weighted sums are not implemented");
  // the weighted kernels come in the widened and accumulating ones' shapes, but
  // their PHASE chunk is their own: a config that names another is refused
  // here, never replaced
  const int op = on ? (p->accumulate ? kOpWeightedAccum : kOpWeightedSum) : (p->accumulate ? kOpWidenAccum : kOpWidenSum);
  if (p->widened) {
    const std::string why = plan_config_error(p, p->req, op);
    if (!why.empty())
      return fail(hipErrorInvalidValue, std::string("plan_set_weighted: the plan's config names a shape the ") +
                                            (on ? "weighted" : "unweighted") + " kernels lack: " + why);
  }
  if (p->weighted != (on != 0)) p->dirty = true;
  p->weighted = on != 0;
  return 0;
}

int hiccl_reduce_plan_weighted(const hiccl_reduce_plan_t *p) { return !p ? -1 : p->weighted ? 1 : 0; }

int hiccl_reduce_plan_out_dtype(const hiccl_reduce_plan_t *p) {
  return !p ? -1 : p->widened ? (int)HICCL_FLOAT32 : p->dtype;
}

int hiccl_reduce_plan_set_engine(hiccl_reduce_plan_t *p, int engine) {
  return plan_set_field(p, &hiccl_reduce_config_t::engine, engine, "plan_set_engine");
}

int hiccl_reduce_plan_set_peer(hiccl_reduce_plan_t *p, int flags) {
  if (!p) return fail(hipErrorInvalidValue, "plan_set_peer: plan is NULL");
  if (flags & ~(HICCL_PEER_STORES | HICCL_PEER_LOADS))
    return fail(hipErrorInvalidValue, "plan_set_peer: flags must be a combination of HICCL_PEER_STORES and HICCL_PEER_LOADS");
  if (p->accumulate && (flags & HICCL_PEER_STORES))
    return fail(hipErrorInvalidValue, "plan_set_peer: an accumulating plan takes no HICCL_PEER_STORES (the old output is "
                                      "read where it is written: keep it in local memory)");
  p->peer = flags;
  p->dirty = true;
  return 0;
}

int hiccl_reduce_plan_peer(const hiccl_reduce_plan_t *p) { return p ? p->peer : -1; }

int hiccl_reduce_plan_store_policy(const hiccl_reduce_plan_t *p) {
  if (!p) return -1;
  return (plan_eff_peer(p) & HICCL_PEER_STORES) ? kPolStoreSys + 1 : kDefPol / 10 + 1;
}

int hiccl_reduce_plan_set_config(hiccl_reduce_plan_t *p, const hiccl_reduce_config_t *cfg) {
  if (!p) return fail(hipErrorInvalidValue, "plan_set_config: plan is NULL");
  hiccl_reduce_config_t z;
  memset(&z, 0, sizeof(z));
  const hiccl_reduce_config_t &c = cfg ? *cfg : z;
  if (int e = check_cfg(&c, "plan_set_config")) return e;
  if (int e = check_op(p->dtype, c.acc, p->op, "plan_set_config")) return e;
  if (p->widened && c.acc != HICCL_ACC_NATIVE)
    return fail(hipErrorInvalidValue, "plan_set_config: a widened plan always accumulates in f32: leave acc at "
                                      "HICCL_ACC_NATIVE");
  // the shape must be one the plan kernels have, whatever engine AUTO picks
  const std::string why = plan_config_error(p, c, p->config_op());
  if (!why.empty()) return fail(hipErrorInvalidValue, "plan_set_config: " + why);
  p->req = c;
  p->dirty = true;
  return 0;
}

int hiccl_reduce_plan_engine(const hiccl_reduce_plan_t *p) { return p ? p->engine : -1; }

static int plan_add_impl(hiccl_reduce_plan_t *p, void *out, const void *const *in, int n, size_t count, bool unscaled,
                         const std::string &who, const float *weights = nullptr, bool weighted = false) {
  if (!p) return fail(hipErrorInvalidValue, who + ": plan is NULL");
  if (p->weighted && !weighted)
    return fail(hipErrorInvalidValue, who + ": a weighted plan takes weighted computes only (hiccl_reduce_plan_add_weighted: "
                                            "its kernels read n weights per compute)");
  if (!p->weighted && weighted)
    return fail(hipErrorInvalidValue, who + ": the plan is not weighted (hiccl_reduce_plan_set_weighted before the first add)");
  if (unscaled && p->widened)
    return fail(hipErrorInvalidValue, who + ": a widened or accumulating plan takes no unscaled compute (its kernels "
                                            "always multiply: one scale per plan)");
  if (p->dtype == HICCL_BYTES && n != 1) return fail(hipErrorInvalidValue, who + ": HICCL_BYTES copies need n == 1");
  if (p->widened) {
    if (int e = check_buffers_widened(out, in, n, count, p->esz, p->osz)) return e;
  } else if (int e = check_buffers(out, in, n, count, p->esz)) {
    return e;
  }
  if (weighted)
    if (int e = check_weights(out, weights, n, count, who)) return e;
  if (count == 0) return 0;
  hiccl_reduce_plan::Comp c;
  c.weights = weights;
  c.out = out;
  c.in.assign(in, in + n);
  c.count = count;
  c.unscaled = unscaled;
  p->comps.push_back(std::move(c));
  if (unscaled) p->num_unscaled++;
  p->dirty = true;  // (and the kernel family of a scaled plan may change: kernel_op)
  return 0;
}

int hiccl_reduce_plan_add(hiccl_reduce_plan_t *p, void *out, const void *const *in, int n, size_t count) {
  return plan_add_impl(p, out, in, n, count, false, "plan_add");
}

int hiccl_reduce_plan_add_unscaled(hiccl_reduce_plan_t *p, void *out, const void *const *in, int n, size_t count) {
  return plan_add_impl(p, out, in, n, count, true, "plan_add_unscaled");
}

int hiccl_reduce_plan_add_weighted(hiccl_reduce_plan_t *p, void *out, const void *const *in, const float *weights, int n,
                                   size_t count) {
  return plan_add_impl(p, out, in, n, count, false, "plan_add_weighted", weights, true);
}

int hiccl_reduce_plan_num_unscaled(const hiccl_reduce_plan_t *p) { return p ? (int)p->num_unscaled : 0; }

int hiccl_reduce_plan_enqueue(hiccl_reduce_plan_t *p, void *stream) {
  if (int e = plan_enqueue_impl(p, (hipStream_t)stream, "plan_enqueue")) return e;
  // no stream bookkeeping (callers on several threads and streams); a
  // re-upload or destroy then synchronises the device before it frees the
  // block a launch may still read
  if (!p->comps.empty()) p->enqueued.store(true, std::memory_order_relaxed);
  return 0;
}

int hiccl_reduce_plan_launch(hiccl_reduce_plan_t *p, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (int e = plan_enqueue_impl(p, s, "plan_launch")) return e;
  if (p->comps.empty()) return 0;
  // a capturing stream is not remembered (plan_sync does not apply to graph
  // replays: synchronise the stream the graph runs on); a re-upload or
  // destroy of a plan captured into a graph synchronises the device
  if (capturing(s, false)) {
    p->enqueued.store(true, std::memory_order_relaxed);
    return 0;
  }
  p->launched = true;
  p->last = s;
  return 0;
}

int hiccl_reduce_plan_launch_each(hiccl_reduce_plan_t *p, void *stream) {
  if (!p) return fail(hipErrorInvalidValue, "plan_launch_each: plan is NULL");
  if (int e = check_hip(hipSetDevice(p->device), "plan_launch_each: hipSetDevice")) return e;
  if (p->comps.empty()) return 0;
  // One one-shot launch per compute, each with the engine AUTO picks for that
  // compute alone (the reference's structure, compute.h:88-91).
  const Scale sc = p->kernel_scale();
  for (auto &c : p->comps) {
    // an unscaled compute of a scaled plan is a plain sum (a widened plan has none)
    const bool plain = !p->widened && (!p->scaled || c.unscaled);
    if (int e = reduce_call(p->dtype, plain ? p->op : p->widened ? p->kernel_op() : kOpScaledSum, plain ? nullptr : &sc,
                            c.out, c.in.data(), (int)c.in.size(), c.count, stream, &p->req, c.weights))
      return e;
  }
  p->launched = true;
  p->last = (hipStream_t)stream;
  return 0;
}

int hiccl_reduce_plan_sync(hiccl_reduce_plan_t *p) {
  if (!p) return fail(hipErrorInvalidValue, "plan_sync: plan is NULL");
  if (!p->launched) return 0;
  if (int e = check_hip(hipSetDevice(p->device), "plan_sync: hipSetDevice")) return e;
  // the reference's wait(): hipStreamSynchronize of the compute's stream
  // (compute.h:107-117) -- no completion event per launch (an event record
  // after every kernel costs the queue ~3 us per step on MI355X)
  if (int e = check_hip(hipStreamSynchronize(p->last), "plan_sync")) return e;
  // nothing of this plan is pending on that stream any more: a later
  // re-upload or destroy does not touch it (the caller may destroy it)
  p->launched = false;
  return 0;
}

int hiccl_reduce_plan_numcomp(const hiccl_reduce_plan_t *p) { return p ? (int)p->comps.size() : 0; }

void *hiccl_reduce_plan_stream(hiccl_reduce_plan_t *p) {
  if (!p) return nullptr;
  if (!p->own) {
    if (check_hip(hipSetDevice(p->device), "plan_stream: hipSetDevice")) return nullptr;
    if (check_hip(hipStreamCreateWithFlags(&p->own, hipStreamNonBlocking), "plan_stream: create")) return nullptr;
  }
  return (void *)p->own;
}

size_t hiccl_reduce_plan_bytes(const hiccl_reduce_plan_t *p) {
  if (!p) return 0;
  size_t b = 0;
  // an accumulating plan reads the old output and writes the new one
  const size_t obytes = p->accumulate ? 2 * p->osz : p->osz;
  for (auto &c : p->comps) b += c.count * (c.in.size() * p->esz + obytes);
  return b;
}

void hiccl_reduce_plan_destroy(hiccl_reduce_plan_t *p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  if (p->d_block) plan_quiesce(p);
  else if (p->launched) (void)hipStreamSynchronize(p->last);
  if (p->d_block) (void)hipFree(p->d_block);
  if (p->own) (void)hipStreamDestroy(p->own);
  delete p;
}

}  // extern "C"
