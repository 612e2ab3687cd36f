// hiccl_amd/csrc/oneshot.cpp -- hiccl_reduce*: one reduction per call, and
// hiccl_reduce_auto_choice*: what AUTO would pick for it.
#include <string.h>

#include <cmath>

#include "plan.h"

using namespace hiccl_impl;

namespace {

uint32_t log2u(int v) {
  uint32_t l = 0;
  while (v > 1) {
    v >>= 1;
    l++;
  }
  return l;
}

// Large-n one-shot path: stage the pointer table in stream-ordered device
// memory and run it as a one-compute plan.
// A weighted sum's one weight pointer -- the caller's, passed along, not copied
// -- goes behind the table (PlanArgsWeighted.weights).
int reduce_via_table(int dtype, const Cfg &c, const Scale &scale, void *out, const void *const *in, int n,
                     size_t count, hipStream_t s, const float *weights) {
  DescTable t((size_t)n, unit_pkts(c.engine, dtype, c.acc, c.unroll, c.op));
  t.add(out, in, (size_t)n, count, out_esize(dtype, c.op));
  std::vector<char> host = t.image(is_weighted_op(c.op) ? sizeof(weights) : 0);
  if (is_weighted_op(c.op)) memcpy(host.data() + t.bytes(), &weights, sizeof(weights));
  char *dmem = nullptr;
  if (int e = check_hip(hipMallocAsync((void **)&dmem, host.size(), s), "hiccl_reduce: hipMallocAsync")) return e;
  // hipMemcpyAsync from pageable memory returns once the source is consumed,
  // so `host` may go out of scope (never under capture: refused by the caller)
  if (int e = check_hip(hipMemcpyAsync(dmem, host.data(), host.size(), hipMemcpyHostToDevice, s),
                        "hiccl_reduce: table upload")) {
    (void)hipFreeAsync(dmem, s);
    return e;
  }
  PlanArgsWeighted a;
  memset(&a, 0, sizeof(a));
  t.bind(a, dmem);
  a.t_begin = 0;
  a.t_end = t.units;
  a.scale = scale;
  if (is_weighted_op(c.op)) a.weights = (const float *const *)(dmem + t.bytes());
  // the store form oneshot_cfg decided: write-through by size or on request
  // (store_policy 4), else nt
  const int pol = plan_pol(c.store == kPolStoreSys ? HICCL_PEER_STORES : 0);
  if (int e = launch_plan(a, dtype, c, n, current_device(), s, pol)) {
    (void)hipFreeAsync(dmem, s);  // nothing launched reads it
    return e;
  }
  return check_hip(hipFreeAsync(dmem, s), "hiccl_reduce: hipFreeAsync");
}

}  // namespace

namespace hiccl_impl {

int check_scale(int dtype, double alpha, const std::string &who, Scale *scale) {
  const size_t esz = esize(dtype);
  if (!esz) return fail(hipErrorInvalidValue, who + ": unknown dtype " + std::to_string(dtype));
  if (dtype != HICCL_FLOAT32 && dtype != HICCL_FLOAT64 && dtype != HICCL_BFLOAT16 && dtype != HICCL_FLOAT16 &&
      dtype != HICCL_FLOAT8_E4M3 && dtype != HICCL_FLOAT8_E5M2)
    return fail(hipErrorInvalidValue, who + ": scaled sums take the floating types only (HICCL_FLOAT32, HICCL_FLOAT64, "
                                            "HICCL_BFLOAT16, HICCL_FLOAT16, HICCL_FLOAT8_E4M3, HICCL_FLOAT8_E5M2)");
  if (!std::isfinite(alpha)) return fail(hipErrorInvalidValue, who + ": alpha must be finite");
  const float a32 = (float)alpha;  // round to nearest even
  if (dtype != HICCL_FLOAT64 && !std::isfinite(a32))
    return fail(hipErrorInvalidValue, who + ": alpha must be finite as a float ((float)alpha overflows)");
  if (scale) *scale = Scale{alpha, a32, 0u};
  return 0;
}

bool widen_in_dtype(int dtype) {
  return dtype == HICCL_BFLOAT16 || dtype == HICCL_FLOAT16 || dtype == HICCL_FLOAT8_E4M3 || dtype == HICCL_FLOAT8_E5M2;
}

int check_weights(const void *out, const float *weights, int n, size_t count, const std::string &who) {
  if (n <= 0) return 0;  // nothing reads them: NULL is fine
  if (!weights) return fail(hipErrorInvalidValue, who + ": weights is NULL (n floats in device memory, one per input)");
  if ((uintptr_t)weights % sizeof(float))
    return fail(hipErrorInvalidValue, who + ": weights must be 4-byte aligned");
  const uintptr_t w0 = (uintptr_t)weights, w1 = w0 + (size_t)n * sizeof(float);
  const uintptr_t o0 = (uintptr_t)out, o1 = o0 + count * sizeof(float);
  if (count && w0 < o1 && o0 < w1)
    return fail(hipErrorInvalidValue, who + ": the weights overlap the output (the kernels read them while they write it)");
  return 0;
}

int check_widened(int in_dtype, int out_dtype, int acc, const double *alpha, const std::string &who, Scale *scale) {
  if (out_dtype != HICCL_FLOAT32)
    return fail(hipErrorInvalidValue, who + ": a widened sum writes HICCL_FLOAT32 only (out_dtype " +
                                          std::to_string(out_dtype) + ")");
  if (!widen_in_dtype(in_dtype))
    return fail(hipErrorInvalidValue, who + ": widened sums take HICCL_BFLOAT16, HICCL_FLOAT16, HICCL_FLOAT8_E4M3 or "
                                            "HICCL_FLOAT8_E5M2 inputs (in_dtype " + std::to_string(in_dtype) + ")");
  if (acc != HICCL_ACC_NATIVE)
    return fail(hipErrorInvalidValue, who + ": a widened sum always accumulates in f32: leave acc at HICCL_ACC_NATIVE");
  Scale sc{1.0, 1.0f, 0u};  // unscaled: the kernels multiply by one
  if (alpha)
    if (int e = check_scale(in_dtype, *alpha, who, &sc)) return e;
  if (scale) *scale = sc;
  return 0;
}

// hiccl_reduce_op (scale NULL: `op` is a hiccl_op_t the caller has checked),
// hiccl_reduce_scaled (op == kOpScaledSum), hiccl_reduce_widened (op ==
// kOpWidenSum: `dtype` is the inputs', the output is f32) and
// hiccl_reduce_accumulate (op == kOpWidenAccum: the same, and the kernels add
// to the output).  hiccl_reduce_weighted (op == kOpWeightedSum or
// kOpWeightedAccum) is either of the last two with `weights`.
int reduce_call(int dtype, int op, const Scale *scale, void *out, const void *const *in, int n, size_t count,
                void *stream, const hiccl_reduce_config_t *cfg, const float *weights) {
  const bool widened = is_widen_op(op);
  const size_t esz = out_esize(dtype, op);  // of the OUTPUT: the split, the packets and the bytes written are its
  const Scale sc = scale ? *scale : Scale{0.0, 0.0f, 0u};
  if (widened) {
    if (int e = check_buffers_widened(out, in, n, count, esize(dtype), esz)) return e;
    if (is_weighted_op(op))
      if (int e = check_weights(out, weights, n, count, "hiccl_reduce_weighted")) return e;
  }
  if (count == 0) return 0;
  if (dtype == HICCL_BYTES && n != 1) return fail(hipErrorInvalidValue, "hiccl_reduce: HICCL_BYTES copies need n == 1");
  if (!widened) {
    if (int e = check_buffers(out, in, n, count, esz)) return e;
  }
  if (int e = check_cfg(cfg, "hiccl_reduce")) return e;
  hipStream_t s = (hipStream_t)stream;
  const int dev = current_device();
  Split sp = split_on(out, count, esz);
  // engine, shape and store form (write-through by size, as a plan's)
  Cfg c = oneshot_cfg(dtype, op, cfg, sp.npkt, (uint64_t)count * esz, n, dev);
  if (n > kMaxArgInputs) {
    const std::string why = plan_shape_error(c, dtype);
    if (!why.empty()) return fail(hipErrorInvalidValue, "hiccl_reduce_ex: n > 64 inputs run on the plan kernel: " + why);
    // the > 64-input pointer table is uploaded from host memory per call: a
    // captured graph would replay a copy from a freed host buffer
    if (capturing(s, false))
      return fail(hipErrorStreamCaptureUnsupported,
                  "hiccl_reduce: n > 64 inputs cannot be captured into a graph (use a plan)");
    return reduce_via_table(dtype, c, sc, out, in, n, count, s, weights);
  }

  const single_fn fn = is_weighted_op(op) ? nullptr : single_for(dtype, c);
  const single_w_fn wfn =
      is_weighted_op(op) ? pick_single_weighted(dtype, c.acc, c.op, c.engine, c.block, c.unroll, c.pol()) : nullptr;
  if (!fn && !wfn)
    return fail(hipErrorInvalidValue, "hiccl_reduce_ex: unsupported config (block " +
                                          std::to_string(c.block) + ", unroll " +
                                          std::to_string(c.unroll) + ", nt " +
                                          std::to_string(c.nt) + ", store " +
                                          std::to_string(c.store) + ", engine " +
                                          std::to_string(c.engine) + ") for this dtype");

  SingleArgsWeighted a;
  memset(&a, 0, sizeof(a));
  a.weights = weights;
  a.out = (char *)out;
  a.npkt = sp.npkt;
  a.head = sp.head;
  a.tail = sp.tail;
  a.n = (uint32_t)n;
  a.ntiles = tiles_for(sp.npkt, (uint64_t)c.block * c.unroll);
  for (int k = 0; k < n; k++) a.in[k] = (const char *)in[k];
  a.scale = sc;

  LaunchShape L = launch_shape(c, n, a.ntiles, device_cus(dev), /*paced=*/true);
  a.sched = L.dynamic ? ticket_counter(dev, s) : nullptr;
  // no counter for this stream (capture, hipStreamPerThread): the launch runs
  // static and unpaced, on the full grid
  if (L.dynamic && !a.sched) L = launch_shape(c, n, a.ntiles, device_cus(dev));
  a.grab = L.grab;
  a.drain = (uint32_t)c.drain;
  a.order = log2u(c.order);
  if (wfn) wfn(a, dim3((unsigned)L.grid), s);
  else fn(a, dim3((unsigned)L.grid), s);
  return check_hip(hipGetLastError(), "hiccl_reduce: launch");
}

}  // namespace hiccl_impl

namespace {

// hiccl_reduce_auto_choice_op and _scaled, the operator checked by the caller.
int auto_choice(int dtype, int op, const hiccl_reduce_config_t *cfg, size_t count, double n, int cus, int *engine,
                int *unroll, int *blocks_per_cu, int *dynamic, int *store_policy) {
  const size_t esz = out_esize(dtype, op);
  if (cus <= 0 || n < 0) return fail(hipErrorInvalidValue, "auto_choice: cus must be > 0 and n >= 0");
  if (int e = check_cfg(cfg, "auto_choice")) return e;
  CusOverride scoped(cus);  // no device query: the choice for `cus` CUs
  const uint64_t npkt = (uint64_t)count * esz / kPacket;
  const Cfg c = oneshot_cfg(dtype, op, cfg, npkt, (uint64_t)count * esz, n, -1);
  // the same refusals as hiccl_reduce_ex: a shape no kernel has is an error
  const bool has = n > kMaxArgInputs ? plan_shape_error(c, dtype).empty() : has_single(dtype, c);
  if (!has) return fail(hipErrorInvalidValue, "auto_choice: no kernel for this config and dtype");
  const uint64_t units = tiles_for(npkt, (uint64_t)c.block * c.unroll);  // tiles or phased chunks
  const LaunchShape L = launch_shape(c, n, units, cus, /*paced=*/n <= kMaxArgInputs);
  if (engine) *engine = c.engine;
  if (unroll) *unroll = c.unroll;
  if (blocks_per_cu) *blocks_per_cu = c.bpc;
  if (dynamic) *dynamic = L.dynamic ? 1 : 0;
  if (store_policy) *store_policy = c.store + 1;
  return 0;
}

}  // namespace

extern "C" {

int hiccl_reduce_op(int dtype, int op, void *out, const void *const *in, int n, size_t count,
                    void *stream, const hiccl_reduce_config_t *cfg) {
  if (!esize(dtype)) return fail(hipErrorInvalidValue, "hiccl_reduce: unknown dtype " + std::to_string(dtype));
  if (int e = check_op(dtype, cfg ? cfg->acc : HICCL_ACC_NATIVE, op, "hiccl_reduce")) return e;
  return reduce_call(dtype, op, nullptr, out, in, n, count, stream, cfg);
}

int hiccl_reduce_scaled(int dtype, double alpha, void *out, const void *const *in, int n, size_t count,
                        void *stream, const hiccl_reduce_config_t *cfg) {
  Scale sc;
  if (int e = check_scale(dtype, alpha, "hiccl_reduce_scaled", &sc)) return e;
  return reduce_call(dtype, kOpScaledSum, &sc, out, in, n, count, stream, cfg);
}

int hiccl_reduce_widened(int in_dtype, int out_dtype, const double *alpha, void *out, const void *const *in, int n,
                         size_t count, void *stream, const hiccl_reduce_config_t *cfg) {
  Scale sc;
  if (int e = check_widened(in_dtype, out_dtype, cfg ? cfg->acc : HICCL_ACC_NATIVE, alpha, "hiccl_reduce_widened", &sc))
    return e;
  return reduce_call(in_dtype, kOpWidenSum, &sc, out, in, n, count, stream, cfg);
}

int hiccl_reduce_accumulate(int in_dtype, int out_dtype, const double *alpha, void *out, const void *const *in, int n,
                            size_t count, void *stream, const hiccl_reduce_config_t *cfg) {
  Scale sc;
  if (int e = check_widened(in_dtype, out_dtype, cfg ? cfg->acc : HICCL_ACC_NATIVE, alpha, "hiccl_reduce_accumulate", &sc))
    return e;
  return reduce_call(in_dtype, kOpWidenAccum, &sc, out, in, n, count, stream, cfg);
}

int hiccl_reduce_auto_choice_accumulate(int in_dtype, const hiccl_reduce_config_t *cfg, size_t count, double n, int cus,
                                        int *engine, int *unroll, int *blocks_per_cu, int *dynamic, int *store_policy) {
  if (int e = check_widened(in_dtype, HICCL_FLOAT32, cfg ? cfg->acc : HICCL_ACC_NATIVE, nullptr,
                            "auto_choice_accumulate", nullptr))
    return e;
  return auto_choice(in_dtype, kOpWidenAccum, cfg, count, n, cus, engine, unroll, blocks_per_cu, dynamic, store_policy);
}

int hiccl_reduce_weighted(int in_dtype, int out_dtype, const double *alpha, int accumulate, void *out,
                          const void *const *in, const float *weights, int n, size_t count, void *stream,
                          const hiccl_reduce_config_t *cfg) {
  Scale sc;
  if (int e = check_widened(in_dtype, out_dtype, cfg ? cfg->acc : HICCL_ACC_NATIVE, alpha, "hiccl_reduce_weighted", &sc))
    return e;
  return reduce_call(in_dtype, accumulate ? kOpWeightedAccum : kOpWeightedSum, &sc, out, in, n, count, stream, cfg,
                     weights);
}

int hiccl_reduce_auto_choice_weighted(int in_dtype, int accumulate, const hiccl_reduce_config_t *cfg, size_t count,
                                      double n, int cus, int *engine, int *unroll, int *blocks_per_cu, int *dynamic,
                                      int *store_policy) {
  if (int e = check_widened(in_dtype, HICCL_FLOAT32, cfg ? cfg->acc : HICCL_ACC_NATIVE, nullptr,
                            "auto_choice_weighted", nullptr))
    return e;
  return auto_choice(in_dtype, accumulate ? kOpWeightedAccum : kOpWeightedSum, cfg, count, n, cus, engine, unroll,
                     blocks_per_cu, dynamic, store_policy);
}

int hiccl_reduce_auto_choice_widened(int in_dtype, const hiccl_reduce_config_t *cfg, size_t count, double n, int cus,
                                     int *engine, int *unroll, int *blocks_per_cu, int *dynamic, int *store_policy) {
  if (int e = check_widened(in_dtype, HICCL_FLOAT32, cfg ? cfg->acc : HICCL_ACC_NATIVE, nullptr, "auto_choice_widened",
                            nullptr))
    return e;
  return auto_choice(in_dtype, kOpWidenSum, cfg, count, n, cus, engine, unroll, blocks_per_cu, dynamic, store_policy);
}

int hiccl_reduce_ex(int dtype, void *out, const void *const *in, int n, size_t count,
                    void *stream, const hiccl_reduce_config_t *cfg) {
  return hiccl_reduce_op(dtype, HICCL_OP_SUM, out, in, n, count, stream, cfg);
}

int hiccl_reduce(int dtype, void *out, const void *const *in, int n, size_t count, void *stream) {
  return hiccl_reduce_ex(dtype, out, in, n, count, stream, nullptr);
}

int hiccl_reduce_f32(float *out, const float *const *in, int n, size_t count, void *stream) {
  return hiccl_reduce_ex(HICCL_FLOAT32, out, (const void *const *)in, n, count, stream, nullptr);
}

int hiccl_reduce_bf16(uint16_t *out, const uint16_t *const *in, int n, size_t count,
                      void *stream) {
  return hiccl_reduce_ex(HICCL_BFLOAT16, out, (const void *const *)in, n, count, stream, nullptr);
}

int hiccl_reduce_f16(uint16_t *out, const uint16_t *const *in, int n, size_t count,
                     void *stream) {
  return hiccl_reduce_ex(HICCL_FLOAT16, out, (const void *const *)in, n, count, stream, nullptr);
}

int hiccl_reduce_auto_choice_op(int dtype, int op, const hiccl_reduce_config_t *cfg, size_t count, double n, int cus,
                                int *engine, int *unroll, int *blocks_per_cu, int *dynamic, int *store_policy) {
  const size_t esz = esize(dtype);
  if (!esz) return fail(hipErrorInvalidValue, "auto_choice: unknown dtype");
  if (int e = check_op(dtype, cfg ? cfg->acc : HICCL_ACC_NATIVE, op, "auto_choice")) return e;
  return auto_choice(dtype, op, cfg, count, n, cus, engine, unroll, blocks_per_cu, dynamic, store_policy);
}

int hiccl_reduce_auto_choice_scaled(int dtype, const hiccl_reduce_config_t *cfg, size_t count, double n, int cus,
                                    int *engine, int *unroll, int *blocks_per_cu, int *dynamic, int *store_policy) {
  if (int e = check_scale(dtype, 1.0, "auto_choice_scaled", nullptr)) return e;
  return auto_choice(dtype, kOpScaledSum, cfg, count, n, cus, engine, unroll, blocks_per_cu, dynamic, store_policy);
}

int hiccl_reduce_auto_choice_ex(int dtype, const hiccl_reduce_config_t *cfg, size_t count, double n, int cus,
                                int *engine, int *unroll, int *blocks_per_cu, int *dynamic, int *store_policy) {
  return hiccl_reduce_auto_choice_op(dtype, HICCL_OP_SUM, cfg, count, n, cus, engine, unroll, blocks_per_cu, dynamic,
                                     store_policy);
}

int hiccl_reduce_auto_choice(int dtype, int acc, size_t count, double n, int cus, int *engine, int *unroll,
                             int *blocks_per_cu, int *dynamic) {
  hiccl_reduce_config_t z;
  memset(&z, 0, sizeof(z));
  z.acc = acc;
  return hiccl_reduce_auto_choice_ex(dtype, &z, count, n, cus, engine, unroll, blocks_per_cu, dynamic, nullptr);
}

}  // extern "C"
