// hiccl_amd/csrc/policy.h -- the launch policy: a caller's config resolved
// into engine, shape, store form, grid and schedule.  Pure functions of
// their arguments plus device_cus(); the rules and thresholds: policy.cpp.
#pragma once

#include <string>

#include "runtime.h"

namespace hiccl_impl __attribute__((visibility("hidden"))) {

struct Cfg {
  int block, unroll, bpc, nt, acc, grid, store, engine, schedule, grab, drain;
  bool store_auto;  // store_policy 0: the store form follows the launch's size (wt_by_size)
  bool wt;          // the launch stores write-through by size: decided BEFORE the engine
                    // (oneshot_cfg, plan_cfg), since AUTO's engine rules differ under it
  int order;        // tile-order segments (hiccl_reduce_config_t.order; 0/1 linear)
  int op;           // hiccl_op_t, kOpWidenSum / kOpWidenAccum, kOpWeightedSum / kOpWeightedAccum, or kOpScaledSum (a scaled sum: untuned, like every operator but
                    // SUM, and honours acc): not a config entry -- the call or the plan names it
                    // (resolve: SUM)
  int pol() const { return store * 10 + nt; }
};

// Raw config: zero block/unroll stay zero until the engine is known.
Cfg resolve(const hiccl_reduce_config_t *c);

// The enumerated and ranged fields of a caller's config (NULL: all
// defaults), refused as `who: ...` with hipErrorInvalidValue.
int check_cfg(const hiccl_reduce_config_t *c, const std::string &who);
// Is `op` one of hiccl_op_t's values (which are not a range)?
bool known_op(int op);
// An operator for this dtype and accumulation mode: known, SUM for
// HICCL_BYTES and HICCL_ACC_WIDE, and an integer type under the bitwise
// operators.  Refused as `who: ...` likewise.
int check_op(int dtype, int acc, int op, const std::string &who);

// A scaled sum's dtype (floating) and alpha (finite; as a float too for the 4-
// and 2-byte types), refused as `who: ...` likewise; *scale (may be NULL): the
// kernels' argument.
int check_scale(int dtype, double alpha, const std::string &who, Scale *scale);
// A widened sum's dtypes (hiccl_reduce_widened: bf16, f16 or FP8 in, f32 out),
// its accumulation mode (native: the accumulator is f32 as it is) and alpha
// (NULL: unscaled, the kernels then multiply by 1), refused as `who: ...`
// likewise; *scale (may be NULL): the kernels' argument.
bool widen_in_dtype(int dtype);
int check_widened(int in_dtype, int out_dtype, int acc, const double *alpha, const std::string &who, Scale *scale);
// Bytes per element a call writes: 4 for a widened sum (accumulating or not),
// else the dtype's.
inline size_t out_esize(int dtype, int op) { return is_widen_op(op) ? 4 : esize(dtype); }
// The one-shot call behind hiccl_reduce_op (scale NULL, `op` checked by the
// caller), hiccl_reduce_scaled (op kOpScaledSum) and hiccl_reduce_widened (op
// kOpWidenSum, dtype the inputs', scale never NULL) and hiccl_reduce_accumulate
// (op kOpWidenAccum, likewise) and hiccl_reduce_weighted (kOpWeightedSum /
// kOpWeightedAccum, likewise, with `weights` -- n floats in device memory, which
// every other op leaves NULL): oneshot.cpp.
int reduce_call(int dtype, int op, const Scale *scale, void *out, const void *const *in, int n, size_t count,
                void *stream, const hiccl_reduce_config_t *cfg, const float *weights = nullptr);
// The weights of a weighted sum (n > 0: not NULL, 4-byte aligned, not
// overlapping the count f32 outputs), refused as `who: ...` with
// hipErrorInvalidValue before any device work.
int check_weights(const void *out, const float *weights, int n, size_t count, const std::string &who);

// Does a launch that writes `out_bytes` from `n` inputs per output (a plan's
// packet-weighted mean) store write-through BY SIZE under the raw config?
bool wt_by_size(const Cfg &raw, int dtype, double n, uint64_t out_bytes);
// Write-through (and peer-policy) TILE launches run at these unrolls.
inline bool wt_unroll(int unroll) { return unroll == 2 || unroll == kDefUnroll; }

// Fill in the engine and its default shape (n: inputs, or a plan's
// packet-weighted mean).
void finish_cfg(Cfg &c, uint64_t npkt, double n, int dtype, int dev);

// The one-shot call's configuration, engine and store form resolved.
Cfg oneshot_cfg(int dtype, int op, const hiccl_reduce_config_t *cfg, uint64_t npkt, uint64_t out_bytes, double n,
                int dev);
// Its kernel (n <= kMaxArgInputs), or NULL.
inline single_fn single_for(int dtype, const Cfg &c) {
  return pick_single(dtype, c.acc, c.op, c.engine, c.block, c.unroll, c.pol());
}
// Is there one?  (A weighted op's kernels have a launcher type of their own.)
inline bool has_single(int dtype, const Cfg &c) {
  if (is_weighted_op(c.op)) return pick_single_weighted(dtype, c.acc, c.op, c.engine, c.block, c.unroll, c.pol()) != nullptr;
  return single_for(dtype, c) != nullptr;
}
// Likewise of the plan kernels.
inline bool has_plan(int dtype, int acc, int op, int engine, int unroll, int pol) {
  if (is_weighted_op(op)) return pick_plan_weighted(dtype, acc, op, engine, unroll, pol) != nullptr;
  return pick_plan(dtype, acc, op, engine, unroll, pol) != nullptr;
}

// The plan kernels' cache policy: nt loads and stores, or a plan's peer
// policy (HICCL_PEER_* flags: system-scope stores and/or loads).
int plan_pol(int peer);
// Packets per work unit (tile or chunk) of a plan kernel.
uint64_t unit_pkts(int engine, int dtype, int acc, int unroll, int op);
// Is `c` (engine resolved, shape filled in by finish_cfg) a shape the plan
// kernels have?  Empty string if so, else why not.
std::string plan_shape_error(const Cfg &c, int dtype);

// The shape of one launch of `units` work units of `n` inputs (mean) on a
// device of `cus` CUs: workgroups, units per ticket, and whether the units
// are handed out by a ticket counter (dynamic) or grid-stride.
struct LaunchShape {
  uint64_t grid;
  uint32_t grab;
  bool dynamic;
};
// `paced`: a launch of the one-shot kernel (its dynamic tiles pace their loads
// and take 7/8 of the default grid).
LaunchShape launch_shape(const Cfg &c, double n, uint64_t units, int cus, bool paced = false);

}  // namespace hiccl_impl
