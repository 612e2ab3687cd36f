// hiccl_amd/csrc/plan.h -- batched plans (plan.cpp) as the other host files
// see them: the plan object, the descriptor-table builder, one plan-kernel
// launch.
#pragma once

#include <atomic>
#include <vector>

#include "policy.h"

struct hiccl_reduce_plan {
  int dtype = 0;
  int device = 0;
  int op = HICCL_OP_SUM;          // hiccl_reduce_plan_set_op
  bool scaled = false;            // hiccl_reduce_plan_set_scale: out = alpha * sum (op stays SUM)
  hiccl_impl::Scale scale{0.0, 0.0f, 0u};
  bool widened = false;           // hiccl_reduce_plan_set_out_dtype: dtype inputs, f32 outputs (op stays SUM)
  // the operator the policy and the kernel tables see
  bool accumulate = false;        // hiccl_reduce_plan_set_accumulate: out += (alpha *) sum, on a widened plan only
  bool weighted = false;          // hiccl_reduce_plan_set_weighted: every compute brings n f32 weights in device memory
  // A scaled plan's family follows its computes: all scaled -- the scaled
  // kernels; all unscaled (hiccl_reduce_plan_add_unscaled) -- the plain SUM
  // kernels, tuned table included; both kinds -- the mixed kernels.
  int kernel_op() const {
    if (weighted) return accumulate ? hiccl_impl::kOpWeightedAccum : hiccl_impl::kOpWeightedSum;
    if (widened) return accumulate ? hiccl_impl::kOpWidenAccum : hiccl_impl::kOpWidenSum;
    if (!scaled || num_unscaled == comps.size()) return op;
    return num_unscaled ? hiccl_impl::kOpMixedSum : hiccl_impl::kOpScaledSum;
  }
  // the operator a config is validated for: the scaled kernels' shapes are the
  // mixed ones' and a subset of the plain sums', whatever computes come later
  int config_op() const { return !widened && scaled ? hiccl_impl::kOpScaledSum : kernel_op(); }
  // the scale a launch carries: a widened plan's kernels always multiply (by one if unscaled)
  hiccl_impl::Scale kernel_scale() const { return widened && !scaled ? hiccl_impl::Scale{1.0, 1.0f, 0u} : scale; }
  bool has_scale() const { return scaled || widened; }
  hiccl_reduce_config_t req;      // hiccl_reduce_plan_set_config / _set_engine / _set_acc (0 = default)
  int engine = HICCL_ENGINE_TILE;  // resolved at upload
  int unroll = hiccl_impl::kDefUnroll;  // TILE packets per lane, resolved at upload
  double mean_n = 0;               // packet-weighted inputs per compute
  int bpc = 1;                     // workgroups per CU, resolved at upload
  int peer = 0;                    // hiccl_reduce_plan_set_peer flags
  int eff_peer = 0;                // peer | the store form plan_store_peer picks, resolved at upload
  size_t esz = 0;                  // bytes per input element
  size_t osz = 0;                  // bytes per output element: esz, or 4 on a widened plan
  struct Comp {
    void *out;
    std::vector<const void *> in;
    size_t count;
    bool unscaled = false;  // hiccl_reduce_plan_add_unscaled: the plain sum, whatever the plan's scale
    const float *weights = nullptr;  // hiccl_reduce_plan_add_weighted: the caller's n floats, passed along
  };
  std::vector<Comp> comps;
  size_t num_unscaled = 0;  // computes with the flag
  bool dirty = true;
  char *d_block = nullptr;  // the uploaded DescTable
  hiccl_impl::PlanArgs args;  // pointers into d_block
  const float *const *d_weights = nullptr;  // a weighted plan: one weight pointer per compute, behind the table in d_block
  hipStream_t own = nullptr;
  hipStream_t last = nullptr;  // stream of the last launch (plan_sync synchronises it)
  bool launched = false;
  std::atomic<bool> enqueued{false};  // some launch went out (on a stream not remembered)
};

namespace hiccl_impl __attribute__((visibility("hidden"))) {

// The plan's peer flags with the store form its launches take (write-through
// on request or by size: wt_by_size) as HICCL_PEER_STORES.
int plan_eff_peer(const hiccl_reduce_plan *p);

// Host image of the descriptor table a plan or program kernel reads,
// [desc | ptrs | unit_comp] (PlanArgs), the pieces 8-B aligned: add the
// computes, then take the image.  A table of one compute has no unit_comp
// piece (the kernels take NULL: every unit is compute 0's).
struct DescTable {
  size_t stride;  // pointer slots per compute: the largest n of the computes to come (>= 1)
  uint64_t unit;  // packets per work unit
  std::vector<PlanDesc> desc;
  std::vector<const void *> ptrs;
  uint64_t units = 0;

  DescTable(size_t stride_, uint64_t unit_) : stride(stride_ ? stride_ : 1), unit(unit_) {}
  // One compute; `flags` goes to PlanDesc.pad (k_program: byte copy, peer
  // policy; k_reduce_plan_mixed: kDescUnscaled).
  void add(void *out, const void *const *in, size_t n, size_t count, size_t esz, uint32_t flags = 0);

  size_t ptrs_off() const { return desc.size() * sizeof(PlanDesc); }
  size_t unit_comp_off() const { return ptrs_off() + ptrs.size() * sizeof(void *); }
  // end of the table: where a program appends its phase and flag arrays
  size_t bytes() const {
    return unit_comp_off() + (desc.size() > 1 ? ((size_t)units * sizeof(uint32_t) + 7) & ~(size_t)7 : 0);
  }
  // The image, `extra` zero bytes appended.
  std::vector<char> image(size_t extra = 0) const;
  // Point a kernel's arguments at the image uploaded to `dev`.
  template <class Args>
  void bind(Args &a, const char *dev) const {
    a.desc = (const PlanDesc *)dev;
    a.ptrs = (const char *const *)(dev + ptrs_off());
    a.unit_comp = desc.size() > 1 ? (const uint32_t *)(dev + unit_comp_off()) : nullptr;
    a.stride = (uint32_t)stride;
  }
};

// One plan-kernel launch of `a` (desc, ptrs, unit_comp, units, stride set),
// shaped by `c` (engine and shape resolved), in cache policy `pol`.
// (a.scale: the scale of a scaled sum, c.op == kOpScaledSum).
// (a.weights: the weight pointers of a weighted sum, which runs the kernels of pick_plan_weighted).
int launch_plan(PlanArgsWeighted a, int dtype, const Cfg &c, double mean_n, int dev, hipStream_t s, int pol);

// Before a device block is freed: no launch may still read it.  True if some
// launch went out on a stream nobody remembered -- the device was synchronised.
bool sync_if_enqueued(std::atomic<bool> &enqueued);

}  // namespace hiccl_impl
