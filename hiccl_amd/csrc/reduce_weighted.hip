// hiccl_amd/csrc/reduce_weighted.hip -- the kernels of the weighted widened
// sums (out = sum of w[k] * x[k], bf16, f16, e4m3 or e5m2 inputs, one f32
// weight per input read from device memory, the output f32, overwritten or
// accumulated into; hiccl_reduce_weighted, hiccl_reduce_plan_set_weighted):
// engine.h's k_reduce_single_weighted and k_reduce_plan_weighted instantiated
// for OpWeighted and OpWeightedAccum over the four widenings, in every engine's
// default shape (no tuning table, no program kernel).
// Not a translation unit of its own: reduce_scale.hip, the unit linked last,
// includes it behind reduce_mixed.hip (see there), so the code objects of the
// other three units stay as they are and the library's count of them does not
// change.
#include "engine.h"

namespace hiccl_impl {

single_w_fn pick_single_weighted(int dtype, int acc, int op, int engine, int block, int unroll, int pol) {
  return with_elem_weighted(dtype, acc, op, (single_w_fn) nullptr, [&](auto e) {
    return pick_single_weighted_op<typename decltype(e)::Op>(engine, block, unroll, pol);
  });
}

plan_w_fn pick_plan_weighted(int dtype, int acc, int op, int engine, int unroll, int pol) {
  return with_elem_weighted(dtype, acc, op, (plan_w_fn) nullptr, [&](auto e) {
    return pick_plan_weighted_eng<typename decltype(e)::Op>(engine, unroll, pol);
  });
}

int phase_p_weighted(int dtype, int op) {
  return with_elem_weighted(dtype, HICCL_ACC_NATIVE, op, 16, [](auto e) { return phase_p_of<typename decltype(e)::Op>(); });
}

}  // namespace hiccl_impl
