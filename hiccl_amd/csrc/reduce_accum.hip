// hiccl_amd/csrc/reduce_accum.hip -- the kernels of the accumulating widened
// sums (out = out + alpha * sum of bf16, f16, e4m3 or e5m2 inputs, the output
// f32; hiccl_reduce_accumulate, hiccl_reduce_plan_set_accumulate): engine.h's
// scaled one-shot and plan kernels instantiated for OpBF16AccF32, OpF16AccF32
// and OpF8AccF32 (both formats), in every engine's default shape (no tuning
// table, no program kernel).  The plain form runs the same kernels with
// alpha = 1.
// Not a translation unit of its own: reduce_scale.hip, the unit linked last,
// includes it behind reduce_widen.hip (see there), so the code objects of the
// other three units stay as they are and the library's count of them does not
// change.
#include "engine.h"

namespace hiccl_impl {

single_fn pick_single_accum(int dtype, int acc, int op, int engine, int block, int unroll, int pol) {
  return part_single<kPartAccum>(dtype, acc, op, engine, block, unroll, pol);
}

plan_fn pick_plan_accum(int dtype, int acc, int op, int engine, int unroll, int pol) {
  return part_plan<kPartAccum>(dtype, acc, op, engine, unroll, pol);
}

}  // namespace hiccl_impl
