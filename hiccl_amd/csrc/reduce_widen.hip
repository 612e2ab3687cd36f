// hiccl_amd/csrc/reduce_widen.hip -- the kernels of the widened sums (bf16,
// f16, e4m3 or e5m2 inputs summed into an f32 output; hiccl_reduce_widened,
// hiccl_reduce_plan_set_out_dtype): engine.h's scaled one-shot and plan kernels
// instantiated for OpBF16ToF32, OpF16ToF32 and OpF8ToF32 (both formats), in
// every engine's default shape (no tuning table, no program kernel).  The
// plain form runs the same kernels with alpha = 1.
// Not a translation unit of its own: reduce_scale.hip, the unit linked last,
// includes it behind reduce_f8.hip (see there), so the code objects of the
// other three units stay as they are and the library's count of them does not
// change.
#include "engine.h"

namespace hiccl_impl {

single_fn pick_single_widen(int dtype, int acc, int op, int engine, int block, int unroll, int pol) {
  return part_single<kPartWiden>(dtype, acc, op, engine, block, unroll, pol);
}

plan_fn pick_plan_widen(int dtype, int acc, int op, int engine, int unroll, int pol) {
  return part_plan<kPartWiden>(dtype, acc, op, engine, unroll, pol);
}

}  // namespace hiccl_impl
