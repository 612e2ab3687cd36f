// hiccl_amd/csrc/reduce_scale.hip -- the scaled-sum kernels (out = alpha *
// sum): engine.h's one-shot and plan kernels instantiated for the six ops
// OpF32Scaled ... OpF16WideScaled (f32, f64, bf16 and f16, the 2-byte types
// under either accumulator), in every engine's default shape (no tuning
// table).  A translation unit of its own, linked last, so that it compiles
// next to the other three and their code objects stay as they are.
//
// The kernels of the two OCP FP8 types (reduce_f8.hip) are compiled into this
// unit too, behind the scaled sums': the library stays at four code objects
// with this one last, which the ISA tier of the scaled sums relies on.  The
// widened sums' kernels (reduce_widen.hip) follow them, for the same reason,
// and the accumulating widened sums' (reduce_accum.hip) follow those, and the
// mixed plan kernels (reduce_mixed.hip) follow those, and the weighted widened
// sums' (reduce_weighted.hip) come last.
#include "engine.h"

namespace hiccl_impl {

single_fn pick_single_scale(int dtype, int acc, int op, int engine, int block, int unroll, int pol) {
  return part_single<kPartScale>(dtype, acc, op, engine, block, unroll, pol);
}

plan_fn pick_plan_scale(int dtype, int acc, int op, int engine, int unroll, int pol) {
  return part_plan<kPartScale>(dtype, acc, op, engine, unroll, pol);
}

}  // namespace hiccl_impl

#include "reduce_f8.hip"
#include "reduce_widen.hip"
#include "reduce_accum.hip"
#include "reduce_mixed.hip"
#include "reduce_weighted.hip"
