// hiccl_amd/csrc/reduce_f8.hip -- the kernels of the two OCP FP8 types
// (HICCL_FLOAT8_E4M3, HICCL_FLOAT8_E5M2): engine.h's one-shot, plan and
// program kernels instantiated for OpF8 (native SUM), OpF8Wide
// (HICCL_ACC_WIDE), OpF8MM (MAX / MIN) and OpF8Scaled (the scaled sums, under
// either accumulator), in every engine's default shape (no tuning table).
// Not a translation unit of its own: reduce_scale.hip, the unit linked last,
// includes it (see there), so the code objects of the other three units stay
// as they are and the library's count of them does not change.
#include "engine.h"

namespace hiccl_impl {

single_fn pick_single_f8(int dtype, int acc, int op, int engine, int block, int unroll, int pol) {
  return part_single<kPartF8>(dtype, acc, op, engine, block, unroll, pol);
}

plan_fn pick_plan_f8(int dtype, int acc, int op, int engine, int unroll, int pol) {
  return part_plan<kPartF8>(dtype, acc, op, engine, unroll, pol);
}

prog_fn pick_prog_f8(int dtype, int op, int unroll) {
  // no program runs a scaled plan (hiccl_program_add_plan)
  return op == kOpScaledSum ? nullptr : part_prog<kPartF8>(dtype, op, unroll);
}

}  // namespace hiccl_impl
