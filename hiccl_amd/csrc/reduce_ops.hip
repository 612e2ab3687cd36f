// hiccl_amd/csrc/reduce_ops.hip -- the MAX and MIN kernels: engine.h's one-shot,
// plan and program kernels instantiated for the twelve ops OpF32MM<MAX> ...
// OpU64MM<MIN>, in every engine's default shape (no tuning table).  A
// translation unit of its own so that it compiles next to reduce.hip.
#include "engine.h"

namespace hiccl_impl {

single_fn pick_single_maxmin(int dtype, int acc, int op, int engine, int block, int unroll, int pol) {
  return part_single<kPartMaxMin>(dtype, acc, op, engine, block, unroll, pol);
}

plan_fn pick_plan_maxmin(int dtype, int acc, int op, int engine, int unroll, int pol) {
  return part_plan<kPartMaxMin>(dtype, acc, op, engine, unroll, pol);
}

prog_fn pick_prog_maxmin(int dtype, int op, int unroll) { return part_prog<kPartMaxMin>(dtype, op, unroll); }

}  // namespace hiccl_impl
