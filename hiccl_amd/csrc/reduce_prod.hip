// hiccl_amd/csrc/reduce_prod.hip -- the PROD and bitwise kernels: engine.h's
// one-shot, plan and program kernels instantiated for the twelve ops
// OpF32Prod ... OpU64Fold<kIntXor> (PROD of the six arithmetic types; BAND,
// BOR, BXOR of int32 and uint64), in every engine's default shape (no tuning
// table).  A translation unit of its own so that it compiles next to
// reduce.hip and reduce_ops.hip.
#include "engine.h"

namespace hiccl_impl {

single_fn pick_single_prod(int dtype, int acc, int op, int engine, int block, int unroll, int pol) {
  return part_single<kPartProd>(dtype, acc, op, engine, block, unroll, pol);
}

plan_fn pick_plan_prod(int dtype, int acc, int op, int engine, int unroll, int pol) {
  return part_plan<kPartProd>(dtype, acc, op, engine, unroll, pol);
}

prog_fn pick_prog_prod(int dtype, int op, int unroll) { return part_prog<kPartProd>(dtype, op, unroll); }

}  // namespace hiccl_impl
