// hiccl_amd/csrc/reduce_mixed.hip -- the mixed plan kernels (kOpMixedSum):
// engine.h's k_reduce_plan_mixed instantiated for the ten scaled ops --
// f32, f64, bf16 and f16 native and wide, e4m3 and e5m2 native and wide -- in
// either engine's default shape under the four plan policies (no tuning
// table).  A scaled plan whose computes are partly unscaled
// (hiccl_reduce_plan_add_unscaled) launches them: scaled per compute.
// Not a translation unit of its own: reduce_scale.hip, the unit linked last,
// includes it behind reduce_accum.hip (see there).
#include "engine.h"

namespace hiccl_impl {

plan_fn pick_plan_mixed(int dtype, int acc, int op, int engine, int unroll, int pol) {
  return with_elem<kPartMixed>(dtype, acc, op, (plan_fn) nullptr, [&](auto e) {
    return pick_plan_mixed_eng<typename decltype(e)::Op>(engine, unroll, pol);
  });
}

}  // namespace hiccl_impl
