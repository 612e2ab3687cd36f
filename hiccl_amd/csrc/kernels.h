// hiccl_amd/csrc/kernels.h -- all the host files see of the gfx950 kernels
// (reduce.hip): the kernels' argument structs, the constants both sides need,
// the kernel-table lookups and the launch wrappers of the plain kernels.
#pragma once

#include <hip/hip_runtime_api.h>

#include <stddef.h>
#include <stdint.h>

// Library-internal: nothing in here is exported from libhiccl_reduce.so.
namespace hiccl_impl __attribute__((visibility("hidden"))) {

constexpr int kPacket = 16;  // bytes per lane per load

// Cache policy, POL = 10*store + load.  load: 0 default, 1 nt (aux bit 1),
// 2 system scope (sc0 sc1: coherent with a peer GPU's writes -- the
// reading XCD's L2 does not serve a line of peer memory it cached earlier).
// store: 0 default, 1 nt, 2 sc1 (aux bit 4: write-through, line dropped
// from the XCD L2), 3 system scope (sc0 sc1: written through to the memory
// that owns the line, a peer GPU's HBM over xGMI included -- nt stores are
// not write-through and may sit dirty in this XCD's L2 after the kernel).
// The system-scope forms are the PEER policies of plans whose outputs or
// inputs live in another GPU's memory (hiccl_reduce_plan_set_peer).
constexpr int kPolLoadSys = 2;
constexpr int kPolStoreSys = 3;
constexpr int kDefPol = 11;  // nt loads, nt stores

// Engine shapes, chosen from on-device sweeps:
//  tile   256 lanes x 4 packets (16 KiB per input per tile), for computes too
//         small to give every CU several phased chunks;
//  phase  512 lanes x P packets (P = phase_p: 16, or 8 where the accumulator
//         of a packet takes 8 VGPRs -- bf16 / f16 WIDE -- or the adds get
//         reassociated: int32 -- or the old output's packets are held next
//         to the accumulators: kOpWidenAccum) -- 128 KiB per input per chunk
//         (64 KiB at P = 8).
// Both: nt loads and nt stores, one workgroup per CU, grid-stride.  Plan
// kernels run the TILE engine at kDefBlock lanes only.
constexpr int kDefBlock = 256;
constexpr int kDefUnroll = 4;
constexpr int kPhBlock = 512;

constexpr int kMaxArgInputs = 64;  // kernarg pointer table (512 B)

// A scaled sum (hiccl_reduce_scaled, hiccl_reduce_plan_set_scale) travels
// through the policy and the kernel tables as an operator of its own, which is
// no hiccl_op_t value: the public entries never take it (known_op refuses it).
constexpr int kOpScaledSum = 0x100;
// A widened sum (hiccl_reduce_widened, hiccl_reduce_plan_set_out_dtype: bf16,
// f16 or FP8 inputs, f32 output) likewise.  The dtype that travels with it is
// the INPUTS'; every packet count is in packets of the f32 OUTPUT (four
// elements).  Its kernels are the scaled ones' kind (they take a Scale): an
// unscaled widened sum passes alpha = 1.
constexpr int kOpWidenSum = 0x101;
// An accumulating widened sum (hiccl_reduce_accumulate,
// hiccl_reduce_plan_set_accumulate): a widened sum whose kernels read the old
// f32 output and add the (scaled) sum to it.  Everything said of kOpWidenSum
// holds; is_widen_op answers for both.
constexpr int kOpWidenAccum = 0x102;
// A weighted widened sum (hiccl_reduce_weighted, hiccl_reduce_plan_set_weighted):
// a widened sum, or an accumulating one, whose inputs each count with an f32
// weight read from device memory when the kernel runs.  Everything said of
// kOpWidenSum / kOpWidenAccum holds and is_widen_op answers for them too; their
// kernels take the weights behind the scaled kernels' arguments
// (SingleArgsWeighted, PlanArgsWeighted) and have launcher types of their own.
constexpr int kOpWeightedSum = 0x104;
constexpr int kOpWeightedAccum = 0x105;
constexpr bool is_weighted_op(int op) { return op == kOpWeightedSum || op == kOpWeightedAccum; }
constexpr bool is_widen_op(int op) { return op == kOpWidenSum || op == kOpWidenAccum || is_weighted_op(op); }
// does the op read the old output (the accumulating families)?
constexpr bool is_accum_op(int op) { return op == kOpWidenAccum || op == kOpWeightedAccum; }
// the unweighted family an op belongs to: its thresholds, its bytes, its PHASE chunk unless phase_p says otherwise
constexpr int unweighted_op(int op) {
  return op == kOpWeightedSum ? kOpWidenSum : op == kOpWeightedAccum ? kOpWidenAccum : op;
}
// A scaled plan in which some computes, not all, write the plain sum
// (hiccl_reduce_plan_add_unscaled: the intermediate computes of an averaging
// Comm<T> step): the MIXED plan kernels, which read the choice per compute from
// PlanDesc.pad (kDescUnscaled).  Plan kernels only; the policy takes it for
// kOpScaledSum.  No public entry takes it either.
constexpr int kOpMixedSum = 0x103;
// PlanDesc.pad bit 3: this compute of a mixed launch is not scaled (bits 0-2
// are the step programs': byte copy, peer flags)
constexpr uint32_t kDescUnscaled = 8u;

// The scale of a scaled sum: alpha as the caller gave it (f64 kernels) and
// rounded to nearest even to f32 (every other type).  The scaled kernels take
// it behind the arguments of the unscaled ones (SingleArgsScaled,
// PlanArgsScaled), whose own argument structs stay as they are.
struct Scale {
  double a64;
  float a32;
  uint32_t pad;
};

struct SingleArgs {
  char *out;          // raw output pointer
  uint64_t npkt;      // body packets
  uint64_t ntiles;    // >= 1
  uint32_t n;         // inputs
  uint32_t head;      // scalar elements before the body
  uint32_t tail;      // scalar elements after the body
  uint32_t order;     // log2 of the tile-order segments (0: linear; tile_order)
  uint32_t *sched;    // dynamic unit counter {ticket, done}, or NULL: static grid-stride
  uint32_t grab;      // units per ticket (dynamic schedule), >= 1
  uint32_t drain;     // 1: wait for a unit's stores before the next unit's loads
  const char *in[kMaxArgInputs];
};

// What the host hands a one-shot launcher: the kernel's arguments, and the
// scale, which only a scaled kernel (k_reduce_single_scaled) is passed.
struct SingleArgsScaled : SingleArgs {
  Scale scale;
};

// Descriptor of one compute in a batched plan (device memory).
struct PlanDesc {
  char *out;
  uint64_t npkt;
  uint64_t tile_begin;  // first global unit of this compute
  uint32_t n, head, tail, pad;
};
static_assert(sizeof(PlanDesc) == 40, "PlanDesc layout");

// A plan launch.  One device block holds [desc | ptrs | unit_comp]:
//   desc[c]                  compute c
//   ptrs[c * stride + k]     input k of compute c (stride = the plan's max n)
//   unit_comp[t]             the compute owning global unit t (NULL: compute 0)
// so a workgroup reaches a unit's input pointers in two dependent scalar
// loads: unit_comp[t], then desc[c] and ptrs[c * stride ...] side by side.
struct PlanArgs {
  const PlanDesc *desc;
  const char *const *ptrs;
  const uint32_t *unit_comp;
  uint64_t t_begin, t_end;
  uint32_t *sched;  // dynamic unit counter, or NULL
  uint32_t stride, grab;
};

struct PlanArgsScaled : PlanArgs {  // as SingleArgsScaled
  Scale scale;
};

// The weighted sums' kernels (k_reduce_single_weighted, k_reduce_plan_weighted)
// take the weights behind the scaled kernels' arguments, whose own structs stay
// as they are: n consecutive floats in device memory for a one-shot call (the
// caller's pointer), one such pointer per compute for a plan (a device table
// behind the plan's descriptor table).
struct SingleArgsWeighted : SingleArgsScaled {
  const float *weights;
};

struct PlanArgsWeighted : PlanArgsScaled {
  const float *const *weights;  // weights[c]: compute c's n floats
};

constexpr int kMaxFlags = 64;  // signal and wait flags per launch (one per lane)

// Several signal/wait phases in ONE launch, executed in order: phase p
// stores its epoch to its flags (system-scope release), then waits for its
// flags (relaxed polls, then a system-scope acquire fence); phase
// p + 1 starts after every wait of phase p has finished.  The transport queues the consecutive signal/wait steps of
// a stream-ordered pipeline (a step's done tokens, the next step's readies)
// into one such launch instead of one launch each: same order of every
// operation on the stream, fewer kernel boundaries (~1.5-1.9 us each).
constexpr int kMaxPhases = 8;

struct SigPhaseArgs {
  uint32_t *sig[kMaxFlags];
  const uint32_t *wait[kMaxFlags];
  uint32_t *err;
  const uint32_t *epoch_dev;  // NULL, or a device word added to every epoch at run time (graph replays)
  uint64_t timeout_ticks;
  uint32_t nphase;
  uint32_t light;  // 1: relaxed stores and polls, no fences (HICCL_PROG_FENCES, as the programs' prologue)
  uint32_t sig_end[kMaxPhases];   // phase p signals sig[sig_end[p-1] .. sig_end[p])
  uint32_t wait_end[kMaxPhases];  // and waits for wait[wait_end[p-1] .. wait_end[p])
  uint32_t epoch[kMaxPhases];
};

constexpr int kProgMaxPhases = 64;
constexpr int kProgBlock = 256;

struct ProgPhase {
  uint32_t sig_begin, sig_end, wait_begin, wait_end;
};

struct ProgArgs {
  const PlanDesc *desc;  // computes of the unit batch; pad bit 0: exact byte copy, bits 1-2: peer flags
  const char *const *ptrs;
  const uint32_t *unit_comp;
  const ProgPhase *phase;
  uint32_t *const *sig;
  const uint32_t *const *wait;
  uint64_t *gate;  // workgroup 0 stores the launch's sequence number here after the phases
  uint32_t *err;
  const uint32_t *epoch_dev;
  uint64_t timeout_ticks;
  uint64_t nunits;
  uint32_t stride, nphase;
  uint64_t seq;  // this launch's gate value (+ *epoch_dev); never reused, see hiccl_program_launch
  uint32_t light;  // 1: relaxed token stores, no fences in the prologue (HICCL_PROG_FENCES, prog_light())
  uint32_t epoch[kProgMaxPhases];  // per launch: phase p stores / awaits epoch[p] (+ *epoch_dev)
};

// ---- what the one list of element types (engine.h) answers (dtype: HICCL_*,
// acc: HICCL_ACC_*, op: HICCL_OP_*)

size_t esize(int dtype);            // bytes per element, 0 for an unknown dtype
// a headline type (f32, bf16 / f16 native) under SUM: the full tuning table
bool tuned_type(int dtype, int acc, int op);
// packets per lane of the PHASE engine's default chunk: a property of (dtype,
// acc) under every operator but kOpWidenAccum, which takes 8, and the weighted
// ops, which answer for themselves (phase_p_weighted).  The operator is
// not defaulted: a caller that sizes units (unit_pkts) must name the launch's
// own, or the descriptor table and the kernel disagree about the chunk.
int phase_p(int dtype, int acc, int op);

// ---- kernel tables: the launcher of a shape, or NULL where no kernel has it
// (engine: HICCL_ENGINE_TILE / _PHASE; pol: 10*store + load)

typedef void (*single_fn)(const SingleArgsScaled &, dim3, hipStream_t);
typedef void (*plan_fn)(const PlanArgsScaled &, dim3, hipStream_t);
typedef void (*prog_fn)(const ProgArgs &, dim3, hipStream_t);

single_fn pick_single(int dtype, int acc, int op, int engine, int block, int unroll, int pol);
plan_fn pick_plan(int dtype, int acc, int op, int engine, int unroll, int pol = kDefPol);
prog_fn pick_prog(int dtype, int op, int unroll);
// the MAX / MIN half of the tables (reduce_ops.hip), reached through the three above
single_fn pick_single_maxmin(int dtype, int acc, int op, int engine, int block, int unroll, int pol);
plan_fn pick_plan_maxmin(int dtype, int acc, int op, int engine, int unroll, int pol);
prog_fn pick_prog_maxmin(int dtype, int op, int unroll);
// the PROD / BAND / BOR / BXOR part (reduce_prod.hip), reached the same way
single_fn pick_single_prod(int dtype, int acc, int op, int engine, int block, int unroll, int pol);
plan_fn pick_plan_prod(int dtype, int acc, int op, int engine, int unroll, int pol);
prog_fn pick_prog_prod(int dtype, int op, int unroll);
// the scaled sums (reduce_scale.hip; op == kOpScaledSum): no program kernels
single_fn pick_single_scale(int dtype, int acc, int op, int engine, int block, int unroll, int pol);
plan_fn pick_plan_scale(int dtype, int acc, int op, int engine, int unroll, int pol);
// the two OCP FP8 types under every operator they have (reduce_f8.hip): SUM,
// MAX, MIN and kOpScaledSum (which has no program kernel)
single_fn pick_single_f8(int dtype, int acc, int op, int engine, int block, int unroll, int pol);
plan_fn pick_plan_f8(int dtype, int acc, int op, int engine, int unroll, int pol);
prog_fn pick_prog_f8(int dtype, int op, int unroll);
// the widened sums (reduce_widen.hip; op == kOpWidenSum, dtype: the inputs'): no program kernels
single_fn pick_single_widen(int dtype, int acc, int op, int engine, int block, int unroll, int pol);
plan_fn pick_plan_widen(int dtype, int acc, int op, int engine, int unroll, int pol);
// the accumulating widened sums (reduce_accum.hip; op == kOpWidenAccum, dtype: the inputs'): no program kernels
single_fn pick_single_accum(int dtype, int acc, int op, int engine, int block, int unroll, int pol);
plan_fn pick_plan_accum(int dtype, int acc, int op, int engine, int unroll, int pol);
// the mixed plan kernels (reduce_mixed.hip; op == kOpMixedSum, the six floating dtypes): plan kernels only
plan_fn pick_plan_mixed(int dtype, int acc, int op, int engine, int unroll, int pol);
// the weighted widened sums (reduce_weighted.hip; op == kOpWeightedSum / kOpWeightedAccum, dtype: the inputs'):
// launchers of their own type, either engine's default shape, no program kernels; phase_p asks
// phase_p_weighted for their PHASE chunk
typedef void (*single_w_fn)(const SingleArgsWeighted &, dim3, hipStream_t);
typedef void (*plan_w_fn)(const PlanArgsWeighted &, dim3, hipStream_t);
single_w_fn pick_single_weighted(int dtype, int acc, int op, int engine, int block, int unroll, int pol);
plan_w_fn pick_plan_weighted(int dtype, int acc, int op, int engine, int unroll, int pol);
int phase_p_weighted(int dtype, int op);

// ---- the plain kernels

void launch_sigwait_phases(const SigPhaseArgs &a, hipStream_t s);
void launch_counter_add(uint32_t *ctr, uint32_t v, hipStream_t s);
// false: no fill kernel for this dtype (the floating types only: FLOAT32 /
// FLOAT64 / BFLOAT16 / FLOAT16 / FLOAT8_E4M3 / FLOAT8_E5M2)
bool launch_fill(int dtype, unsigned blocks, hipStream_t s, char *out, uint64_t count, uint64_t key, uint64_t first);
void launch_copy(unsigned blocks, hipStream_t s, void *dst, const void *src, uint64_t npkt);
void launch_copy_bytes(hipStream_t s, char *dst, const char *src, uint64_t nbytes);

}  // namespace hiccl_impl
