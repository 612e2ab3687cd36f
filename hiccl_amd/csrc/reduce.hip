// hiccl_amd/csrc/reduce.hip -- MI355X (gfx950 / CDNA4) bucket-reduction stage.
//
// Implements include/hiccl_reduce.h.  The arithmetic is the reference's
// reduce_kernel<T> (source/compute.h:2-12 GPU, :14-23 CPU):
//
//     T acc = 0; for (k = 0; k < n; k++) acc += in[k][i]; out[i] = acc;
//
// reproduced bit for bit (same order, accumulator starts at +0 in T, every
// add rounded to T, no FMA, no tree).  Everything else is MI355X-first:
//
//  * pure HBM stream, (n + 1) * sizeof(T) bytes per element, no MFMA;
//  * 16-byte packets per lane (global_load_dwordx4 with an SGPR base +
//    32-bit lane offset), U packets per input per lane per tile, so each
//    lane has G*U independent 16-B loads in flight before the in-order adds;
//  * a persistent grid (CUs x blocks_per_cu workgroups); work units handed
//    out grid-stride or by a device ticket counter (dynamic schedule: no
//    workgroup is bound to a fixed subset of DRAM channels), buffer
//    descriptors make partial units predicate-free;
//  * two engines: TILE (all n inputs of a 16 KiB tile loaded together) and
//    PHASE (a 128 KiB chunk swept input by input); AUTO picks per launch;
//  * the input pointer table travels in the kernarg segment (scalar loads,
//    no device-side T** table and no H2D copy per call, cf. compute.h:70-72);
//  * the output is 16-B aligned by peeling a scalar head; inputs may be
//    mutually misaligned (partition() element offsets, reduce.h:401-415):
//    gfx950 serves unaligned dwordx4 loads in hardware;
//  * a batched plan kernel runs every compute of a pipeline step in ONE launch
//    from a device descriptor table (vs one kernel + one stream + one
//    hipStreamSynchronize per compute, compute.h:87-117);
//  * stream-ordered transport signalling (k_sigwait_phases) and step
//    programs (k_program: token phases folded into a batch's launch), with
//    fenced tokens by default (release stores, relaxed polls closed by one
//    acquire fence per phase; hiccl_token_mode).
//
// Layout / roofline / measured numbers: DESIGN.md.
//
// The engines and kernels are templates in engine.h.  This file instantiates
// them for the SUM ops and holds the plain kernels (fills, copies, stream
// signalling); reduce_ops.hip instantiates them for MAX and MIN, reduce_f8.hip
// for the two OCP FP8 types.  The host
// files (policy.cpp: the AUTO rules; oneshot.cpp, plan.cpp, ...: the C ABI)
// see both through kernels.h.

#include "engine.h"

namespace {

// ------------------------------------------------------- synthetic inputs --

__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ float uniform_f32(uint64_t key, uint64_t i) {
  uint64_t h = splitmix64(key + i);
  return (float)(uint32_t)(h >> 40) * (1.0f / 8388608.0f) - 1.0f;
}

template <int DT>
__global__ __launch_bounds__(256) void k_fill(char *out, uint64_t count, uint64_t key,
                                              uint64_t first) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < count;
       i += (uint64_t)gridDim.x * 256) {
    float v = uniform_f32(key, first + i);
    if constexpr (DT == HICCL_FLOAT32) ((float *)out)[i] = v;
    if constexpr (DT == HICCL_FLOAT64) ((double *)out)[i] = (double)v;
    if constexpr (DT == HICCL_BFLOAT16) ((uint16_t *)out)[i] = bf_round(v);
    if constexpr (DT == HICCL_FLOAT16) ((uint16_t *)out)[i] = f16_round(v);
    // FP8: the same f32 value under round_F (|v| <= 1, so the clamp is idle)
    if constexpr (DT == HICCL_FLOAT8_E4M3) ((uint8_t *)out)[i] = F8<kE4M3>::round1<true>(v);
    if constexpr (DT == HICCL_FLOAT8_E5M2) ((uint8_t *)out)[i] = F8<kE5M2>::round1<true>(v);
  }
}

__global__ __launch_bounds__(256) void k_copy(u32x4 *__restrict__ dst,
                                              const u32x4 *__restrict__ src, uint64_t npkt) {
  constexpr int U = 4;
  const uint64_t stride = (uint64_t)gridDim.x * 256 * U;
  for (uint64_t b = (uint64_t)blockIdx.x * 256 * U; b < npkt; b += stride) {
    u32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      uint64_t p = b + u * 256 + threadIdx.x;
      if (p < npkt) v[u] = src[p];
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      uint64_t p = b + u * 256 + threadIdx.x;
      if (p < npkt) dst[p] = v[u];
    }
  }
}

__global__ void k_copy_bytes(char *dst, const char *src, uint64_t nbytes) {
  for (uint64_t i = threadIdx.x; i < nbytes; i += blockDim.x) dst[i] = src[i];
}

// ------------------------------------------------------ stream signalling --
// One wave: lanes < nsig publish `epoch` to (typically peer, IPC-mapped)
// flags with a system-scope release store; lanes < nwait spin on local flags
// with system-scope acquire loads until they reach `epoch`.  Every spin is
// bounded (s_memrealtime, 100 MHz): on timeout the lane records an error and
// exits, so a broken protocol can never hang the GPU.  k_sigwait_phases runs
// several such phases in order in one launch (SigPhaseArgs, kernels.h).

__global__ __launch_bounds__(64) void k_sigwait_phases(SigPhaseArgs a) {
  const uint32_t lane = threadIdx.x;
  const uint32_t add = a.epoch_dev ? __hip_atomic_load(a.epoch_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
  uint32_t s0 = 0, w0 = 0;
  for (uint32_t p = 0; p < a.nphase; p++) {
    const uint32_t epoch = a.epoch[p] + add;
    const uint32_t s1 = a.sig_end[p], w1 = a.wait_end[p];
    if (s0 + lane < s1) {
      if (a.light)
        __hip_atomic_store(a.sig[s0 + lane], epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      else
        __hip_atomic_store(a.sig[s0 + lane], epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (w0 + lane < w1) {
      const uint32_t *f = a.wait[w0 + lane];
      const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
      // relaxed polls in both modes (no cache invalidate per poll); in the
      // fenced mode the system-scope acquire fence below, executed by
      // this lane after its last poll, makes the load that saw the peer's
      // release store synchronise with it -- the fence form of an acquire
      // load, paid once per phase instead of once per poll
      auto poll = [&]() { return __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); };
      while ((int32_t)(poll() - epoch) < 0) {
        __builtin_amdgcn_s_sleep(2);
        if (a.err && __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) break;
        if (__builtin_amdgcn_s_memrealtime() - t0 > a.timeout_ticks) {
          if (a.err) __hip_atomic_store(a.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          break;
        }
      }
    }
    // fenced mode: each lane's acquire half of its polls, sequenced after
    // its last poll; then every lane's waits (and acquires, carried to the
    // other lanes by the barrier's workgroup-scope fences) precede any store
    // of the next phase
    if (!a.light) __atomic_thread_fence(__ATOMIC_ACQUIRE);
    __syncthreads();
    s0 = s1;
    w0 = w1;
  }
}

// One lane adds v to a device counter (stream-ordered; graph replay number).
__global__ __launch_bounds__(64) void k_counter_add(uint32_t *ctr, uint32_t v) {
  if (threadIdx.x == 0) __hip_atomic_fetch_add(ctr, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

// ---------------------------------------------- what kernels.h declares ----

namespace hiccl_impl {

size_t esize(int dtype) {
  if (is_f8(dtype)) return OpF8<kE4M3>::kEsz;
  return with_elem_sum(dtype, HICCL_ACC_NATIVE, (size_t)0, [](auto e) { return (size_t)decltype(e)::Op::kEsz; });
}

bool tuned_type(int dtype, int acc, int op) {
  // no MAX / MIN, PROD or bitwise op and no FP8 type is tuned (engine.h's list), so the other parts are not asked
  return part_tuned<kPartSum>(dtype, acc, op);
}

int phase_p(int dtype, int acc, int op) {
  if (is_weighted_op(op)) return phase_p_weighted(dtype, op);  // (reduce_weighted.hip)
  if (op == kOpWidenAccum) return phase_p_of<OpBF16AccF32>();  // the four accumulating ops alike
  if (is_f8(dtype)) return acc == HICCL_ACC_WIDE ? phase_p_of<OpF8Wide<kE4M3>>() : phase_p_of<OpF8<kE4M3>>();
  return with_elem_sum(dtype, acc, 16, [](auto e) { return phase_p_of<typename decltype(e)::Op>(); });
}

// SUM's kernels are this unit's; MAX and MIN come from reduce_ops.hip, PROD
// and the bitwise operators from reduce_prod.hip, the scaled sums from
// reduce_scale.hip; the FP8 types' kernels, whatever the operator, from
// reduce_f8.hip; the widened sums (whose dtype is the inputs') from
// reduce_widen.hip, the accumulating ones from reduce_accum.hip.
single_fn pick_single(int dtype, int acc, int op, int engine, int block, int unroll, int pol) {
  if (is_weighted_op(op)) return nullptr;  // pick_single_weighted: launchers of another type
  if (op == kOpWidenAccum) return pick_single_accum(dtype, acc, op, engine, block, unroll, pol);
  if (op == kOpWidenSum) return pick_single_widen(dtype, acc, op, engine, block, unroll, pol);
  if (is_f8(dtype)) return pick_single_f8(dtype, acc, op, engine, block, unroll, pol);
  if (op == kOpScaledSum) return pick_single_scale(dtype, acc, op, engine, block, unroll, pol);
  if (op >= HICCL_OP_PROD) return pick_single_prod(dtype, acc, op, engine, block, unroll, pol);
  if (op != HICCL_OP_SUM) return pick_single_maxmin(dtype, acc, op, engine, block, unroll, pol);
  return part_single<kPartSum>(dtype, acc, op, engine, block, unroll, pol);
}

plan_fn pick_plan(int dtype, int acc, int op, int engine, int unroll, int pol) {
  if (is_weighted_op(op)) return nullptr;  // pick_plan_weighted
  if (op == kOpMixedSum) return pick_plan_mixed(dtype, acc, op, engine, unroll, pol);  // (reduce_mixed.hip)
  if (op == kOpWidenAccum) return pick_plan_accum(dtype, acc, op, engine, unroll, pol);
  if (op == kOpWidenSum) return pick_plan_widen(dtype, acc, op, engine, unroll, pol);
  if (is_f8(dtype)) return pick_plan_f8(dtype, acc, op, engine, unroll, pol);
  if (op == kOpScaledSum) return pick_plan_scale(dtype, acc, op, engine, unroll, pol);
  if (op >= HICCL_OP_PROD) return pick_plan_prod(dtype, acc, op, engine, unroll, pol);
  if (op != HICCL_OP_SUM) return pick_plan_maxmin(dtype, acc, op, engine, unroll, pol);
  return part_plan<kPartSum>(dtype, acc, op, engine, unroll, pol);
}

prog_fn pick_prog(int dtype, int op, int unroll) {
  if (is_widen_op(op)) return nullptr;  // no program runs a widened plan (hiccl_program_add_plan)
  if (is_f8(dtype)) return pick_prog_f8(dtype, op, unroll);
  if (op >= HICCL_OP_PROD) return pick_prog_prod(dtype, op, unroll);
  if (op != HICCL_OP_SUM) return pick_prog_maxmin(dtype, op, unroll);
  return part_prog<kPartSum>(dtype, op, unroll);
}

void launch_sigwait_phases(const SigPhaseArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_sigwait_phases, dim3(1), dim3(64), 0, s, a);
}

void launch_counter_add(uint32_t *ctr, uint32_t v, hipStream_t s) {
  hipLaunchKernelGGL(k_counter_add, dim3(1), dim3(64), 0, s, ctr, v);
}

bool launch_fill(int dtype, unsigned blocks, hipStream_t s, char *out, uint64_t count, uint64_t key, uint64_t first) {
  if (dtype == HICCL_FLOAT8_E4M3 || dtype == HICCL_FLOAT8_E5M2) {
    if (dtype == HICCL_FLOAT8_E4M3)
      hipLaunchKernelGGL(k_fill<HICCL_FLOAT8_E4M3>, dim3(blocks), dim3(256), 0, s, out, count, key, first);
    else
      hipLaunchKernelGGL(k_fill<HICCL_FLOAT8_E5M2>, dim3(blocks), dim3(256), 0, s, out, count, key, first);
    return true;
  }
  return with_elem_sum(dtype, HICCL_ACC_NATIVE, false, [&](auto e) {
    typedef decltype(e) E;
    // the floating types: f32, f64, bf16, f16
    if constexpr (std::is_floating_point<typename E::Op::sacc_t>::value ||
                  std::is_same<typename E::Op::sacc_t, half_t>::value) {
      hipLaunchKernelGGL(k_fill<E::dtype>, dim3(blocks), dim3(256), 0, s, out, count, key, first);
      return true;
    } else {
      return false;
    }
  });
}

void launch_copy(unsigned blocks, hipStream_t s, void *dst, const void *src, uint64_t npkt) {
  hipLaunchKernelGGL(k_copy, dim3(blocks), dim3(256), 0, s, (u32x4 *)dst, (const u32x4 *)src, npkt);
}

void launch_copy_bytes(hipStream_t s, char *dst, const char *src, uint64_t nbytes) {
  hipLaunchKernelGGL(k_copy_bytes, dim3(1), dim3(64), 0, s, dst, src, nbytes);
}

}  // namespace hiccl_impl

