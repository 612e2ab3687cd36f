// hiccl_amd/csrc/policy.cpp -- the AUTO rules and their thresholds: which
// engine, tile shape, workgroups per CU, schedule and store form a launch
// takes (policy.h).  Measured numbers behind each rule: DESIGN.md sections
// 4-5 and the profiles named here.
//
// f16 (HICCL_FLOAT16) takes bf16's rules unchanged, native and wide alike:
// its bytes and packet shapes are bf16's and its ALU work is lower (one
// v_pk_add_f16 per two elements).  None of the thresholds below has been
// measured for f16; DESIGN.md section 5 (M17) records the one f16 / bf16
// comparison.
//
// Every operator but SUM (hiccl_op_t: MAX, MIN, PROD, BAND, BOR, BXOR) is
// untuned under every dtype: tuned_type answers false for them, so they take
// no wide or half-size tile and none of the rules made for the tuned types;
// every other rule applies by dtype unchanged.  No threshold below has been
// measured for any of them; DESIGN.md section 5 records the one MAX / SUM
// comparison (M18) and the PROD / SUM ones, f32 and uint64 (M19).
//
// A scaled sum (kOpScaledSum, kernels.h) is untuned in the same way, under
// either accumulator: it takes the rules of an untuned operator of its dtype,
// and none has been measured for it beyond M20's one f32 shape.
//
// A mixed plan (kOpMixedSum: a scaled plan some of whose computes are
// unscaled) takes the scaled sum's rules word for word (threshold_op); its
// kernels have the scaled plan kernels' shapes.  One measurement: M24.
//
// The OCP FP8 types (HICCL_FLOAT8_E4M3, HICCL_FLOAT8_E5M2) are untuned under
// every operator and either accumulator: they take the rules f64 takes (no
// wide or half-size tile, no rule of the tuned types), with their own chunk
// (phase_p: 16 packets native, 8 with the f32 accumulator).  No threshold
// below has been measured for FP8; DESIGN.md section 5 (M21) records the one
// FP8 / bf16 comparison.
//
// A widened sum (kOpWidenSum, kernels.h: bf16, f16 or FP8 inputs, an f32
// output) is untuned too.  The dtype it brings is the INPUTS' and every
// packet and byte count it brings is the OUTPUT's (four elements per packet,
// 4 * count bytes written), so it takes the rules f64 takes on the same
// packets -- tuned_type answers false for the operator, phase_p of a native
// 2-byte or FP8 accumulator is the 16 the widened ops have -- and the store
// form follows the bytes written.  No threshold below has been measured for
// it; DESIGN.md section 5 (M22) records the one measurement.
//
// An accumulating widened sum (kOpWidenAccum) takes the widened sum's rules
// word for word: the same packets, the same bytes written, and the widened
// sum's 16-packet chunk in every threshold (auto_engine, auto_bpc), so it
// answers what the widened sum answers.  Only the shape its PHASE kernels run
// differs: 8 packets per lane (phase_p with the operator: finish_cfg,
// unit_pkts, plan_shape_error).  It reads 4 more bytes per element (the old
// output), which no rule counts.  No AUTO threshold of its own; DESIGN.md
// section 5 (M23).
#include "policy.h"

namespace hiccl_impl {

namespace {

// Tickets per workgroup below which a dynamic schedule does not pay off
// (C4 at 16 / 64 MiB per input: 4 / 16 tickets per workgroup lose 33 / 14 %
// to the per-ticket barrier; 64 tickets at 256 MiB gain 3 %).
constexpr uint64_t kDynMinUnitsPerWG = 32;
// AUTO schedules dynamically from this many inputs on (TILE engine).
constexpr double kDynMinInputs = 5;
// A ticket should cover at least this many 16 KiB input tiles of traffic
// ((n + 1) per tile): one tile at n >= 8, two at n = 4..7, ... -- a ticket
// costs an atomic and a workgroup barrier (profiles/r01_schedsweep*.jsonl).
constexpr double kTicketTiles = 9;
// AUTO takes the tile engine (n >= kDynMinInputs) from this many tickets per
// workgroup on: below it the phased engine is ahead.
constexpr uint64_t kTileMinTicketsPerWG = 64;

// Wide tiles (TILE, 256 lanes x 8 packets = 32 KiB per input) on the
// dynamic schedule for few inputs (2..4) and large buckets: 32 packets per
// lane in flight over the n inputs at once.  From 128 tickets per workgroup
// (1 GiB per input) they lead the phased engine by 2-8 % (n = 2 / 3 / 4 at
// 1-4 GiB per input: 6.34-6.47 / 6.26-6.60 / 6.17-6.51 vs 5.77-6.25 TB/s);
// at 512 MiB they tie, at 256 MiB they lose (profiles/r02f_widetile_sweep.jsonl,
// r02f_widedyn_sweep.jsonl).  f32 and bf16 (native accumulation) only.
constexpr int kWideUnroll = 8;
constexpr uint64_t kWideMinTicketsPerWG = 128;

// A launch that writes at most this many bytes stores write-through (system
// scope, sc0 sc1) unless its config names a store form: see wt_by_size.
// Copies (one input) up to 32 MiB; reductions (two or more inputs per
// output, packet-weighted for a plan) up to 256 MiB.
constexpr uint64_t kWtMaxBytes = 32ull << 20;
constexpr uint64_t kWtMaxBytesReduce = 256ull << 20;
inline uint64_t wt_cap(double n) { return n >= 1.5 ? kWtMaxBytesReduce : kWtMaxBytes; }

// The paced one-shot tiles' share of the default grid (launch_shape).
constexpr uint64_t kPacedGridNum = 7, kPacedGridDen = 8;

// The operator AUTO's thresholds are counted for: an accumulating widened sum
// takes the widened sum's, on purpose -- the same chunk (16 packets) in every
// threshold, so both sums resolve to the same engine, grid and store form, and
// only the shape its PHASE kernels run differs (phase_p with the launch's own
// operator: finish_cfg, unit_pkts, plan_shape_error).
// A mixed plan (kOpMixedSum: scaled per compute) takes the scaled sum's: its
// kernels are the scaled ones with a factor chosen per unit.
// A weighted sum takes its unweighted family's, and so the widened sum's.
inline int threshold_op(int op) {
  return is_widen_op(op) ? kOpWidenSum : op == kOpMixedSum ? kOpScaledSum : op;
}

constexpr int kDefBpc = 1;
constexpr int kSmallBpc = 4;
// auto engine: with >= 5 inputs the TILE engine on the dynamic schedule;
// with fewer, PHASE (static) when every CU gets a chunk, else TILE
// (profiles/r01_schedsweep*.jsonl, r01_crossover.jsonl).
constexpr uint64_t kPhaseMinChunksPerCU = 1;

// Units per ticket of the dynamic schedule: one 128 KiB phased chunk or one
// wide tile; for 16 KiB tiles enough to cover kTicketTiles tile-loads.
uint32_t default_grab(int engine, double n, int unroll = kDefUnroll) {
  if (engine == HICCL_ENGINE_PHASE || unroll >= kWideUnroll) return 1u;
  const double g = kTicketTiles / (n + 1.0);
  return g <= 1.0 ? 1u : (uint32_t)(g + 0.999);
}

// Wide tiles for this launch: the unroll (16 for two inputs, 8 for three or
// four: n = 2 at 1-2 GiB per input 6.50-6.66 vs 6.33-6.46 TB/s at 8; n = 3 / 4
// lead at 8, profiles/r02g_wideverify.jsonl), or 0.  f32 / bf16 native only,
// from kWideMinTicketsPerWG 8-packet tiles per workgroup (1 GiB per input).
// Wide tiles exist only at block 256 with nt loads and nt stores
// (pick_single): a caller that asks for another block or cache policy keeps
// the u4 / PHASE choice instead of an unsupported shape.
int auto_wide_unroll(uint64_t npkt, double n, int dtype, const Cfg &c, int dev) {
  if (!tuned_type(dtype, c.acc, c.op) || n < 1.5 || n >= kDynMinInputs) return 0;
  if ((c.block && c.block != kDefBlock) || c.nt != kDefPol % 10 || c.store != kDefPol / 10) return 0;
  if (npkt / ((uint64_t)kDefBlock * kWideUnroll) < kWideMinTicketsPerWG * (uint64_t)device_cus(dev)) return 0;
  return n < 2.5 ? 2 * kWideUnroll : kWideUnroll;
}

// Auto engine from the packets per input of a launch (summed over its
// computes) and the number of inputs (packet-weighted mean for a plan).
// Interleaved engine x schedule sweeps, n = 5 / 8 / 16 x 32 MiB-1 GiB per
// input (profiles/r01g_xover.jsonl; bf16: r01g_bf16_crossover.jsonl): the
// tile engine on the dynamic schedule leads from 64 tickets per workgroup
// (n = 8, 1 GiB: 6.71 vs 6.32 TB/s phased), the phased engine below it
// (n = 8, 128 MiB = 32 tickets: 6.41 vs 5.94); with <= 4 inputs the phased
// engine leads at every size with a chunk per CU (r01_schedsweep.jsonl) --
// except from 1 GiB per input, where wide tiles lead (auto_wide_unroll).
int auto_engine(uint64_t npkt, double n, int dtype, const Cfg &c, int dev) {
  const int acc = c.acc;
  if (auto_wide_unroll(npkt, n, dtype, c, dev)) return HICCL_ENGINE_TILE;
  const bool packed_ok = !((dtype == HICCL_BFLOAT16 || dtype == HICCL_FLOAT16) && acc == HICCL_ACC_WIDE);
  // Round 5: a launch that stores write-through (store form left to size, at
  // most wt_cap written; f32, bf16) runs faster on the phased engine wherever the
  // dynamic tiles would otherwise take it -- 256 MiB per input, n = 8 / 16 /
  // 32 / 64: 6.49 / 6.45 / 6.71 / 6.59 vs 6.37-6.40 TB/s interleaved
  // (profiles/r05ab_c3_engines_many.jsonl; n = 8 on another box 6.50 vs
  // 6.42, r05v_c3_engines.jsonl), config 4's 256 MiB plan 6.60 vs 6.44
  // (r05aa_c4_engines.jsonl; bf16 6.62 vs 6.33, r05ad_c4_engines_bf16.jsonl);
  // at 1 GiB (nt) the tiles keep their lead.  `c.wt` is the store form the
  // launch actually takes (by size, where a write-through kernel exists).
  const bool wt = c.wt;
  const bool wt_f32 = wt && dtype == HICCL_FLOAT32;
  const bool wt_many = wt && tuned_type(dtype, acc, c.op);
  if (n >= kDynMinInputs && packed_ok && !wt_many) {
    const uint64_t tickets = npkt / ((uint64_t)kDefBlock * kDefUnroll) / default_grab(HICCL_ENGINE_TILE, n);
    if (tickets >= kTileMinTicketsPerWG * (uint64_t)device_cus(dev)) return HICCL_ENGINE_TILE;
  }
  const uint64_t chunk = (uint64_t)kPhBlock * phase_p(dtype, acc, threshold_op(c.op));
  const uint64_t cus = (uint64_t)device_cus(dev);
  const uint64_t per_cu = npkt / (cus * chunk);  // phased chunks per CU
  // Round 3, on the round-2 kernels (interleaved one-shot sweeps of n = 2 /
  // 3 / 4 / 8 at 1-4.5 chunks per CU: f32 profiles/r03n_midsize.jsonl, bf16
  // r03o_midsize_bf16.jsonl, f64 r03x_midsize_f64.jsonl, int32 and bf16 with
  // the f32 accumulator -- 64 KiB chunks -- r03ze_midsize_i32.jsonl /
  // r03ze_midsize_bf16wide.jsonl; the C5 step shape scaled up,
  // r03n_stepscale.jsonl): the phased engine needs both several chunks per
  // CU and whole rounds of them -- one chunk per workgroup (a CU per
  // workgroup) is a single memory round trip with no overlap, and a last
  // round that only part of the grid works on (1.25 / 1.5 / 2.5 chunks per
  // CU) idles the rest: PHASE lost 3-20 % to static tiles there (f32 n = 3
  // at 40 MiB: 5.08 vs 6.15 TB/s; the C5 step at 8 x 2^18: 29.6 vs 23.2
  // us).  `round_eff` = chunks / (whole rounds x CUs).
  const bool big_chunk = chunk >= 8192;  // 128 KiB per input (P = 16)
  const uint64_t chunks = (npkt + chunk - 1) / chunk;
  const double round_eff = chunks ? (double)chunks / (double)(((chunks + cus - 1) / cus) * cus) : 0.0;
  if (n < 2.5) return per_cu > 16 && round_eff >= 0.89 ? HICCL_ENGINE_PHASE : HICCL_ENGINE_TILE;
  // Round 5: with the write-through stores a launch of this size takes
  // (store form left to size, at most wt_cap written; f32), static tiles lead
  // the phased engine at three inputs: 6.80 vs 6.62 TB/s interleaved at
  // 3 x 256 MiB (profiles/r05v_c3_engines.jsonl; 6.86 vs 6.63 on another
  // box, r05r_nway.jsonl); at two and four inputs the nt table holds.
  if (n >= 2.5 && n < 3.5 && wt_f32) return HICCL_ENGINE_TILE;
  if (n < kDynMinInputs) return per_cu >= 4 && round_eff >= 0.89 ? HICCL_ENGINE_PHASE : HICCL_ENGINE_TILE;
  // many inputs, under the dynamic tiles' ticket count: PHASE from one
  // whole chunk per CU unless too much of the last round idles (f32 n = 8 at
  // 40 MiB, 1.25 per CU: tiles 6.03 vs 5.45; at 48 / 80 MiB PHASE holds:
  // 6.08 / 6.25; with 64 KiB chunks PHASE needs 80 %: int32 / bf16-wide n =
  // 8 at 1.5 per CU: tiles 5.84 / 5.94 vs 5.58 / 5.68); from 16 inputs a
  // 128 KiB chunk is >= 2 MiB of reads, and PHASE leads already with 70 %
  // of the CUs holding one (24 MiB per input, 0.75 chunks per CU: n = 16 /
  // 32 PHASE 6.56 / 6.34 vs tiles 6.15-6.25; at 0.5 per CU tiles lead:
  // 6.21 / 6.25 vs 5.43 / 5.61; profiles/r03q_sweep_manyn.jsonl)
  const bool enough = per_cu >= 1 || (n >= 16 && big_chunk);
  return enough && round_eff >= (big_chunk ? 0.7 : 0.8) ? HICCL_ENGINE_PHASE : HICCL_ENGINE_TILE;
}

// Workgroups per CU: a tile launch too small for a phased chunk per CU has
// few tiles per workgroup and is latency-bound -- four workgroups per CU
// keep more of it in flight (n = 8, 16 MiB per input: 6.31 vs 6.01 TB/s,
// 32 MiB: 6.27-6.40 vs 5.97-6.13; profiles/r01g_small_sweep.jsonl).
int auto_bpc(int engine, uint64_t npkt, int dtype, int acc, int op, int dev) {
  const uint64_t chunk = (uint64_t)kPhBlock * phase_p(dtype, acc, threshold_op(op));
  return engine == HICCL_ENGINE_TILE && npkt < kPhaseMinChunksPerCU * (uint64_t)device_cus(dev) * chunk
             ? kSmallBpc
             : kDefBpc;
}

// Packets per lane of the TILE engine: a launch with fewer than two 16 KiB
// tiles per CU is pure latency (one round trip per workgroup) -- half-size
// tiles on twice the workgroups finish it sooner (the C5 step, four n = 2
// and one n = 4 computes of 2^18 f32: 4.75 vs 5.32 us queued,
// profiles/r02c_plan_sweep.jsonl); 2 exists for the headline types only.
int auto_unroll(uint64_t npkt, int dtype, const Cfg &c, int dev) {
  return tuned_type(dtype, c.acc, c.op) && npkt < 2ull * device_cus(dev) * kDefBlock * kDefUnroll ? 2 : kDefUnroll;
}

}  // namespace

Cfg resolve(const hiccl_reduce_config_t *c) {
  Cfg r{0, 0, 0, kDefPol % 10, HICCL_ACC_NATIVE, 0, kDefPol / 10, HICCL_ENGINE_AUTO, HICCL_SCHED_AUTO, 0, 0, true,
        false, 0};
  if (c) {
    r.block = c->block;
    r.unroll = c->unroll;
    if (c->blocks_per_cu) r.bpc = c->blocks_per_cu;
    if (c->nontemporal) r.nt = c->nontemporal - 1;
    r.acc = c->acc;
    r.grid = c->grid;
    if (c->store_policy) r.store = c->store_policy - 1;
    r.store_auto = c->store_policy == 0;
    r.engine = c->engine;
    r.schedule = c->schedule;
    r.grab = c->grab;
    r.drain = c->drain;
    r.order = c->order;
  }
  return r;
}

int check_cfg(const hiccl_reduce_config_t *c, const std::string &who) {
  if (!c) return 0;
  if (c->acc != HICCL_ACC_NATIVE && c->acc != HICCL_ACC_WIDE) return fail(hipErrorInvalidValue, who + ": bad acc mode");
  if (c->engine < HICCL_ENGINE_AUTO || c->engine > HICCL_ENGINE_PHASE)
    return fail(hipErrorInvalidValue, who + ": bad engine");
  if (c->schedule < HICCL_SCHED_AUTO || c->schedule > HICCL_SCHED_DYNAMIC)
    return fail(hipErrorInvalidValue, who + ": bad schedule");
  if (c->grab < 0 || c->grab > 4096) return fail(hipErrorInvalidValue, who + ": bad grab");
  if (c->order < 0 || c->order > 4096 || (c->order & (c->order - 1)))
    return fail(hipErrorInvalidValue, who + ": order must be 0 or a power of two <= 4096");
  if (c->blocks_per_cu < 0 || c->blocks_per_cu > 64) return fail(hipErrorInvalidValue, who + ": blocks_per_cu");
  if (c->grid < 0) return fail(hipErrorInvalidValue, who + ": grid < 0");
  return 0;
}

// hiccl_op_t's values are not dense (0-2, 16-19): membership, not a range.
bool known_op(int op) {
  switch (op) {
    case HICCL_OP_SUM:
    case HICCL_OP_MAX:
    case HICCL_OP_MIN:
    case HICCL_OP_PROD:
    case HICCL_OP_BAND:
    case HICCL_OP_BOR:
    case HICCL_OP_BXOR: return true;
    default: return false;
  }
}

int check_op(int dtype, int acc, int op, const std::string &who) {
  if (!known_op(op)) return fail(hipErrorInvalidValue, who + ": unknown op " + std::to_string(op));
  if (op == HICCL_OP_SUM) return 0;
  if (dtype == HICCL_BYTES) return fail(hipErrorInvalidValue, who + ": HICCL_BYTES copies take HICCL_OP_SUM only");
  if (acc == HICCL_ACC_WIDE)
    return fail(hipErrorInvalidValue, who + ": HICCL_ACC_WIDE is a rounding mode of sums (HICCL_OP_SUM only)");
  const bool bitwise = op == HICCL_OP_BAND || op == HICCL_OP_BOR || op == HICCL_OP_BXOR;
  // an unknown dtype is left to the caller's own dtype check
  if (bitwise && esize(dtype) && dtype != HICCL_INT32 && dtype != HICCL_UINT64)
    return fail(hipErrorInvalidValue,
                who + ": HICCL_OP_BAND / _BOR / _BXOR take the integer types only (HICCL_INT32, HICCL_UINT64)");
  if (op == HICCL_OP_PROD && (dtype == HICCL_FLOAT8_E4M3 || dtype == HICCL_FLOAT8_E5M2))
    return fail(hipErrorInvalidValue,
                who + ": HICCL_OP_PROD is not defined for the FP8 types (HICCL_FLOAT8_E4M3, HICCL_FLOAT8_E5M2)");
  return 0;
}

// nt stores are not write-through: a launch's output lines may sit dirty in
// the XCD L2s until the end-of-kernel release writes them back, on the
// critical path of the next kernel on the stream (MI355X_MICROARCH.md
// "boundary": + B / 6 TB/s for B dirty bytes).  So a launch that writes at
// most wt_cap(n) bytes stores with system-scope write-through (sc0 sc1, the
// peer-store form) instead, when its config leaves the store form to size
// (store_policy 0), loads nt (the only write-through kernels) and names no
// TILE unroll other than 2 or 4 -- one rule for one-shot calls and plans.  A
// write-through kernel at another unroll may exist (one-shot TILE unroll 1
// does) and is reached on request, store_policy 4; by size it is not taken.
// Measured on the C5 step (4 x n = 2 + 1 x n = 4 computes of 2^18 f32,
// 5 MiB written, plus its five 1 MiB byte copies; tools/step_store_probe.py,
// profiles/r05d_step_store.jsonl): the reduction 4.52 -> 3.53 us per eager
// launch (0.49 -> 0.63 of 8 TB/s), 3.01 -> 2.91 us under graph replay, the
// copies 3.53 -> 3.28 us; 10-20 MiB written 20-38 % faster.  Byte copies
// lose from 48 MiB written (1-4 %); reductions keep gaining up to 256 MiB
// (tools/store_threshold_probe.py: 8 inputs writing 32-256 MiB 1.6-3 %
// faster, config 3's buckets -- n x 256 MiB -- 1.2-9.2 %, n = 2 reaching
// 7.02 TB/s; profiles/r05o_store_threshold.jsonl, r05p_store_c3.jsonl) and
// stop at 512 MiB and 1 GiB (-0.7 / -0.6 % on the TILE engine, config 2 no
// gain; r05q_store_big.jsonl, r05j_c2_store_ab.jsonl): hence the two caps.
bool wt_by_size(const Cfg &raw, int dtype, double n, uint64_t out_bytes) {
  const bool u_ok = !raw.unroll || wt_unroll(raw.unroll) || raw.engine == HICCL_ENGINE_PHASE;
  return raw.store_auto && raw.nt == kDefPol % 10 && u_ok && out_bytes <= wt_cap(dtype == HICCL_BYTES ? 1.0 : n);
}

void finish_cfg(Cfg &c, uint64_t npkt, double n, int dtype, int dev) {
  if (c.engine == HICCL_ENGINE_AUTO)
    c.engine = (c.block || c.unroll) ? HICCL_ENGINE_TILE : auto_engine(npkt, n, dtype, c, dev);
  if (c.engine == HICCL_ENGINE_PHASE) {
    if (!c.block) c.block = kPhBlock;
    if (!c.unroll) c.unroll = phase_p(dtype, c.acc, c.op);
  } else {
    if (!c.block) c.block = kDefBlock;
    if (!c.unroll) {
      const int wide = auto_wide_unroll(npkt, n, dtype, c, dev);
      c.unroll = wide ? wide : auto_unroll(npkt, dtype, c, dev);
    }
  }
  if (!c.bpc) c.bpc = auto_bpc(c.engine, npkt, dtype, c.acc, c.op, dev);
}

// The store form is decided first (wt_by_size), since AUTO's engine rules
// differ under it (auto_engine).  If the shape finish_cfg then picks lacks a
// write-through kernel, the call keeps nt stores and its engine is chosen
// again for them.  n > 64 inputs run on the plan kernel (reduce_via_table),
// whose kernels decide.  hiccl_reduce_ex and hiccl_reduce_auto_choice_ex
// share it.
Cfg oneshot_cfg(int dtype, int op, const hiccl_reduce_config_t *cfg, uint64_t npkt, uint64_t out_bytes, double n,
                int dev) {
  Cfg raw = resolve(cfg);
  raw.op = op;
  Cfg c = raw;
  c.wt = wt_by_size(raw, dtype, n, out_bytes);
  finish_cfg(c, npkt, n, dtype, dev);
  if (!c.wt) return c;
  Cfg w = c;
  w.store = kPolStoreSys;
  if (n > kMaxArgInputs ? has_plan(dtype, w.acc, w.op, w.engine, w.unroll, plan_pol(HICCL_PEER_STORES))
                        : has_single(dtype, w))
    return w;
  c = raw;
  finish_cfg(c, npkt, n, dtype, dev);
  return c;
}

int plan_pol(int peer) {
  return 10 * ((peer & HICCL_PEER_STORES) ? kPolStoreSys : kDefPol / 10) +
         ((peer & HICCL_PEER_LOADS) ? kPolLoadSys : kDefPol % 10);
}

uint64_t unit_pkts(int engine, int dtype, int acc, int unroll, int op) {
  return engine == HICCL_ENGINE_PHASE ? (uint64_t)kPhBlock * phase_p(dtype, acc, op)
                                      : (uint64_t)kDefBlock * (unroll ? unroll : kDefUnroll);
}

std::string plan_shape_error(const Cfg &c, int dtype) {
  if (c.nt != kDefPol % 10 || (c.store != kDefPol / 10 && c.store != kPolStoreSys))
    return "plan kernels load nt (nontemporal 2) and store nt (store_policy 2), system-scope write-through "
           "(store_policy 4) or either by the launch's size (store_policy 0)";
  if (c.drain) return "plan kernels do not support drain";
  if (c.order != 0 && c.order != 1) return "plan kernels run their units in linear order (order 0)";
  if (c.engine == HICCL_ENGINE_PHASE) {
    if (c.block != kPhBlock || c.unroll != phase_p(dtype, c.acc, c.op))
      return "plan kernels run the PHASE engine in its default shape only (block 512, unroll " +
             std::to_string(phase_p(dtype, c.acc, c.op)) + ")";
    return "";
  }
  if (c.block != kDefBlock) return "plan kernels run the TILE engine at block 256 only";
  const bool wt = c.store == kPolStoreSys;
  if (wt && !wt_unroll(c.unroll))
    return "write-through plan kernels (store_policy 4) run the TILE engine at unroll 4 (f32 / bf16 / f16: 2 or 4) only";
  if (!has_plan(dtype, c.acc, c.op, HICCL_ENGINE_TILE, c.unroll, plan_pol(wt ? HICCL_PEER_STORES : 0)))
    return "plan kernels run the TILE engine at unroll 4 (f32 / bf16 / f16: 1, 2, 4, 8 or 16) only";
  return "";
}

// AUTO is dynamic for the TILE engine from kDynMinInputs inputs or with wide
// tiles (with the static grid-stride each workgroup is bound to the same
// addresses mod grid x 16 KiB, i.e. to a fixed subset of DRAM channels, and
// the ones on slow channels straggle: 5.6-5.7 vs 6.3-6.7 TB/s on C2), and
// only from kDynMinUnitsPerWG tickets per workgroup.
//
// `paced`: the launch runs the one-shot kernel, whose dynamic tiles pace
// their load burst (reduce.hip group_at).  Such a launch takes 7 of every 8
// workgroups of the default grid (28 of an XCD's 32 CUs): config 2 in fresh
// processes, alternating rounds, 1.402 ms at 224 workgroups against 1.445 at
// 256, 1.418 / 1.406 at 240 / 232 and 1.402 / 1.407 / 1.418 at 216 / 208 /
// 200; the unpaced kernels gained 0.5-0.8 % from the same step (waterfall
// loops 1.435 vs 1.441, scalar descriptors 1.445 vs 1.457;
// profiles/r07a_pace_ab.jsonl, r07a_grid_ab.jsonl).  Whether the schedule is dynamic is decided on the
// full grid, so the rule moves no launch between the schedules; a grid the
// caller names is kept.
LaunchShape launch_shape(const Cfg &c, double n, uint64_t units, int cus, bool paced) {
  LaunchShape L;
  L.grid = c.grid > 0 ? (uint64_t)c.grid : (uint64_t)cus * c.bpc;
  if (L.grid > units) L.grid = units;
  L.grab = c.grab > 0 ? (uint32_t)c.grab : default_grab(c.engine, n, c.unroll);
  const bool auto_static = c.engine != HICCL_ENGINE_TILE || (n < kDynMinInputs && c.unroll < kWideUnroll);
  L.dynamic = c.schedule != HICCL_SCHED_STATIC && !(c.schedule == HICCL_SCHED_AUTO && auto_static) &&
              (units + L.grab - 1) / L.grab >= kDynMinUnitsPerWG * L.grid;
  if (paced && L.dynamic && c.engine == HICCL_ENGINE_TILE && c.grid <= 0 && L.grid >= 8)
    L.grid = L.grid * kPacedGridNum / kPacedGridDen;
  return L;
}

}  // namespace hiccl_impl
