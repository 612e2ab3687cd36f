"""GPU tier: the per-unit values reduce.hip declares workgroup-uniform.

unit_body passes a unit's byte offset and its valid byte count through
readfirstlane, so every buffer descriptor of the unit stays in SGPRs.
readfirstlane broadcasts the first active lane's value without a question: a
value that was NOT the same in every lane would send the other lanes to the
first lane's tile, silently.  These cases walk every path on which the unit
index reaches the body -- the dynamic tickets (out of LDS), the static
grid-stride, tile_order with unequal segments, the last partial unit, the
phased engine, byte offsets past 2^32, k_program -- at the smallest shapes
that have them, each bit for bit against the oracle, with guard bytes around
the output (tests/test_reduce_gpu.py gpu_reduce).

The forced grid of 2 workgroups makes a launch of 65-67 tiles eligible for
the dynamic schedule (>= 32 tickets per workgroup at one tile per ticket);
each test asks the library's own answer (auto_choice) that it is.
"""
import functools

import numpy as np
import pytest
import torch

import hiccl_amd
import hostile as H
from conftest import Oracle, bits_equal, first_mismatch
from hiccl_amd import _lib as L
from test_hostile_gpu import check_output, new_output, offsets_for, place_inputs
from test_reduce_gpu import DEV, gpu_reduce

pytestmark = pytest.mark.gpu

TILE, PHASE = L.HICCL_ENGINE_TILE, L.HICCL_ENGINE_PHASE
STATIC, DYNAMIC = L.HICCL_SCHED_STATIC, L.HICCL_SCHED_DYNAMIC
NT, WT = 2, 4  # hiccl_reduce_config_t.store_policy
TILE_PKTS = 256 * 4  # the default tile: 4,096 f32 or 8,192 bf16
TYPES = {"f32": (np.float32, torch.float32), "bf16": (np.uint16, torch.bfloat16)}


def vec(dt):
    return 16 // np.dtype(dt).itemsize


def tiles_count(tiles, dt):
    """`tiles` full tiles, half a tile and 3 elements: a partial last unit
    and, where the output is aligned, a scalar tail."""
    return (tiles * TILE_PKTS + TILE_PKTS // 2) * vec(dt) + 3


@functools.lru_cache(maxsize=None)
def case(tname, n, count):
    """Inputs and the oracle's sum of one shape (read-only, shared)."""
    dt = TYPES[tname][0]
    ora = Oracle()
    x = ora.fill(n, count, seed=100 + n, dtype=dt)
    exp = ora.reduce(list(x), dtype=dt)
    x.setflags(write=False)
    exp.setflags(write=False)
    return x, exp


def tile_cfg(schedule=DYNAMIC, store=NT, order=0):
    return dict(engine=TILE, block=256, unroll=4, grid=2, schedule=schedule, grab=1, store_policy=store, order=order)


def run(oracle, tname, n, count, cfg, off, dynamic=None):
    dt, tdt = TYPES[tname]
    V = vec(dt)
    if dynamic is not None:
        got = hiccl_amd.auto_choice(tdt, count, n, config=cfg)
        assert got["dynamic"] == int(dynamic) and got["store_policy"] == cfg.get("store_policy", got["store_policy"]), got
    x, exp = case(tname, n, count)
    offsets = [(off + 1 + k) % V for k in range(n)] if off else [0] * n
    got = gpu_reduce(x, count, dt, offsets=offsets, out_offset=off, config=cfg)
    assert bits_equal(got, exp), f"{tname} n={n} count={count} off={off} {cfg}: {first_mismatch(got, exp)}"


@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [3, 8])
@pytest.mark.parametrize("tname", list(TYPES))
@pytest.mark.parametrize("variant", ["dynamic", "static", "dynamic-wt"])
def test_tiles_on_two_workgroups(oracle, variant, tname, n, off):
    """65 tiles, half a tile and 3 elements on a grid of 2: the unit index
    out of the ticket counter (nt stores: the headline kernel; write-through:
    the kernel a launch this small takes by itself) and from the static
    grid-stride; n on both sides of the 8-input group; output and inputs
    aligned and 1-3 elements off (a scalar head, mutually misaligned inputs)."""
    cfg = tile_cfg(schedule=STATIC if variant == "static" else DYNAMIC, store=WT if variant.endswith("wt") else NT)
    run(oracle, tname, n, tiles_count(65, TYPES[tname][0]), cfg, off, dynamic=variant != "static")


@pytest.mark.parametrize("tiles", [64, 66], ids=["65tiles", "67tiles"])
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("n", [3, 8])
@pytest.mark.parametrize("tname", list(TYPES))
def test_tile_order_unequal_segments(oracle, tname, n, order, tiles):
    """tile_order over 2 and 4 segments of 65 and 67 units (full tiles plus
    the partial one): the segments differ in length, so the last units take
    the branch for the long segments' extra tiles."""
    count = tiles_count(tiles, TYPES[tname][0])
    for off in (0, 1):
        run(oracle, tname, n, count, tile_cfg(order=order), off, dynamic=True)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [2, 5])
@pytest.mark.parametrize("tname", list(TYPES))
def test_phase_one_shot(oracle, tname, n, off):
    """The phased engine: 3 chunks of 512 x 16 packets and a partial one
    (half a chunk and 3 elements); n even and odd (the pair loop's tail)."""
    dt = TYPES[tname][0]
    chunk = 512 * 16
    count = (3 * chunk + chunk // 2) * vec(dt) + 3
    run(oracle, tname, n, count, dict(engine=PHASE, store_policy=NT), off)


def test_byte_offset_past_4gib(oracle):
    """One f32 input of 2^30 + 3 x 4,096 + 5 elements, default config: the
    last units' byte offsets need more than 32 bits, in both halves of the
    value made scalar.  out = +0 + x; 2^20 seeded sample indices and the
    whole last 64 KiB against the oracle's generator.  8 GiB of device
    memory, one launch."""
    count, seed = (1 << 30) + 3 * 4096 + 5, 77
    try:
        x = torch.empty(count, device=DEV)
        out = torch.empty(count, device=DEV)
    except torch.OutOfMemoryError:
        pytest.fail("needs 8 GiB of device memory")
    hiccl_amd.fill_uniform(x, seed, 0)
    out.view(torch.int32).fill_(0x5A5A5A5A)
    hiccl_amd.reduce(out, [x])
    torch.cuda.synchronize()
    last = 65536 // 4
    idx = np.concatenate([np.random.default_rng(seed).integers(0, count, 1 << 20, dtype=np.int64),
                          np.arange(count - last, count, dtype=np.int64)])
    exp = oracle.sample_sum(idx.astype(np.uint64), seed, 1)
    got = out[torch.from_numpy(idx).to(DEV)].cpu().numpy()
    del x, out
    torch.cuda.empty_cache()
    assert (idx >= 1 << 30).sum() >= count - (1 << 30)  # every element at a byte offset >= 2^32 is compared
    assert bits_equal(got, exp), first_mismatch(got, exp)


def test_program_u64_two_computes(oracle):
    """k_program's units (static, unit_comp table, tile engine at 4 packets
    per lane): one u64 batch of 2 computes with heads, tails, full and
    partial tiles; launched twice."""
    dt, tdt, V = np.uint64, torch.int64, 2
    specs = [(2, 1, (V - 1) + (2 * TILE_PKTS + 3) * V + 1), (5, 0, (TILE_PKTS + TILE_PKTS // 2) * V + 1)]
    red = hiccl_amd.Compute(tdt, device=0)
    outs, exps = [], []
    for c, (n, off, count) in enumerate(specs):
        x = H.wrapping("u64", n, count, seed=40 + c)
        ob = new_output(count, off, tdt)
        red.add(place_inputs(x, offsets_for(n, V, off), tdt), (ob, off), count, compid=0)
        outs.append((ob, off, count))
        exps.append(oracle.reduce(list(x), dtype=dt))
    prog = hiccl_amd.Program(tdt, device=0)
    prog.add_plan(red)
    assert prog.units() == len(specs) and prog.phases() == 0
    for launch in range(2):
        for ob, _, _ in outs:
            ob.view(torch.uint8).fill_(0xA5)
        prog.launch()
        torch.cuda.synchronize()
        for c, ((ob, off, count), exp) in enumerate(zip(outs, exps)):
            check_output(ob, off, count, dt, exp, f"u64 program launch {launch} compute {c}")
    prog.close()
    red.close()
