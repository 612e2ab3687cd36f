"""GPU tier: every kernel and element type on hostile values and ragged shapes.

tests/test_reduce_gpu.py checks the kernels' shapes thoroughly, almost only on
uniform [-1, 1) data.  This file runs the values of tests/hostile.py (signed
zeros, NaN, +-Inf, subnormal inputs and results, overflow before a cancel,
order-sensitive cancels, ties to even, the bf16 round-to-Inf tie, wide random
magnitudes, raw random bit patterns; wrapping integers) through

  1. every one-shot kernel shape of every floating op, n on both sides of the
     8-input group and of the phased pair loop, every part of a unit present
     (scalar head, full units, a half unit, 3 odd packets, scalar tail);
  2. the scalar head / tail path, every class on every element;
  3. all 65,536 bf16 bit patterns as a single input (out = +0 + x);
  4. the plan kernel: batched, either engine and every tile size, one launch
     per compute, every peer policy (the scalar part between system-scope
     fences);
  5. k_program at both unrolls, all five dtypes, mixed with exact byte copies;
  6. f64 / u64 / i32: mutually misaligned inputs, input counts, unit borders.

Expected values always come from the CPU oracle on the same arrays
(tests/test_hostile_cpu.py pins it on these inputs), compared bit for bit; a
NaN output is compared by NaN-ness only, so every test first asserts that at
most a quarter of what it expects is NaN.
"""
import functools

import numpy as np
import pytest
import torch

import hiccl_amd
import hostile as H
from conftest import bits_equal, first_mismatch
from hiccl_amd import _lib as L
from test_reduce_gpu import DEV, TORCH_OF, gpu_reduce, to_dev, to_host

pytestmark = pytest.mark.gpu

TILE, PHASE, AUTO = L.HICCL_ENGINE_TILE, L.HICCL_ENGINE_PHASE, L.HICCL_ENGINE_AUTO
NT = 2  # hiccl_reduce_config_t.store_policy: nt stores whatever the launch's size (default: write-through when small)
NS = [1, 2, 3, 8, 9, 17]

# op -> (hostile kind, NumPy carrier, bf16 f32-accumulator mode, headline type with the full shape table,
#        packets per lane of the phased engine)
OPS = {"f32": ("f32", np.float32, False, True, 16), "f64": ("f64", np.float64, False, False, 16),
       "bf16": ("bf16", np.uint16, False, True, 16), "bf16wide": ("bf16", np.uint16, True, False, 8)}
INT_OPS = {"u64": (np.uint64, 16), "i32": (np.int32, 8)}  # carrier, phased P


def vec(dtype):
    return 16 // np.dtype(dtype).itemsize  # elements per 16-byte packet


def cfg_of(op, **kw):
    """Config dict of a floating op (the accumulator mode goes with it)."""
    if op in OPS and OPS[op][2]:
        kw["acc"] = L.HICCL_ACC_WIDE
    return kw


def shapes_of(op):
    """(id, config, packets per unit) of every one-shot shape the op has
    (reduce.hip pick_single_op), plus the default shape of either engine with
    nt stores (small launches store write-through: another instantiation)."""
    _, _, _, tuned, P = OPS[op]
    out = []
    if tuned:
        out += [(f"t256u{u}", cfg_of(op, engine=TILE, block=256, unroll=u), 256 * u) for u in (1, 2, 4, 8, 16)]
        out += [(f"t512u{u}", cfg_of(op, engine=TILE, block=512, unroll=u), 512 * u) for u in (1, 2, 4)]
    else:
        out += [("tile", cfg_of(op, engine=TILE), 256 * 4)]
    out += [("phase", cfg_of(op, engine=PHASE), 512 * P),
            ("tile-nt", cfg_of(op, engine=TILE, store_policy=NT), 256 * 4),
            ("phase-nt", cfg_of(op, engine=PHASE, store_policy=NT), 512 * P)]
    return out


DEFAULT_SHAPES = ("t256u4", "tile", "phase")
ONE_SHOT = [pytest.param(op, cfg, unit, id=f"{op}-{sid}") for op in OPS for sid, cfg, unit in shapes_of(op)]
ONE_SHOT_DEFAULT = [pytest.param(op, cfg, unit, id=f"{op}-{sid}") for op in OPS for sid, cfg, unit in shapes_of(op)
                    if sid in DEFAULT_SHAPES]


def full_count(unit, V):
    """The smallest count with every part of a unit: a scalar head (the
    output starts one element past a 16-byte boundary), two full units, a
    half unit, three more packets, a scalar tail."""
    return (V - 1) + (2 * unit + unit // 2 + 3) * V + (V - 1)


def offsets_for(n, V, out_off):
    """Input 0 one element off the output's 16-byte phase, the others on
    every phase in turn."""
    return [(out_off + 1 + k) % V for k in range(n)]


def check(op, exp, got, what):
    H.assert_nan_cap(OPS[op][0], exp)
    assert bits_equal(got, exp), f"{what}: {first_mismatch(got, exp)}"


def run_one_shot(oracle, op, x, cfg, out_off=1, what=""):
    kind, dt, wide, _, _ = OPS[op]
    n, count = x.shape
    exp = oracle.reduce(list(x), count=count, dtype=dt, wide=wide)
    got = gpu_reduce(x, count, dt, offsets=offsets_for(n, vec(dt), out_off), out_offset=out_off, config=cfg)
    check(op, exp, got, f"{op} n={n} count={count} {cfg} {what}")
    return exp


# ---------------------------------------------------------------- 1. one-shot

@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("op,cfg,unit", ONE_SHOT)
def test_one_shot_hostile(oracle, op, cfg, unit, n):
    """Every class through the vector add of every shape: n = 8 is one full
    group, 9 and 17 a group plus a remainder (and the second and later trips
    of the phased pair loop, odd and even); with NCLS prime every class lands
    on every packet slot, lane and bf16 half."""
    kind, dt = OPS[op][:2]
    count = full_count(unit, vec(dt))
    x = H.hostile(kind, n, count, shift=n, seed=n)
    exp = run_one_shot(oracle, op, x, cfg)
    s = H.shares(kind, exp)
    assert s["inf"] > 0 and s["zero"] > 0 and s["sub"] > 0, s  # the outputs a flush or a fold would change are there


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("op,cfg,unit", ONE_SHOT_DEFAULT)
def test_one_shot_raw_bits(oracle, op, cfg, unit, n):
    """Uniformly random bit patterns, and the same with the inputs' exponents
    within +-9 of input 0's (the adds interact): the default shape per engine."""
    kind, dt = OPS[op][:2]
    count = full_count(unit, vec(dt))
    for near in (False, True):
        run_one_shot(oracle, op, H.raw_bits(kind, n, count, seed=n, near=near), cfg, what=f"near={near}")


@pytest.mark.parametrize("n", [4, 5, 6, 7, 12, 13, 14, 15])
@pytest.mark.parametrize("op", list(OPS))
def test_one_shot_remainder_groups(oracle, op, n):
    """The remainder groups of 4 to 7 inputs (tile_body's switch), alone and
    after a full group of 8; either engine's default shape."""
    kind, dt, _, _, P = OPS[op]
    for engine, unit in ((TILE, 1024), (PHASE, 512 * P)):
        x = H.hostile(kind, n, full_count(unit, vec(dt)), shift=n, seed=n)
        run_one_shot(oracle, op, x, cfg_of(op, engine=engine))


# ------------------------------------------------------------ 2. scalar path

@pytest.mark.parametrize("n", [1, 3, 9])
@pytest.mark.parametrize("engine", [TILE, PHASE], ids=["tile", "phase"])
@pytest.mark.parametrize("op", list(OPS))
def test_scalar_head_and_tail_every_class(oracle, op, engine, n):
    """count = head + one packet + tail, every shift: every class reaches
    Op::sadd / Op::sstore on every head and every tail element.  Then counts
    below one packet: the scalar-only compute (npkt == 0), as a head (output
    one element past a 16-byte boundary) and as a tail (output aligned)."""
    kind, dt, wide, _, _ = OPS[op]
    V = vec(dt)
    cfg = cfg_of(op, engine=engine)
    exps = []
    for shift in range(H.NCLS):
        for out_off, count in ((1, (V - 1) + V + (V - 1)), (1, V - 1), (0, V - 1)):
            x = H.hostile(kind, n, count, shift=shift, seed=shift)
            exp = oracle.reduce(list(x), dtype=dt, wide=wide)
            got = gpu_reduce(x, count, dt, offsets=offsets_for(n, V, out_off), out_offset=out_off, config=cfg)
            assert bits_equal(got, exp), f"{op} n={n} shift={shift} count={count} out_off={out_off}: " \
                                         f"{first_mismatch(got, exp)} (classes {H.class_of(count, shift).tolist()})"
            exps.append(exp)
    H.assert_nan_cap(kind, np.concatenate(exps))


# ------------------------------------------------------- 3. bf16, exhaustive

@pytest.mark.parametrize("out_off", [0, 1], ids=["aligned", "odd"])
@pytest.mark.parametrize("engine", [TILE, PHASE], ids=["tile", "phase"])
@pytest.mark.parametrize("op", ["bf16", "bf16wide"])
def test_bf16_every_bit_pattern_single_input(oracle, op, engine, out_off):
    """One input holding all 65,536 bf16 patterns: out = +0 + x for each one
    (subnormals kept, -0 -> +0, Inf kept, NaN stays NaN), through the vector
    add and the conversion; rotated so that the scalar head and tail get
    other patterns at the odd offset."""
    x = np.roll(np.arange(1 << 16, dtype=np.uint32).astype(np.uint16), 5 * out_off)[None, :]
    exp = run_one_shot(oracle, op, x, cfg_of(op, engine=engine), out_off=out_off)
    finite = ~H.is_nan("bf16", x[0])
    want = x[0].copy()
    want[want == 0x8000] = 0  # +0 + -0 = +0
    assert np.array_equal(exp[finite], want[finite])  # the oracle agrees with the plain statement of 0 + x


# ------------------------------------------------------------------ 4. plans

SENTINEL = 0xA5  # every byte of an output and its guards before a launch: a finite value in every type, not NaN


def place_inputs(x, offsets, tdt):
    """Each input row at an element offset inside its own buffer."""
    ins = []
    for k in range(x.shape[0]):
        b = torch.empty(x.shape[1] + offsets[k] + 8, dtype=tdt, device=DEV)
        b.view(torch.uint8).fill_(0x5A)
        b[offsets[k]:offsets[k] + x.shape[1]].copy_(to_dev(x[k]).view(tdt))
        ins.append((b, offsets[k]))
    return ins


def new_output(count, out_off, tdt):
    ob = torch.empty(count + out_off + 8, dtype=tdt, device=DEV)
    ob.view(torch.uint8).fill_(SENTINEL)
    return ob


def check_output(ob, out_off, count, dt, exp, what):
    host = to_host(ob, dt)
    got = host[out_off:out_off + count]
    assert bits_equal(got, exp), f"{what}: {first_mismatch(got, exp)}"
    assert (host[:out_off].view(np.uint8) == SENTINEL).all(), f"{what}: guard before the output written"
    assert (host[out_off + count:].view(np.uint8) == SENTINEL).all(), f"{what}: guard after the output written"


def ragged_specs(V):
    """(n, output element offset, count) of a ragged batch: counts from 1 to
    a few units (TILE units are 256 to 4096 packets here, the phased unit
    4096 or 8192), two scalar-only computes (a head alone, a tail alone), n
    mixed over 1-17, exact unit multiples next to odd ones."""
    body = [(2, 1, 1, 1), (9, V - 1, 255, V - 1), (17, 1, 513, 0), (5, 0, 1024, 0), (8, 2 % V, 1025, V - 1),
            (4, 1, 2563, 1), (1, 0, 4103, 0), (16, 1, 8193, 1), (7, 3 % V, 20483, V - 1), (2, 1, 300, 0),
            (12, 0, 2055, 1)]
    specs = [(1, 1, V - 1), (3, 0, 1)]
    specs += [(n, off, (V - off) % V + pkts * V + tail) for n, off, pkts, tail in body]
    return specs


@functools.lru_cache(maxsize=None)
def ragged_batch(source, V):
    """The batch's inputs (read-only, shared by every variant)."""
    out = []
    for c, (n, off, count) in enumerate(ragged_specs(V)):
        x = H.wrapping(source, n, count, seed=c) if source in INT_OPS else H.hostile(source, n, count, shift=c, seed=50 + c)
        out.append((n, off, count, x))
    return out


PLAN_VARIANTS = {
    # id: (engine, one launch per compute, peer flags, store_policy, TILE unroll)
    "auto": (AUTO, False, 0, 0, 0), "tile": (TILE, False, 0, 0, 0), "phase": (PHASE, False, 0, 0, 0),
    "each": (AUTO, True, 0, 0, 0), "nt": (AUTO, False, 0, NT, 0),
    "peer1": (AUTO, False, 1, 0, 0), "peer2": (AUTO, False, 2, 0, 0), "peer3": (AUTO, False, 3, 0, 0),
    "peer2-nt": (AUTO, False, 2, NT, 0),  # system-scope loads with plain nt stores
    "phase-peer3": (PHASE, False, 3, 0, 0),
    # the plan kernels' other tile sizes (a batch this small takes unroll 2 by itself where the type has it)
    "tile-u4": (TILE, False, 0, 0, 4), "tile-u1": (TILE, False, 0, 0, 1), "tile-u8": (TILE, False, 0, 0, 8),
    "tile-u16": (TILE, False, 0, 0, 16),
}
# unroll 1, 8 and 16 exist for the headline types only (reduce.hip pick_plan_pol)
PLAN_CASES = [pytest.param(op, v, id=f"{op}-{v}") for op in OPS for v in PLAN_VARIANTS
              if OPS[op][3] or PLAN_VARIANTS[v][4] in (0, 4)]


@pytest.mark.parametrize("op,variant", PLAN_CASES)
def test_plan_hostile_ragged_batch(oracle, op, variant):
    """A ragged, mutually misaligned batch of hostile computes as one plan:
    AUTO, either engine forced, every tile size, one launch per compute, and the peer-policy
    kernels (their scalar part runs between system-scope fences); launched
    twice, outputs and guards prefilled with a non-NaN sentinel each time."""
    kind, dt, wide, _, _ = OPS[op]
    engine, each, peer, store, unroll = PLAN_VARIANTS[variant]
    V, tdt = vec(dt), TORCH_OF[np.dtype(dt)]
    cfg = cfg_of(op, engine=engine)
    if store:
        cfg["store_policy"] = store
    if unroll:
        cfg["unroll"] = unroll
    comp = hiccl_amd.Compute(tdt, device=0, config=cfg)
    if peer:
        comp.set_peer(peer)
    outs, exps = [], []
    for n, off, count, x in ragged_batch(kind, V):
        ins = place_inputs(x, offsets_for(n, V, off), tdt)
        ob = new_output(count, off, tdt)
        comp.add(ins, (ob, off), count, compid=0)
        outs.append((ob, off, count))
        exps.append(oracle.reduce(list(x), dtype=dt, wide=wide))
    H.assert_nan_cap(kind, np.concatenate(exps))
    assert comp.peer() == peer
    for launch in range(2):
        for ob, _, _ in outs:
            ob.view(torch.uint8).fill_(SENTINEL)
        comp.start(each=each)
        comp.wait()
        if not each and engine != AUTO:
            assert comp.engine() == engine
        for c, ((ob, off, count), exp) in enumerate(zip(outs, exps)):
            check_output(ob, off, count, dt, exp, f"{op} {variant} launch {launch} compute {c} "
                                                  f"(n, off, count = {ragged_specs(V)[c]})")
    comp.close()


# --------------------------------------------------------------- 5. programs

PROG_TYPES = {"f32": np.float32, "bf16": np.uint16, "f64": np.float64, "u64": np.uint64, "i32": np.int32}
PROG_VARIANTS = {
    # id: (peer flags of the reduction plan, its store_policy) -> the policy k_program runs it under
    "default": (0, 0),   # a small plan stores write-through by size: system-scope stores
    "nt": (0, NT),       # the program's own policy, nt loads and stores
    "peer1": (1, 0), "peer2-nt": (2, NT), "peer3": (3, 0),
}
PROG_CASES = [pytest.param(t, v, id=f"{t}-{v}") for t in PROG_TYPES for v in PROG_VARIANTS
              if t not in INT_OPS or v in ("default", "nt")]


def body_packets(ptr, count, esz):
    """Packets of a compute's 16-byte aligned body (runtime.cpp split_on)."""
    head = min(((16 - ptr % 16) % 16) // esz, count)
    return (count - head) * esz // 16


@pytest.mark.parametrize("size", ["unroll2", "unroll4"])
@pytest.mark.parametrize("dtype,variant", PROG_CASES)
def test_program_hostile_mixed_batch(oracle, dtype, variant, size):
    """One k_program launch holding reductions of hostile data (wrapping
    integers for u64 / i32; n = 1, 2, 5, 9, 17, heads and tails, two
    scalar-only computes) between two plans of exact byte copies at odd byte
    offsets, against the oracle and byte for byte; no signal phases.  The
    headline types run 512-packet tiles while the batch holds fewer than two
    1024-packet tiles per CU (8 MiB on 256 CUs) and 1024-packet tiles above:
    `unroll2` stays under that, `unroll4` passes it with many small computes
    that read three shared inputs.  Launched twice."""
    dt = PROG_TYPES[dtype]
    peer, store = PROG_VARIANTS[variant]
    V, esz, tdt = vec(dt), np.dtype(dt).itemsize, TORCH_OF[np.dtype(dt)]
    source = dtype  # the hostile kind, or the integer kind, carries the dtype's name
    specs = [(1, 1, V - 1), (2, 1, (V - 1) + V + 1), (5, V - 1, 1 + 700 * V + (V - 1)), (9, 1, (V - 1) + 1027 * V + 1),
             (17, 0, 513 * V + (V - 1)), (2, 0, 1), (1, 1, (V - 1) + 2051 * V + 1)]
    red = hiccl_amd.Compute(tdt, device=0, config=dict(store_policy=store) if store else None)
    if peer:
        red.set_peer(peer)
    outs, exps, pkts = [], [], 0

    def add(x, off, ins=None):
        n, count = x.shape
        ob = new_output(count, off, tdt)
        red.add(ins or place_inputs(x, offsets_for(n, V, off), tdt), (ob, off), count, compid=0)
        outs.append((ob, off, count))
        return body_packets(ob.data_ptr() + off * esz, count, esz)

    for c, (n, off, count) in enumerate(specs):
        x = H.wrapping(source, n, count, seed=c) if dtype in INT_OPS else H.hostile(source, n, count, shift=c, seed=70 + c)
        pkts += add(x, off)
        exps.append(oracle.reduce(list(x), dtype=dt))
    # two byte-copy plans: hostile values (NaN patterns, -0, subnormals) as raw bytes, plus signalling NaNs
    raw = H.wrapping("u64", 3, 700, seed=9) if dtype in INT_OPS else H.hostile(source, 3, 5600 // esz, shift=2, seed=9)
    payload = np.concatenate([np.frombuffer(raw.tobytes(), np.uint8),
                              np.frombuffer(np.array([0x7FA00001, 0xFFFFFFFF, 0x80000000, 0x7F800001], np.uint32).tobytes(), np.uint8)])
    src = torch.from_numpy(payload.copy()).to(DEV)
    copies, cps = [], []
    for so, do, nb in ((1, 3, len(payload) - 5), (13, 11, 4099)):
        dst = torch.zeros(nb + 64, dtype=torch.uint8, device=DEV)
        cp = hiccl_amd.Compute(torch.uint8, device=0)
        cp.add([(src, so)], (dst, do), nb, compid=0)
        pkts += body_packets(dst.data_ptr() + do, nb, 1)
        copies.append((dst, so, do, nb))
        cps.append(cp)
    threshold = 2 * torch.cuda.get_device_properties(0).multi_processor_count * 256 * 4
    if size == "unroll4":  # many small computes over three shared inputs, until the batch passes the threshold
        fcount = (V - 1) + 16384 * V + 1
        shared = H.wrapping(source, 3, fcount, seed=33) if dtype in INT_OPS else H.hostile(source, 3, fcount, shift=5, seed=33)
        shared_exp = [oracle.reduce(list(shared[:k]), dtype=dt) for k in (1, 2, 3)]
        shared_ins = place_inputs(shared, offsets_for(3, V, 1), tdt)
        j = 0
        while pkts < threshold + 1024:
            k = 1 + j % 3
            pkts += add(shared[:k], 1, shared_ins[:k])
            exps.append(shared_exp[k - 1])
            j += 1
        assert pkts >= threshold and j < 64
    else:
        assert pkts < threshold
    if dtype not in INT_OPS:
        H.assert_nan_cap(dtype, np.concatenate(exps))
    prog = hiccl_amd.Program(tdt, device=0)
    prog.add_plan(cps[0])
    prog.add_plan(red)
    prog.add_plan(cps[1])
    assert prog.units() == len(outs) + 2 and prog.phases() == 0
    host_src = payload
    for launch in range(2):
        for ob, _, _ in outs:
            ob.view(torch.uint8).fill_(SENTINEL)
        for dst, _, _, _ in copies:
            dst.zero_()
        prog.launch()
        torch.cuda.synchronize()
        for c, ((ob, off, count), exp) in enumerate(zip(outs, exps)):
            check_output(ob, off, count, dt, exp, f"{dtype} {variant} {size} launch {launch} compute {c}")
        for dst, so, do, nb in copies:
            d = dst.cpu().numpy()
            assert np.array_equal(d[do:do + nb], host_src[so:so + nb]), f"copy ({so}, {do}, {nb}) launch {launch}"
            assert not d[:do].any() and not d[do + nb:].any()
    prog.close()
    red.close()
    for cp in cps:
        cp.close()


# ------------------------------------- 6. f64 / u64 / i32: the shape matrix

MATRIX_TYPES = {"f64": (np.float64, 16), "u64": (np.uint64, 16), "i32": (np.int32, 8)}  # carrier, phased P
ENGINE_CFG = pytest.mark.parametrize("engine", [TILE, PHASE], ids=["tile", "phase"])


def matrix_data(t, n, count, seed):
    if n == 0:
        return np.zeros((0, count), MATRIX_TYPES[t][0])
    if t != "f64":
        return H.wrapping(t, n, count, seed=seed)
    # an array shorter than the class list cannot hold a NaN class and stay under the NaN cap: it starts after
    # them (the scalar sweep above puts the NaN classes on every element of such counts)
    return H.hostile("f64", n, count, shift=seed if count >= H.NCLS else H.CLASSES.index("pos_inf"), seed=seed)


def matrix_run(oracle, t, x, count, engine, offsets, out_off, what):
    dt = MATRIX_TYPES[t][0]
    exp = oracle.reduce(list(x), count=count, dtype=dt)
    if t == "f64":
        H.assert_nan_cap("f64", exp)
    got = gpu_reduce(x, count, dt, offsets=offsets, out_offset=out_off, config=dict(engine=engine))
    assert bits_equal(got, exp), f"{t} {what}: {first_mismatch(got, exp)}"


MISALIGN = [pytest.param(t, io, oo, id=f"{t}-in{io}-out{oo}") for t, (dt, _) in MATRIX_TYPES.items()
            for io in range(vec(dt)) for oo in range(vec(dt))]


@ENGINE_CFG
@pytest.mark.parametrize("t,in_off,out_off", MISALIGN)
def test_matrix_misaligned_inputs(oracle, t, in_off, out_off, engine):
    """Input 0 at every element offset against every output offset (V = 2 or
    4 elements per packet), the other inputs on the offsets after it."""
    dt, P = MATRIX_TYPES[t]
    V, n = vec(dt), 5
    offs = [(in_off + k) % V for k in range(n)]
    for count in (1, V + 1, 1024 * V + 3, (2 * 512 * P + 517) * V + 1):
        x = matrix_data(t, n, count, seed=count % 97)
        matrix_run(oracle, t, x, count, engine, offs, out_off, f"offs={offs} out={out_off} count={count}")


@ENGINE_CFG
@pytest.mark.parametrize("n", [0, 1, 2, 7, 8, 9, 65])
@pytest.mark.parametrize("t", list(MATRIX_TYPES))
def test_matrix_input_counts(oracle, t, n, engine):
    """n = 0 (+0 written), both sides of the 8-input group, and > 64 inputs
    (the pointer table in device memory, on the plan kernel)."""
    dt, _ = MATRIX_TYPES[t]
    V = vec(dt)
    count = full_count(1024, V)
    x = matrix_data(t, n, count, seed=n)
    matrix_run(oracle, t, x, count, engine, offsets_for(n, V, 1), 1, f"n={n}")


def border_counts(dt, P):
    V = vec(dt)
    return sorted({b + d for b in (V, 1024 * V, 512 * P * V) for d in (-1, 0, 1)})


BORDERS = [pytest.param(t, c, id=f"{t}-{c}") for t, (dt, P) in MATRIX_TYPES.items() for c in border_counts(dt, P)]


@ENGINE_CFG
@pytest.mark.parametrize("t,count", BORDERS)
def test_matrix_unit_borders(oracle, t, count, engine):
    """One below, at and one above a packet, a TILE unit (1024 packets) and
    a phased unit (512 x 16 packets; i32: 512 x 8), with the output aligned
    and one element past a boundary (the same body behind a scalar head)."""
    dt, _ = MATRIX_TYPES[t]
    V, n = vec(dt), 4
    for out_off in (0, 1):
        c = count + (V - 1 if out_off else 0)
        x = matrix_data(t, n, c, seed=count % 89)
        matrix_run(oracle, t, x, c, engine, [0] * n, out_off, f"count={c} out_off={out_off}")
