"""GPU tier of the fp16 element type (torch.float16 / HICCL_FLOAT16): every
layer that takes the type, on the hostile values of tests/hostile_f16.py.

  1. every one-shot kernel shape of OpF16 (native v_pk_add_f16 accumulation)
     and of OpF16Wide (f32 accumulator, HICCL_ACC_WIDE), n on both sides of
     the 8-input group, every part of a unit present;
  2. tamed raw bit patterns, and the remainder groups of 4-7 inputs;
  3. the scalar head / tail path, every class on every element;
  4. all 65,536 patterns: as a single input, and added to 16 fixed addends;
  5. the plan kernel: a ragged batch, either engine, every tile size and peer
     policy, one launch per compute;
  6. k_program at both unrolls, mixed with byte copies, behind a signal phase;
  7. the host pipe;  8. fill_uniform;  9. the fixture;  10. Compute<HiCCL::f16>.

Expected values are the NumPy restatements of tests/hostile_f16.py (native:
in-order float16 adds from +0, which tests/golden/make_golden_f16.py pins to
the reference's reduce_kernel<_Float16>; wide: in-order float32 adds, rounded
once), compared bit for bit; a NaN output is compared by NaN-ness only, so
every test first asserts that at most a quarter of what it expects is NaN.
Shapes are the smallest with every part of a unit (test_hostile_gpu.full_count).
"""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import hiccl_amd
import hostile_f16 as H
from conftest import ROOT, load_golden
from hiccl_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TDT = torch.float16
V = 8  # halves per 16-byte packet
TILE, PHASE, AUTO = L.HICCL_ENGINE_TILE, L.HICCL_ENGINE_PHASE, L.HICCL_ENGINE_AUTO
NT = 2  # hiccl_reduce_config_t.store_policy: nt stores whatever the launch's size
NS = [1, 2, 3, 8, 9, 17]
SENTINEL = 0xA5  # every byte of an output and its guards before a launch (0xA5A5: a finite half)

# op -> (f32 accumulator, headline type with the full shape table, packets per lane of the phased engine)
OPS = {"f16": (False, True, 16), "f16wide": (True, False, 8)}
ENGINE_IDS = pytest.mark.parametrize("engine", [TILE, PHASE], ids=["tile", "phase"])


# ------------------------------------------------------------ device helpers

def to_dev(bits):
    """uint16 half patterns -> a float16 device tensor holding those bits."""
    a = np.ascontiguousarray(bits, np.uint16)
    return torch.from_numpy(a.view(np.int16).copy()).view(TDT).to(DEV)


def to_host(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def place_inputs(x, offsets):
    """Each input row at an element offset inside a buffer of its own."""
    ins = []
    for k in range(x.shape[0]):
        b = torch.empty(x.shape[1] + offsets[k] + 8, dtype=TDT, device=DEV)
        b.view(torch.uint8).fill_(0x5A)
        b[offsets[k]:offsets[k] + x.shape[1]].copy_(to_dev(x[k]))
        ins.append((b, offsets[k]))
    return ins


def new_output(count, out_off):
    ob = torch.empty(count + out_off + 8, dtype=TDT, device=DEV)
    ob.view(torch.uint8).fill_(SENTINEL)
    return ob


def check_output(ob, out_off, count, exp, what):
    host = to_host(ob)
    got = host[out_off:out_off + count]
    assert H.bits_equal(got, exp), f"{what}: {H.first_mismatch(got, exp)}"
    assert (host[:out_off].view(np.uint8) == SENTINEL).all(), f"{what}: guard before the output written"
    assert (host[out_off + count:].view(np.uint8) == SENTINEL).all(), f"{what}: guard after the output written"


def gpu_reduce(x, offsets, out_off, config, what=""):
    """One-shot reduction of the rows of x, inputs and output at element
    offsets; returns the output's bits (guards checked)."""
    n, count = x.shape
    ins = place_inputs(x, offsets)
    ob = new_output(count, out_off)
    hiccl_amd.reduce(ob[out_off:out_off + count], [b[o:o + count] for b, o in ins], count=count, config=config)
    torch.cuda.synchronize()
    host = to_host(ob)
    assert (host[:out_off].view(np.uint8) == SENTINEL).all(), f"{what}: guard before the output written"
    assert (host[out_off + count:].view(np.uint8) == SENTINEL).all(), f"{what}: guard after the output written"
    return host[out_off:out_off + count]


def cfg_of(op, **kw):
    if OPS[op][0]:
        kw["acc"] = L.HICCL_ACC_WIDE
    return kw


def full_count(unit):
    """Scalar head, two full units, a half unit, three packets, scalar tail."""
    return (V - 1) + (2 * unit + unit // 2 + 3) * V + (V - 1)


def offsets_for(n, out_off):
    """Input k at element phase (out_off + 1 + k) mod V."""
    return [(out_off + 1 + k) % V for k in range(n)]


def run_one_shot(op, x, cfg, out_off=1, what=""):
    exp = H.expected(x, wide=OPS[op][0])
    H.assert_nan_cap(exp)
    what = f"{op} n={x.shape[0]} count={x.shape[1]} {cfg} {what}"
    got = gpu_reduce(x, offsets_for(x.shape[0], out_off), out_off, cfg, what)
    assert H.bits_equal(got, exp), f"{what}: {H.first_mismatch(got, exp)}"
    return exp


def shapes_of(op):
    """(id, config, packets per unit) of every one-shot shape the op has."""
    _, tuned, P = OPS[op]
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


# ---------------------------------------------------------------- 1. one-shot

@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("op,cfg,unit", ONE_SHOT)
def test_one_shot_hostile(op, cfg, unit, n):
    """Every class through the vector add of every shape; with 17 classes
    (prime) every class lands on every packet slot, lane and half of a pair."""
    x = H.hostile(n, full_count(unit), shift=n, seed=n)
    exp = run_one_shot(op, x, cfg)
    s = H.shares(exp)
    assert s["inf"] > 0 and s["zero"] > 0 and s["sub"] > 0, s


# ----------------------------------- 2. tamed raw bits and remainder groups

@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("op,cfg,unit", ONE_SHOT_DEFAULT)
def test_one_shot_tamed_bits(op, cfg, unit, n):
    """Random bit patterns (exponents tamed outside every eighth column),
    plain and with the inputs' exponents near input 0's."""
    for near in (False, True):
        run_one_shot(op, H.tamed_bits(n, full_count(unit), seed=n, near=near), cfg, what=f"near={near}")


@pytest.mark.parametrize("n", [4, 5, 6, 7, 12, 13, 14, 15])
@pytest.mark.parametrize("op", list(OPS))
def test_one_shot_remainder_groups(op, n):
    """The remainder groups of 4 to 7 inputs (tile_body's switch), alone and
    after a full group of 8; either engine's default shape."""
    for engine, unit in ((TILE, 1024), (PHASE, 512 * OPS[op][2])):
        run_one_shot(op, H.hostile(n, full_count(unit), shift=n, seed=n), cfg_of(op, engine=engine))


# ------------------------------------------------------------ 3. scalar path

@pytest.mark.parametrize("n", [1, 3, 9])
@ENGINE_IDS
@pytest.mark.parametrize("op", list(OPS))
def test_scalar_head_and_tail_every_class(op, engine, n):
    """count = head + one packet + tail at every shift: every class reaches
    Op::sadd / Op::sstore on every head and tail element.  Then counts below
    a packet (a scalar-only compute), as a head and as a tail."""
    cfg = cfg_of(op, engine=engine)
    exps = []
    for shift in range(H.NCLS):
        for out_off, count in ((1, (V - 1) + V + (V - 1)), (1, V - 1), (0, V - 1)):
            x = H.hostile(n, count, shift=shift, seed=shift)
            exp = H.expected(x, wide=OPS[op][0])
            what = f"{op} n={n} shift={shift} count={count} out_off={out_off}"
            got = gpu_reduce(x, offsets_for(n, out_off), out_off, cfg, what)
            assert H.bits_equal(got, exp), f"{what}: {H.first_mismatch(got, exp)} " \
                                           f"(classes {H.class_of(count, shift).tolist()})"
            exps.append(exp)
    H.assert_nan_cap(np.concatenate(exps))


# ------------------------------------------------------------ 4. exhaustive

ALL_PATTERNS = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)


@pytest.mark.parametrize("out_off", [0, 1], ids=["aligned", "odd"])
@ENGINE_IDS
@pytest.mark.parametrize("op", list(OPS))
def test_every_bit_pattern_single_input(op, engine, out_off):
    """out = +0 + x for each of the 65,536 patterns: subnormals kept,
    -0 -> +0, Inf kept, NaN stays NaN; rotated at the odd offset so that
    the scalar head and tail get other patterns."""
    x = np.roll(ALL_PATTERNS, 5 * out_off)[None, :]
    exp = run_one_shot(op, x, cfg_of(op, engine=engine), out_off=out_off)
    finite = ~H.is_nan(x[0])
    want = x[0].copy()
    want[want == 0x8000] = 0
    assert np.array_equal(exp[finite], want[finite])  # the restatement agrees with the plain statement of 0 + x


@ENGINE_IDS
@pytest.mark.parametrize("op", list(OPS))
def test_every_bit_pattern_plus_sixteen_addends(op, engine):
    """Two inputs of 16 x 65,536 elements: every pattern, plus one of the 16
    addends of the C++ `+=` test per 65,536-block (+-0, +-2^-24, +-2^-14,
    +-1, 1 + 2^-10, -2048, +-65504, 16, +-Inf, a NaN): one half add (or one
    f32 add and one rounding) on every pair.  About 9 % of the outputs are NaN."""
    x = np.stack([np.tile(ALL_PATTERNS, 16), np.repeat(H.ADDENDS, 1 << 16)])
    exp = run_one_shot(op, x, cfg_of(op, engine=engine), out_off=1)
    assert 0.05 < H.shares(exp)["nan"] < 0.12


# ------------------------------------------------------------------ 5. plans

UNIT4 = 1024 * V  # elements of one TILE unit at unroll 4


def ragged_specs():
    """(n, output element offset, count): below a packet, exactly one unit
    (aligned: 1024 packets, no head or tail) and one element fewer / more,
    a few units with heads and tails, n from 1 to 17."""
    body = [(2, 1, 1, 1), (9, V - 1, 255, V - 1), (17, 1, 513, 0), (8, 2, 1025, V - 1), (4, 1, 2563, 1),
            (1, 0, 4103, 0), (16, 1, 8193, 1), (7, 3, 9000, V - 1), (12, 0, 2055, 1)]
    specs = [(1, 1, V - 1), (3, 0, 1), (5, 0, UNIT4), (3, 0, UNIT4 - 1), (9, 0, UNIT4 + 1)]
    specs += [(n, off, (V - off) % V + pkts * V + tail) for n, off, pkts, tail in body]
    return specs


@functools.lru_cache(maxsize=None)
def ragged_batch():
    return [(n, off, count, H.hostile(n, count, shift=c, seed=50 + c)) for c, (n, off, count) in enumerate(ragged_specs())]


PLAN_VARIANTS = {
    # id: (engine, one launch per compute, peer flags, store_policy, TILE unroll)
    "auto": (AUTO, False, 0, 0, 0), "tile": (TILE, False, 0, 0, 0), "phase": (PHASE, False, 0, 0, 0),
    "each": (AUTO, True, 0, 0, 0), "nt": (AUTO, False, 0, NT, 0),
    "peer1": (AUTO, False, L.HICCL_PEER_STORES, 0, 0), "peer2": (AUTO, False, L.HICCL_PEER_LOADS, 0, 0),
    "peer3": (AUTO, False, L.HICCL_PEER_STORES | L.HICCL_PEER_LOADS, 0, 0),
    "phase-peer3": (PHASE, False, 3, 0, 0),
    "tile-u1": (TILE, False, 0, 0, 1), "tile-u2": (TILE, False, 0, 0, 2), "tile-u4": (TILE, False, 0, 0, 4),
    "tile-u8": (TILE, False, 0, 0, 8), "tile-u16": (TILE, False, 0, 0, 16),
}
# unroll 1, 2, 8 and 16 exist for the native op only
PLAN_CASES = [pytest.param(op, v, id=f"{op}-{v}") for op in OPS for v in PLAN_VARIANTS
              if OPS[op][1] or PLAN_VARIANTS[v][4] in (0, 4)]


@pytest.mark.parametrize("op,variant", PLAN_CASES)
def test_plan_hostile_ragged_batch(op, variant):
    """A ragged, mutually misaligned batch of hostile computes as ONE launch
    (or one launch per compute: the same bits); guards around every output
    stay untouched; launched twice."""
    wide = OPS[op][0]
    engine, each, peer, store, unroll = PLAN_VARIANTS[variant]
    cfg = cfg_of(op, engine=engine)
    if store:
        cfg["store_policy"] = store
    if unroll:
        cfg["unroll"] = unroll
    comp = hiccl_amd.Compute(TDT, device=0, config=cfg)
    if peer:
        comp.set_peer(peer)
    outs, exps = [], []
    for n, off, count, x in ragged_batch():
        ob = new_output(count, off)
        comp.add(place_inputs(x, offsets_for(n, off)), (ob, off), count, compid=0)
        outs.append((ob, off, count))
        exps.append(H.expected(x, wide))
    H.assert_nan_cap(np.concatenate(exps))
    assert comp.peer() == peer and comp.numcomp == len(ragged_specs())
    for launch in range(2):
        for ob, _, _ in outs:
            ob.view(torch.uint8).fill_(SENTINEL)
        comp.start(each=each)
        comp.wait()
        if not each and engine != AUTO:
            assert comp.engine() == engine
        for c, ((ob, off, count), exp) in enumerate(zip(outs, exps)):
            check_output(ob, off, count, exp, f"{op} {variant} launch {launch} compute {c} "
                                              f"(n, off, count = {ragged_specs()[c]})")
    comp.close()


# --------------------------------------------------------------- 6. programs

def body_packets(ptr, count, esz):
    """Packets of a compute's 16-byte aligned body."""
    head = min(((16 - ptr % 16) % 16) // esz, count)
    return (count - head) * esz // 16


@pytest.mark.parametrize("size", ["unroll2", "unroll4"])
def test_program_mixed_batch_behind_a_signal_phase(size):
    """One k_program launch: a signal phase (a flag on this device stored and
    awaited with the launch's epoch), then f16 reductions of hostile data
    (n = 1, 2, 5, 9, 17, heads and tails, scalar-only computes) between two
    plans of exact byte copies at odd byte offsets.  512-packet tiles while
    the batch holds fewer than two 1024-packet tiles per CU (`unroll2`),
    1024-packet tiles above (`unroll4`: many small computes over three shared
    inputs).  Launched twice with different epochs."""
    specs = [(1, 1, V - 1), (2, 1, (V - 1) + V + 1), (5, V - 1, 1 + 700 * V + (V - 1)), (9, 1, (V - 1) + 1027 * V + 1),
             (17, 0, 513 * V + (V - 1)), (2, 0, 1), (1, 1, (V - 1) + 2051 * V + 1)]
    red = hiccl_amd.Compute(TDT, device=0)
    outs, exps, pkts = [], [], 0

    def add(x, off, ins=None):
        n, count = x.shape
        ob = new_output(count, off)
        red.add(ins or place_inputs(x, offsets_for(n, off)), (ob, off), count, compid=0)
        outs.append((ob, off, count))
        return body_packets(ob.data_ptr() + off * 2, count, 2)

    for c, (n, off, count) in enumerate(specs):
        x = H.hostile(n, count, shift=c, seed=70 + c)
        pkts += add(x, off)
        exps.append(H.native_sum(x))
    payload = np.frombuffer(H.hostile(3, 2800, shift=2, seed=9).tobytes() +
                            np.array([0x7FA00001, 0xFFFFFFFF, 0x80000000, 0x7F800001], np.uint32).tobytes(), np.uint8)
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
    if size == "unroll4":
        fcount = (V - 1) + 16384 * V + 1
        shared = H.hostile(3, fcount, shift=5, seed=33)
        shared_exp = [H.native_sum(shared[:k]) for k in (1, 2, 3)]
        shared_ins = place_inputs(shared, offsets_for(3, 1))
        j = 0
        while pkts < threshold + 1024:
            k = 1 + j % 3
            pkts += add(shared[:k], 1, shared_ins[:k])
            exps.append(shared_exp[k - 1])
            j += 1
        assert pkts >= threshold and j < 64
    else:
        assert pkts < threshold
    H.assert_nan_cap(np.concatenate(exps))
    flags = torch.zeros(4, dtype=torch.int32, device=DEV)
    prog = hiccl_amd.Program(TDT, device=0)
    prog.add_signal([flags.data_ptr()], [flags.data_ptr()])
    prog.add_plan(cps[0])
    prog.add_plan(red)
    prog.add_plan(cps[1])
    assert prog.units() == len(outs) + 2 and prog.phases() == 1
    for launch in range(2):
        for ob, _, _ in outs:
            ob.view(torch.uint8).fill_(SENTINEL)
        for dst, _, _, _ in copies:
            dst.zero_()
        prog.launch(epochs=[7 + launch], timeout_s=5.0)
        torch.cuda.synchronize()
        assert flags[0].item() == 7 + launch
        for c, ((ob, off, count), exp) in enumerate(zip(outs, exps)):
            check_output(ob, off, count, exp, f"{size} launch {launch} compute {c}")
        for dst, so, do, nb in copies:
            d = dst.cpu().numpy()
            assert np.array_equal(d[do:do + nb], payload[so:so + nb]), f"copy ({so}, {do}, {nb}) launch {launch}"
            assert not d[:do].any() and not d[do + nb:].any()
    prog.close()
    red.close()
    for cp in cps:
        cp.close()


def test_program_refuses_a_wide_plan_and_other_dtypes():
    prog = hiccl_amd.Program(TDT, device=0)
    wide = hiccl_amd.Compute(TDT, device=0, acc=L.HICCL_ACC_WIDE)
    with pytest.raises(hiccl_amd.HicclError, match="natively"):
        prog.add_plan(wide)
    bf = hiccl_amd.Compute(torch.bfloat16, device=0)
    with pytest.raises(hiccl_amd.HicclError, match="dtype"):
        prog.add_plan(bf)
    assert prog.units() == 0
    for o in (prog, wide, bf):
        o.close()


# -------------------------------------------------------------- 7. host pipe

@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
def test_host_pipe(pinned):
    """torch.float16 host tensors, n = 3, 64 KiB chunks and a count that is no
    multiple of the chunk: the same bits as the device path."""
    n, count = 3, 3 * 32768 + 4102
    x = H.hostile(n, count, shift=1, seed=21)
    exp = H.native_sum(x)
    H.assert_nan_cap(exp)

    def host_tensor(bits, offset):
        buf = torch.empty(len(bits) + offset + 4, dtype=TDT)
        if pinned:
            buf = buf.pin_memory()
        view = buf[offset:offset + len(bits)]
        view.copy_(torch.from_numpy(bits.view(np.int16).copy()).view(TDT))
        return view

    ins = [host_tensor(x[k], k % 3) for k in range(n)]
    out = host_tensor(np.zeros(count, np.uint16), 1)
    pipe = hiccl_amd.HostPipe(TDT, device=0, chunk_bytes=65536, depth=2)
    pipe.reduce(out, ins)
    got = out.view(torch.int16).numpy().view(np.uint16)
    assert H.bits_equal(got, exp), H.first_mismatch(got, exp)
    pipe.close()


# ------------------------------------------------------------------- 8. fill

def test_fill_uniform_is_the_f32_fill_rounded_to_half():
    count, seed = 70_003, 4321
    for k, first in ((0, 0), (5, 12345)):
        h = torch.empty(count, dtype=TDT, device=DEV)
        f = torch.empty(count, dtype=torch.float32, device=DEV)
        hiccl_amd.fill_uniform(h, seed, k, first=first)
        hiccl_amd.fill_uniform(f, seed, k, first=first)
        torch.cuda.synchronize()
        assert torch.equal(h.view(torch.int16), f.to(TDT).view(torch.int16))
        assert -1.0 <= h.float().min().item() and h.float().max().item() <= 1.0 and h.float().std().item() > 0.5


def test_bucket_layout_takes_float16():
    ins, out = hiccl_amd.bucket(3, 4102, dtype=TDT, device=DEV)
    stride = L.lib().hiccl_bucket_stride(L.HICCL_FLOAT16, 4102)
    assert [t.data_ptr() - ins[0].data_ptr() for t in ins + [out]] == [j * stride for j in range(4)]
    x = H.hostile(3, 4102, shift=3, seed=3)
    for k in range(3):
        ins[k].copy_(to_dev(x[k]))
    hiccl_amd.reduce(out, ins)
    torch.cuda.synchronize()
    assert H.bits_equal(to_host(out), H.native_sum(x))


# ---------------------------------------------------------------- 9. fixture

def test_golden_fixture_default_call():
    """Every case of reduce_f16.npz (the reference's reduce_kernel<_Float16>)
    through the default one-shot call, and through hiccl_reduce_f16."""
    import ctypes
    for case, d in load_golden("reduce_f16").items():
        x, y = d["in"], d["out"]
        H.assert_nan_cap(y)
        got = gpu_reduce(x, [0] * x.shape[0], 0, None, case)
        assert H.bits_equal(got, y), f"{case}: {H.first_mismatch(got, y)}"
    x, y = d["in"], d["out"]
    ins = [to_dev(r) for r in x]
    out = torch.empty(len(y), dtype=TDT, device=DEV)
    tab = (ctypes.c_void_p * len(ins))(*[t.data_ptr() for t in ins])
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(L.lib().hiccl_reduce_f16(ctypes.c_void_p(out.data_ptr()), tab, len(ins), len(y), s), "hiccl_reduce_f16")
    torch.cuda.synchronize()
    assert H.bits_equal(to_host(out), y)


# -------------------------------------------------------------------- 10. C++

def test_cpp_compute_f16_on_gpu(tmp_path):
    """build/f16_compute_hip (tests/cpp/f16_compute.cpp, built by make):
    Compute<HiCCL::f16> add / start / wait on one hostile compute of n = 3
    gives the bits of the host port (the same file built with
    HICCL_PORT_HOST) and of NumPy."""
    n, count = 3, 17 * 241 + 5
    x = H.hostile(n, count, shift=3, seed=3)
    exp = H.native_sum(x)
    H.assert_nan_cap(exp)
    inp = tmp_path / "in.bin"
    x.tofile(inp)
    outs = {}
    for port in ("hip", "host"):
        exe = os.path.join(ROOT, "build", f"f16_compute_{port}")
        assert os.path.exists(exe), "run make"
        out = tmp_path / f"out_{port}.bin"
        p = subprocess.run(["timeout", "-k", "5", "60", exe, str(inp), str(out), str(n), str(count)],
                           capture_output=True, text=True)
        assert p.returncode == 0 and "f16_compute: PASSED" in p.stdout, p.stdout + p.stderr
        outs[port] = np.fromfile(out, np.uint16)
        assert H.bits_equal(outs[port], exp), f"{port}: {H.first_mismatch(outs[port], exp)}"
    assert H.bits_equal(outs["hip"], outs["host"])
