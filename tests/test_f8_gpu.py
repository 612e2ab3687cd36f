"""GPU tier of the OCP FP8 element types (HICCL_FLOAT8_E4M3, HICCL_FLOAT8_E5M2;
torch.float8_e4m3fn, torch.float8_e5m2) on every layer, bit for bit against the
torch restatement (tests/f8_expected.py); a NaN output compares by NaN-ness.

  1. exhaustive tables: all 256 bytes as a single input and all 65,536 pairs as
     n = 2, under SUM native, SUM WIDE, MAX, MIN and the scaled sums (native
     and WIDE, six alphas), each through a one-shot call on each engine and
     through a plan;
  2. the one-shot sweep: counts 0 ... 131,072 + 16,384 + 7 (a PHASE chunk, a
     tile and a tail) x n = 0 ... 17, output and inputs at independent byte
     offsets, both store forms, both engines; n = 65 (the plan kernel); in
     place; the dynamic schedule, forced; one captured and twice-replayed call;
  3. a plan of 5 ragged computes (set_op, set_scale, set_acc, launch_each,
     enqueue, both peer flags, re-upload), a program with two token phases, the
     host pipe, hiccl_fill_uniform, hiccl_amd.Compute, build/f8_compute_hip.

A 1-byte element puts 16 elements in a packet: a TILE tile is 16,384 elements
per input, the native PHASE chunk 131,072.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import f8_expected as E
import hiccl_amd
from conftest import ROOT
from hiccl_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE, PHASE = L.HICCL_ENGINE_TILE, L.HICCL_ENGINE_PHASE
ENGINES = pytest.mark.parametrize("engine", [TILE, PHASE], ids=["tile", "phase"])
FMTS = pytest.mark.parametrize("fmt", E.FORMATS)
SENTINEL = 0xA5
TILE_ELEMS, CHUNK_ELEMS = 16384, 131072

# mode -> (op, wide, scaled)
MODES = {"sum": ("sum", False, False), "wide": ("sum", True, False), "max": ("max", False, False),
         "min": ("min", False, False), "scaled": ("sum", False, True), "scaled-wide": ("sum", True, True)}
OPCODE = {"sum": L.HICCL_OP_SUM, "max": L.HICCL_OP_MAX, "min": L.HICCL_OP_MIN}
# the exhaustive tables' variants: (mode, alpha)
VARIANTS = [pytest.param(m, None, id=m) for m in ("sum", "wide", "max", "min")] + \
           [pytest.param(m, a, id=f"{m}-{a:g}") for m in ("scaled", "scaled-wide") for a in E.ALPHAS]


def config(engine, wide=False, store=0, **more):
    cfg = dict(engine=engine, **more)
    if wide:
        cfg["acc"] = L.HICCL_ACC_WIDE
    if store:
        cfg["store_policy"] = store
    return cfg


def place(b, off):
    """The bytes of b on the device, `off` bytes past an aligned base: (slab, view)."""
    slab = torch.full((b.numel() + off + 32,), SENTINEL, dtype=torch.uint8, device=DEV)
    slab[off:off + b.numel()] = b.to(DEV)
    return slab, slab[off:off + b.numel()]


def out_slab(count, off):
    slab = torch.full((count + off + 32,), SENTINEL, dtype=torch.uint8, device=DEV)
    return slab, slab[off:off + count]


def check(slab, off, count, exp, fmt, what):
    torch.cuda.synchronize()
    host = slab.cpu()
    E.assert_equal(host[off:off + count], exp, fmt, what)
    assert (host[:off] == SENTINEL).all() and (host[off + count:] == SENTINEL).all(), f"{what}: wrote outside the output"


def as_f8(t, fmt):
    return t.view(E.TORCH[fmt])


def one_shot(fmt, ins, count, mode, alpha, cfg, what, out_off=1, in_offs=None, exp=None):
    op, wide, scaled = MODES[mode]
    if exp is None:
        exp = E.expected(ins, fmt, op, wide, alpha if scaled else None, count)
    placed = [place(x, (in_offs[k] if in_offs else k % 16)) for k, x in enumerate(ins)]
    slab, out = out_slab(count, out_off)
    hiccl_amd.reduce(as_f8(out, fmt), [as_f8(v, fmt) for _, v in placed], count=count, config=cfg, op=OPCODE[op],
                     scale=alpha if scaled else None)
    check(slab, out_off, count, exp, fmt, what)


def via_plan(fmt, ins, count, mode, alpha, what, exp, engine=L.HICCL_ENGINE_AUTO):
    op, wide, scaled = MODES[mode]
    comp = hiccl_amd.Compute(E.TORCH[fmt], device=0, acc=L.HICCL_ACC_WIDE if wide else L.HICCL_ACC_NATIVE,
                             engine=engine, op=OPCODE[op], scale=alpha if scaled else None)
    placed = [place(x, 1 + k % 16) for k, x in enumerate(ins)]
    slab, out = out_slab(count, 3)
    comp.add([as_f8(v, fmt) for _, v in placed], as_f8(out, fmt), count, compid=0)
    comp.start()
    comp.wait()
    comp.close()
    check(slab, 3, count, exp, fmt, what)


# ------------------------------------------------------ 1. exhaustive tables

@pytest.mark.parametrize("mode,alpha", VARIANTS)
@FMTS
def test_every_byte_and_every_pair(fmt, mode, alpha):
    """All 256 bytes as one input and all 65,536 ordered pairs as two, through
    a one-shot call on each engine and through a plan.  The pairs hold every
    NaN, Inf, +-max, subnormal and zero against every other byte: Inf + -Inf,
    448 + 448, -0 + -0, the saturating clamp and (scaled by 1e38) f32's Inf."""
    op, wide, scaled = MODES[mode]
    a, b = E.pair_table()
    for ins, name in (([E.ALL_BYTES], "bytes"), ([a, b], "pairs")):
        count = ins[0].numel()
        exp = E.expected(ins, fmt, op, wide, alpha if scaled else None)
        for engine in (TILE, PHASE):
            one_shot(fmt, ins, count, mode, alpha, config(engine, wide), f"{fmt} {mode} {alpha} {name} engine {engine}",
                     exp=exp)
        via_plan(fmt, ins, count, mode, alpha, f"{fmt} {mode} {alpha} {name} plan", exp)
    if mode == "sum":  # what the definition says in words
        s = E.expected([a, b], fmt)
        assert int(s[0x8080]) == 0x00, "-0 + -0 is +0 (the accumulator starts at +0)"
        top = E.MIN_ID[fmt] if fmt == "e4m3" else 0x7B
        assert int(s[top << 8 | top]) == top, "max + max saturates"
        if fmt == "e5m2":
            assert bool(E.is_nan(s, fmt)[0x7C << 8 | 0xFC]), "Inf + -Inf is NaN"


# ---------------------------------------------------------- 2. one-shot sweep

COUNTS = (0, 1, 15, 16, 17, 2 * TILE_ELEMS + 5, CHUNK_ELEMS + TILE_ELEMS + 7)
NS = (0, 1, 2, 3, 8, 9, 17)
OUT_OFFS = (0, 1, 3, 15)
ALPHA = 0.3


@functools.lru_cache(maxsize=None)
def sweep_inputs(fmt, n, count):
    """Hostile bytes for odd n, small finite values for even n (sums that are
    not all NaN or saturated)."""
    return tuple((E.hostile_bytes if n % 2 else E.tame_bytes)(fmt, n, count, seed=count % 1000 + 1))


@functools.lru_cache(maxsize=None)
def sweep_expected(fmt, mode, n, count):
    op, wide, scaled = MODES[mode]
    return E.expected(list(sweep_inputs(fmt, n, count)), fmt, op, wide, ALPHA if scaled else None, count)


@pytest.mark.parametrize("store", [2, 4], ids=["nt", "wt"])
@ENGINES
@pytest.mark.parametrize("mode", list(MODES))
@FMTS
def test_one_shot_sweep(fmt, mode, engine, store):
    """Every count x every n, the output at byte offset 0 / 1 / 3 / 15 and
    input k at k mod 16, so heads, tails and mutually misaligned packets all
    occur; count 0 writes nothing, n = 0 writes the identity (a scaled sum:
    +0 times alpha)."""
    cfg = config(engine, MODES[mode][1], store)
    i = 0
    for count in COUNTS:
        for n in NS:
            ins = list(sweep_inputs(fmt, n, count))
            one_shot(fmt, ins, count, mode, ALPHA, cfg, f"{fmt} {mode} n={n} count={count} {cfg}",
                     out_off=OUT_OFFS[i % 4], exp=sweep_expected(fmt, mode, n, count))
            i += 1


@ENGINES
@pytest.mark.parametrize("mode", ["sum", "max", "scaled-wide"])
@FMTS
def test_sixty_five_inputs_run_the_plan_kernel(fmt, mode, engine):
    n, count = 65, 2 * TILE_ELEMS + 5
    ins = E.tame_bytes(fmt, n, count, seed=65)
    ins[7] = E.hostile_bytes(fmt, 1, count, seed=7)[0]
    one_shot(fmt, ins, count, mode, ALPHA, config(engine, MODES[mode][1]), f"{fmt} {mode} n=65 engine {engine}", out_off=3)


@ENGINES
@pytest.mark.parametrize("which", ["first", "last"])
@pytest.mark.parametrize("mode", ["sum", "wide", "min"])
@FMTS
def test_in_place(fmt, mode, which, engine):
    """out == in[0] and out == in[n - 1], at a byte offset."""
    op, wide, _ = MODES[mode]
    n, count, off = 3, 2 * TILE_ELEMS + 5, 5
    ins = E.hostile_bytes(fmt, n, count, seed=11)
    exp = E.expected(ins, fmt, op, wide)
    placed = [place(x, off if k == (0 if which == "first" else n - 1) else k) for k, x in enumerate(ins)]
    slab, out = placed[0 if which == "first" else n - 1]
    hiccl_amd.reduce(as_f8(out, fmt), [as_f8(v, fmt) for _, v in placed], count=count, config=config(engine, wide),
                     op=OPCODE[op])
    check(slab, off, count, exp, fmt, f"{fmt} {mode} in place ({which}) engine {engine}")


@pytest.mark.parametrize("mode", ["sum", "scaled"])
@FMTS
def test_forced_dynamic_schedule(fmt, mode):
    """TILE on the ticket counter: grid 2 and 2^20 elements are 64 tiles, 32
    tickets per workgroup."""
    n, count = 8, 1 << 20
    cfg = config(TILE, schedule=L.HICCL_SCHED_DYNAMIC, grid=2)
    choice = hiccl_amd.auto_choice(E.TORCH[fmt], count, n, config=cfg, scale=mode == "scaled")
    assert choice["dynamic"] == 1 and choice["engine"] == TILE
    ins = E.tame_bytes(fmt, n, count, seed=3)
    ins[2] = E.hostile_bytes(fmt, 1, count, seed=4)[0]
    one_shot(fmt, ins, count, mode, ALPHA, cfg, f"{fmt} {mode} dynamic", out_off=0)
    one_shot(fmt, ins, count, mode, ALPHA, cfg, f"{fmt} {mode} dynamic, second launch on the same counter", out_off=0)


@FMTS
def test_captured_and_twice_replayed_call(fmt):
    n, count = 8, 2 * TILE_ELEMS + 5
    ins = E.tame_bytes(fmt, n, count, seed=21)
    dev_ins = [place(x, k % 16)[1] for k, x in enumerate(ins)]
    slab, out = out_slab(count, 1)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hiccl_amd.reduce(as_f8(out, fmt), [as_f8(v, fmt) for v in dev_ins])  # warm-up outside capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        hiccl_amd.reduce(as_f8(out, fmt), [as_f8(v, fmt) for v in dev_ins])
    for rep in range(2):
        new = [torch.roll(x, rep + 1) for x in ins]
        for v, x in zip(dev_ins, new):
            v.copy_(x.to(DEV))
        out.fill_(SENTINEL)
        g.replay()
        check(slab, 1, count, E.expected(new, fmt), fmt, f"{fmt} replay {rep}")


# ------------------------------------------------- 3. plans, programs, the rest

RAGGED = ((2, 1), (3, 17), (8, TILE_ELEMS + 5), (1, 16), (17, 2 * TILE_ELEMS + 33))  # (n, count)


def ragged_plan(fmt, comp, seed):
    """Five computes of ragged counts on `comp`; returns [(slab, off, count, ins)]."""
    recs = []
    for c, (n, count) in enumerate(RAGGED):
        ins = (E.hostile_bytes if c % 2 else E.tame_bytes)(fmt, n, count, seed=seed + c)
        placed = [place(x, (k + c) % 16) for k, x in enumerate(ins)]
        off = OUT_OFFS[c % 4]
        slab, out = out_slab(count, off)
        comp.add([as_f8(v, fmt) for _, v in placed], as_f8(out, fmt), count, compid=0)
        recs.append((slab, off, count, ins, placed))
    return recs


def check_plan(fmt, recs, what, op="sum", wide=False, alpha=None):
    for c, (slab, off, count, ins, _) in enumerate(recs):
        check(slab, off, count, E.expected(ins, fmt, op, wide, alpha), fmt, f"{fmt} {what} compute {c}")
        slab[off:off + count] = SENTINEL


@ENGINES
@FMTS
def test_plan_of_five_ragged_computes(fmt, engine):
    """set_op, set_scale, set_acc, launch_each, enqueue and both peer flags on
    one device; every change re-uploads."""
    comp = hiccl_amd.Compute(E.TORCH[fmt], device=0, engine=engine)
    recs = ragged_plan(fmt, comp, seed=100)
    assert comp.numcomp == 5
    comp.start()
    comp.wait()
    check_plan(fmt, recs, "sum")
    for op in ("max", "min"):
        comp.set_op(OPCODE[op])
        comp.start()
        comp.wait()
        check_plan(fmt, recs, op, op=op)
    with pytest.raises(hiccl_amd.HicclError, match="HICCL_ACC_WIDE"):
        comp.set_acc(L.HICCL_ACC_WIDE)  # the plan is MIN
    comp.set_op(L.HICCL_OP_SUM)
    comp.set_scale(ALPHA)
    comp.start(each=True)
    comp.wait()
    check_plan(fmt, recs, "scaled, launch_each", alpha=ALPHA)
    comp.set_acc(L.HICCL_ACC_WIDE)
    comp.enqueue()
    check_plan(fmt, recs, "scaled wide, enqueue", wide=True, alpha=ALPHA)
    comp.set_scale(None)
    for peer in (L.HICCL_PEER_STORES, L.HICCL_PEER_LOADS, L.HICCL_PEER_STORES | L.HICCL_PEER_LOADS):
        comp.set_peer(peer)
        comp.start()
        comp.wait()
        check_plan(fmt, recs, f"wide, peer {peer}", wide=True)
    comp.set_acc(L.HICCL_ACC_NATIVE)
    comp.start()
    comp.wait()
    check_plan(fmt, recs, "native, both peer flags")
    comp.close()


@pytest.mark.parametrize("op", ["sum", "max"])
@FMTS
def test_program_with_two_token_phases(fmt, op):
    """Two token phases, an FP8 plan and a HICCL_BYTES plan in one launch."""
    red = hiccl_amd.Compute(E.TORCH[fmt], device=0, op=OPCODE[op])
    recs = ragged_plan(fmt, red, seed=200)
    payload = torch.arange(5000, dtype=torch.int32).to(torch.uint8)
    src = payload.to(DEV)
    dst = torch.zeros(payload.numel() + 64, dtype=torch.uint8, device=DEV)
    cp = hiccl_amd.Compute(torch.uint8, device=0)
    nb = payload.numel() - 5
    cp.add([(src, 1)], (dst, 3), nb, compid=0)
    flags = torch.zeros(4, dtype=torch.int32, device=DEV)
    prog = hiccl_amd.Program(E.TORCH[fmt], device=0)
    prog.add_signal([flags.data_ptr()], [flags.data_ptr()])
    prog.add_signal([flags[1:].data_ptr()], [flags[1:].data_ptr()])
    prog.add_plan(cp)
    prog.add_plan(red)
    assert prog.phases() == 2
    for launch in range(2):
        dst.zero_()
        prog.launch(epochs=[5 + launch, 9 + launch], timeout_s=5.0)
        torch.cuda.synchronize()
        assert flags[:2].tolist() == [5 + launch, 9 + launch]
        check_plan(fmt, recs, f"program {op} launch {launch}", op=op)
        d = dst.cpu()
        assert torch.equal(d[3:3 + nb], payload[1:1 + nb]) and not d[:3].any() and not d[3 + nb:].any()
    scaled = hiccl_amd.Compute(E.TORCH[fmt], device=0, scale=0.5)
    recs2 = ragged_plan(fmt, scaled, seed=300)
    assert len(recs2) == 5
    with pytest.raises(hiccl_amd.HicclError):
        hiccl_amd.Program(E.TORCH[fmt], device=0).add_plan(scaled)  # no program runs a scaled plan
    for c in (red, cp, scaled):
        c.close()
    prog.close()


@pytest.mark.parametrize("alpha", [None, ALPHA], ids=["sum", "scaled"])
@FMTS
def test_host_pipe(fmt, alpha):
    n, count = 3, 300000
    ins = E.tame_bytes(fmt, n, count, seed=31)
    ins[1] = E.hostile_bytes(fmt, 1, count, seed=32)[0]
    pipe = hiccl_amd.HostPipe(E.TORCH[fmt], device=0, chunk_bytes=64 << 10, depth=2, scale=alpha)
    out = torch.full((count,), SENTINEL, dtype=torch.uint8)
    pipe.reduce(as_f8(out, fmt), [as_f8(x, fmt) for x in ins])
    pipe.close()
    E.assert_equal(out, E.expected(ins, fmt, alpha=alpha), fmt, f"{fmt} host pipe {alpha}")


@FMTS
def test_fill_uniform(fmt):
    """The f32 value the oracle's generator gives, under round_F."""
    count, seed, k, first = 70001, 77, 3, 5
    t = torch.full((count,), SENTINEL, dtype=torch.uint8, device=DEV)
    hiccl_amd.fill_uniform(as_f8(t, fmt), seed, k, first)
    torch.cuda.synchronize()
    ora = ctypes.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))
    x = np.empty(count, np.float32)
    ora.oracle_fill_uniform_f32.restype = None
    ora.oracle_fill_uniform_f32(ctypes.c_void_p(x.ctypes.data), ctypes.c_size_t(count), ctypes.c_uint64(seed),
                                ctypes.c_uint32(k), ctypes.c_size_t(first))
    E.assert_equal(t, E.round_f(torch.from_numpy(x), fmt), fmt, f"{fmt} fill_uniform")


@FMTS
def test_python_reduce_and_compute_on_torch_fp8_tensors(fmt):
    """hiccl_amd.reduce with op= and scale=, and hiccl_amd.Compute, on tensors
    of the torch FP8 dtype itself (no byte views)."""
    n, count = 4, 4099
    ins = E.tame_bytes(fmt, n, count, seed=41)
    xs = [as_f8(x, fmt).to(DEV) for x in ins]
    assert xs[0].dtype == E.TORCH[fmt]
    out = torch.empty(count, dtype=E.TORCH[fmt], device=DEV)
    hiccl_amd.reduce(out, xs)
    E.assert_equal(out, E.expected(ins, fmt), fmt, "reduce")
    hiccl_amd.reduce(out, xs, op=L.HICCL_OP_MAX)
    E.assert_equal(out, E.expected(ins, fmt, "max"), fmt, "reduce op=MAX")
    hiccl_amd.reduce(out, xs, scale=1 / n)
    E.assert_equal(out, E.expected(ins, fmt, alpha=1 / n), fmt, "reduce scale=")
    with pytest.raises(TypeError, match="PROD"):
        hiccl_amd.reduce(out, xs, op=L.HICCL_OP_PROD)
    with pytest.raises(TypeError, match="integer types only"):
        hiccl_amd.reduce(out, xs, op=L.HICCL_OP_BXOR)
    comp = hiccl_amd.Compute(E.TORCH[fmt], device=0)
    comp.add(xs, out, count, compid=0)
    comp.start()
    comp.wait()
    comp.close()
    E.assert_equal(out, E.expected(ins, fmt), fmt, "Compute")


def test_compute_cpp_on_the_gpu(tmp_path):
    """build/f8_compute_hip (tests/cpp/f8_compute.cpp, built by make):
    Compute<f8e4m3> and Compute<f8e5m2> on the GPU, plain and with set_scale."""
    assert os.path.exists(os.path.join(ROOT, "build", "f8_compute_hip")), "run make"
    n, count, alpha = 5, 2 * TILE_ELEMS + 77, 1.0 / 3.0
    paths, data = {}, {}
    for fmt in E.FORMATS:
        data[fmt] = E.hostile_bytes(fmt, 2, count, seed=51) + E.tame_bytes(fmt, n - 2, count, seed=52)
        paths[fmt] = (tmp_path / f"in_{fmt}.bin", tmp_path / f"out_{fmt}.bin")
        torch.stack(data[fmt]).numpy().tofile(paths[fmt][0])
    cmd = ["timeout", "-k", "5", "120", os.path.join(ROOT, "build", "f8_compute_hip")]
    for fmt in E.FORMATS:
        cmd += [str(p) for p in paths[fmt]]
    p = subprocess.run(cmd + [str(n), str(count), float(alpha).hex()], capture_output=True, text=True)
    assert p.returncode == 0 and "f8_compute: PASSED" in p.stdout, p.stdout + p.stderr
    for fmt in E.FORMATS:
        for suffix, a in (("", alpha), (".plain", None)):
            got = torch.from_numpy(np.fromfile(str(paths[fmt][1]) + suffix, np.uint8))
            E.assert_equal(got, E.expected(data[fmt], fmt, alpha=a), fmt, f"Compute<{fmt}>{suffix}")
