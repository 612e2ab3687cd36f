"""GPU tier of the widened sums (bf16, f16, e4m3 or e5m2 inputs summed into an
f32 output: hiccl_reduce_widened, hiccl_reduce_plan_set_out_dtype) on every
layer that takes them.  Every comparison is bit-exact on the f32 words, a NaN
by NaN-ness, against the stored fixtures (tests/golden/reduce_widen_*.npz: the
reference's reduce_kernel<float> on the widened inputs) or the restatement the
fixtures pin (tests/widen_expected.py); every expected array is checked on the
CPU, before any device call, to be at most hostile.NAN_CAP NaN.

  1. one-shot against the fixtures: n = 1, 2, 3, 8, 9, 17, unscaled and under
     every alpha, TILE and PHASE forced and AUTO, write-through by size and nt;
  2. counts around every boundary of the layout (4 elements per packet, 4,096
     per tile, 32,768 per chunk), output offsets 0-3, mutually different input
     offsets, guard words around the output;
  3. n = 0 ... 65 (n = 65 takes the table path);
  4. unscaled equals scale = 1.0 word for word;
  5. every pattern of the type against 16 addends (the manifest's hashes);
  6. equal to hiccl_amd.reduce in f32 on x.float() inputs on the same device;
  7. plans: five computes of unequal n and count in one launch, both peer
     flags, launch_each, set_scale / clear_scale; Compute(out_dtype=);
  8. one captured and replayed call with n = 8;
  9. WidenCompute<bf16> / WidenCompute<f8e4m3> from tests/cpp/widen_sum.cpp;
 10. the Python refusals that need a tensor.
"""
import functools
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import hiccl_amd
import widen_expected as E
from conftest import GOLDEN, ROOT, load_golden
from hiccl_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE, PHASE, AUTO = L.HICCL_ENGINE_TILE, L.HICCL_ENGINE_PHASE, L.HICCL_ENGINE_AUTO
NT, WT = 2, 4  # hiccl_reduce_config_t.store_policy
COUNT = E.COUNT
PACKET, TILE_ELEMS, CHUNK_ELEMS = 4, 4096, 32768  # elements: a packet, a TILE tile (256 x 4 packets), a PHASE chunk (512 x 16)
COUNTS = (0, 1, 3, 4, 5, 4095, 4096, 4097, 4102, 32767, 32768, 32769, 2 * 32768 + 5)
GUARD = 64  # f32 guard words on either side of an output
SENTINEL = 0x7FA5A5A5  # an int32 bit pattern (a NaN as f32) no kernel writes
KINDS = pytest.mark.parametrize("kind", E.KINDS)
ENGINES3 = pytest.mark.parametrize("engine", [TILE, PHASE, AUTO], ids=["tile", "phase", "auto"])


@functools.lru_cache(maxsize=None)
def fixture(kind):
    return load_golden(f"reduce_widen_{kind}")


def in_offsets(kind, n, shift=0):
    """Mutually different element offsets: 0-7 elements for the 2-byte types,
    0-15 bytes for FP8 (they repeat only past 8 / 16 inputs)."""
    span = 8 if E.ESZ[kind] == 2 else 16
    return [(k + 1 + shift) % span for k in range(n)]


def place_inputs(kind, x, offs):
    """Row k of x on the device at element offset offs[k] past a 16-byte
    boundary; returns tensors of the kind's torch dtype."""
    count, esz = x.shape[1], E.ESZ[kind]
    out = []
    for row, off in zip(x, offs):
        buf = torch.zeros(count * esz + 64, dtype=torch.uint8, device=DEV)
        assert buf.data_ptr() % 16 == 0
        lo = off * esz
        buf[lo:lo + count * esz].copy_(torch.from_numpy(np.ascontiguousarray(row).view(np.uint8).copy()))
        out.append(buf[lo:lo + count * esz].view(E.TORCH[kind]))
    return out


def new_output(count, off):
    """An f32 output of `count` elements `off` elements past a 16-byte
    boundary, between two runs of GUARD sentinel words: (buffer, view)."""
    buf = torch.full((max(count, 4) + 2 * GUARD + 8,), SENTINEL, dtype=torch.int32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    lo = GUARD + off
    return buf, buf[lo:lo + max(count, 4)].view(torch.float32)  # (a count of 0 still names a buffer)


def check_output(buf, off, count, exp, what):
    host = buf.cpu().numpy()
    lo = GUARD + off
    assert (host[:lo] == SENTINEL).all(), f"{what}: the guard before the output was written"
    assert (host[lo + count:] == SENTINEL).all(), f"{what}: the guard after the output was written"
    E.assert_equal(host[lo:lo + count].view(np.float32), exp, what)


def run_widened(kind, x, exp, cfg, what, alpha=None, out_off=1, shift=0, ins=None, count=None, inf_of=None):
    """One one-shot call on the rows of x; checks the words and the guards.
    `inf_of`: widen_expected.assert_nan_cap's (alpha = 0 against a sum that
    the caller has compared bit for bit)."""
    count = x.shape[1] if count is None else count
    E.assert_nan_cap(exp, inf_of)
    if ins is None:
        ins = place_inputs(kind, x, in_offsets(kind, x.shape[0], shift))
    buf, out = new_output(count, out_off)
    if ins:
        hiccl_amd.reduce_widened(out, ins, count=count, config=cfg, scale=alpha)
    else:  # n == 0: the pointer form names the input dtype
        with torch.cuda.device(DEV):
            hiccl_amd.reduce_widened_ptrs(E.CODE[kind], out.data_ptr(), [], count, config=cfg, scale=alpha)
    torch.cuda.synchronize()
    check_output(buf, out_off, count, exp, what)


def config(engine, store=0):
    cfg = dict(engine=engine)
    if store:
        cfg["store_policy"] = store
    return cfg


# ---------------------------------------------------------------- 1. fixtures

@pytest.mark.parametrize("store", [0, NT], ids=["wt-by-size", "nt"])
@ENGINES3
@KINDS
def test_one_shot_fixture_cases(kind, engine, store):
    """Every stored case (n = 1, 2, 3, 8, 9, 17), unscaled and under every
    alpha, the output one element past 16 bytes and the inputs mutually
    misaligned, so head and tail run the scalar path."""
    cfg = config(engine, store)
    for n in E.NS:
        x, d = E.inputs(kind, n), fixture(kind)[f"n{n}"]
        ins = place_inputs(kind, x, in_offsets(kind, n))
        run_widened(kind, x, d["s"], cfg, f"{kind} n={n} unscaled {cfg}", ins=ins)
        for i, (name, alpha) in enumerate(E.ALPHAS):
            exp = d["s"] if i == 0 else d[f"a{i}"]
            run_widened(kind, x, exp, cfg, f"{kind} n={n} alpha {name} {cfg}", alpha=alpha, ins=ins,
                        inf_of=d["s"] if alpha == 0.0 else None)  # (the unscaled run above compared d["s"])


@KINDS
def test_write_through_on_request(kind):
    """store_policy 4 on both engines (the system-scope write-through kernels)."""
    x, d = E.inputs(kind, 9), fixture(kind)["n9"]
    for engine in (TILE, PHASE):
        run_widened(kind, x, d["s"], config(engine, WT), f"{kind} wt engine {engine}")
        run_widened(kind, x, d["a2"], config(engine, WT), f"{kind} wt engine {engine} scaled", alpha=E.ALPHAS[2][1])


# ------------------------------------------------------- 2. counts and offsets

@pytest.mark.parametrize("engine", [TILE, PHASE], ids=["tile", "phase"])
@KINDS
def test_counts_around_every_boundary(kind, engine):
    """Every count around a packet, a tile and a chunk, the output 0-3
    elements past a 16-byte boundary (head 0, 3, 2, 1 scalars), the inputs at
    mutually different offsets that change from count to count; count 0 is a
    no-op that leaves the output alone."""
    cfg = config(engine)
    n = 3
    # from column 4 on: the hostile generators' first four columns hold two NaN
    # classes, more than NAN_CAP of a compute of three to five elements
    big = E.inputs(kind, n, max(COUNTS) + 4)[:, 4:]
    for i, count in enumerate(COUNTS):
        alpha = None if i % 2 else 0.5
        if count == 0:  # placed inputs of four elements, none of them asked for
            ins = place_inputs(kind, big[:, :4], in_offsets(kind, n))
            run_widened(kind, big[:, :0], np.empty(0, np.float32), cfg, f"{kind} count=0", ins=ins, count=0, alpha=alpha)
            continue
        x = big[:, :count]
        run_widened(kind, x, E.widened(kind, x, alpha), cfg, f"{kind} count={count} off={i % 4}", out_off=i % 4, shift=i,
                    alpha=alpha)
        if count in (5, 4097, 32769):  # every output offset at a count that has a head, a body and a tail
            for off in range(4):
                run_widened(kind, x, E.widened(kind, x, 1.0 / 3.0), cfg, f"{kind} count={count} off={off} scaled",
                            alpha=1.0 / 3.0, out_off=off, shift=off + 3)


@KINDS
def test_every_input_offset(kind):
    """One input swept over every offset of its range (0-7 elements, FP8 0-15
    bytes) against two fixed ones, nine inputs: a full group and a remainder."""
    n, count = 9, TILE_ELEMS + 7
    x = E.inputs(kind, n, count)
    exp = E.widened(kind, x)
    span = 8 if E.ESZ[kind] == 2 else 16
    for off in range(span):
        offs = [(off + 3 * k) % span for k in range(n)]
        ins = place_inputs(kind, x, offs)
        run_widened(kind, x, exp, config(TILE), f"{kind} input offsets {offs}", ins=ins, out_off=off % 4)


# ------------------------------------------------------------------ 3. inputs

@pytest.mark.parametrize("engine", [TILE, PHASE], ids=["tile", "phase"])
@KINDS
def test_every_n(kind, engine):
    """n = 0 (writes +0, scaled a zero with alpha's sign), 1, 2, 3, 8, 9, 17
    and 65, which runs the plan kernel from an uploaded pointer table."""
    cfg = config(engine)
    count = COUNT if engine == TILE else CHUNK_ELEMS + 37
    for n in (0, 1, 2, 3, 8, 9, 17, 65):
        x = E.inputs(kind, n, count)
        run_widened(kind, x, E.widened(kind, x, count=count), cfg, f"{kind} n={n}", count=count)
        exp = E.widened(kind, x, -1.0 / 1024.0, count=count)
        if n == 0:
            assert (exp.view(np.uint32) == 0x80000000).all()
        run_widened(kind, x, exp, cfg, f"{kind} n={n} scaled", alpha=-1.0 / 1024.0, count=count)


# ------------------------------------------------------------- 4. scale = 1.0

@ENGINES3
@KINDS
def test_unscaled_equals_scale_one_word_for_word(kind, engine):
    """The unscaled form against scale = 1.0: the same words, NaN payloads
    included (for every non-NaN s, fl32(s * 1.0f) is s)."""
    for n in (2, 9):
        x = E.inputs(kind, n, COUNT)
        E.assert_nan_cap(E.widened(kind, x))
        ins = place_inputs(kind, x, in_offsets(kind, n))
        words = []
        for alpha in (None, 1.0):
            buf, out = new_output(COUNT, 1)
            hiccl_amd.reduce_widened(out, ins, config=config(engine), scale=alpha)
            torch.cuda.synchronize()
            words.append(out.cpu().numpy().view(np.uint32))
        assert np.array_equal(words[0], words[1]), f"{kind} n={n}: unscaled and scale=1.0 differ"
        E.assert_equal(words[0].view(np.float32), E.widened(kind, x), f"{kind} n={n}")


# -------------------------------------------------------------- 5. patterns

@KINDS
def test_every_pattern_against_sixteen_addends(kind):
    """Every 16-bit pattern (bf16, f16) or byte (FP8) as input 0 against each
    of 16 addends as input 1: the words hash to the reference's
    (manifest_widen.json)."""
    with open(os.path.join(GOLDEN, "manifest_widen.json")) as fh:
        want = json.load(fh)["patterns"][kind]
    exp = E.patterns_expected(kind)
    E.assert_nan_cap(exp)
    assert E.words_hash(exp) == want
    rows = []
    for i in range(16):
        x = E.pattern_inputs(kind, i)
        ins = place_inputs(kind, x, [0, 1])
        buf, out = new_output(x.shape[1], i % 4)
        hiccl_amd.reduce_widened(out, ins, config=config(TILE if i % 2 else PHASE))
        torch.cuda.synchronize()
        rows.append(out.cpu().numpy())
        E.assert_equal(rows[-1], exp[i], f"{kind} addend {i}")
    assert E.words_hash(np.stack(rows)) == want


# ------------------------------------------------------- 6. the f32 reduction

@ENGINES3
@KINDS
def test_equals_the_f32_sum_of_the_converted_inputs(kind, engine):
    """hiccl_amd.reduce in f32 on x.float() inputs on the same device: both
    are in-order f32 sums from +0."""
    n, count = 8, TILE_ELEMS + CHUNK_ELEMS + 5
    x = E.inputs(kind, n, count)
    E.assert_nan_cap(E.widened(kind, x))
    ins = place_inputs(kind, x, in_offsets(kind, n))
    floats = [t.float() for t in ins]
    want = torch.empty(count, dtype=torch.float32, device=DEV)
    hiccl_amd.reduce(want, floats, config=config(engine))
    buf, out = new_output(count, 2)
    hiccl_amd.reduce_widened(out, ins, config=config(engine))
    torch.cuda.synchronize()
    E.assert_equal(want.cpu().numpy(), E.widened(kind, x), f"{kind}: the f32 path")
    check_output(buf, 2, count, want.cpu().numpy(), f"{kind}: widened against reduce(f32) on x.float()")


# -------------------------------------------------------------------- 7. plans

PLAN_SHAPES = ((3, 4097), (1, 5), (9, 32768 + 3), (17, 1000), (2, 4096))  # (n, count) of the five computes


def _plan_case(kind, comp):
    """Adds the five computes; returns [(buffer, out offset, count, inputs as arrays)]."""
    cases = []
    for j, (n, count) in enumerate(PLAN_SHAPES):
        x = E.inputs(kind, n, count)
        ins = place_inputs(kind, x, in_offsets(kind, n, j))
        buf, out = new_output(count, j % 4)
        comp.add(ins, out, count, compid=0)
        cases.append((buf, j % 4, count, x))
    return cases


def _check_plan(kind, cases, alpha, what):
    torch.cuda.synchronize()
    for j, (buf, off, count, x) in enumerate(cases):
        check_output(buf, off, count, E.widened(kind, x, alpha), f"{kind} {what} compute {j}")


@pytest.mark.parametrize("peer", [0, L.HICCL_PEER_STORES, L.HICCL_PEER_LOADS, L.HICCL_PEER_STORES | L.HICCL_PEER_LOADS],
                         ids=["plain", "peer-stores", "peer-loads", "peer-both"])
@pytest.mark.parametrize("engine", [TILE, PHASE], ids=["tile", "phase"])
@KINDS
def test_plan_of_five_computes(kind, engine, peer):
    """Compute(out_dtype=torch.float32): five computes of unequal n and count
    in one launch through start / wait, compared compute by compute; then
    scaled, cleared, and one launch per compute (launch_each)."""
    for n, count in PLAN_SHAPES:
        E.assert_nan_cap(E.widened(kind, E.inputs(kind, n, count)))
    comp = hiccl_amd.Compute(E.TORCH[kind], device=0, out_dtype=torch.float32, engine=engine)
    try:
        assert L.lib().hiccl_reduce_plan_out_dtype(comp._plan) == L.HICCL_FLOAT32
        if peer:
            comp.set_peer(peer)
        cases = _plan_case(kind, comp)
        assert comp.numcomp == 5
        assert comp.bytes() == sum(c * (n * E.ESZ[kind] + 4) for n, c in PLAN_SHAPES)
        comp.start()
        comp.wait()
        assert comp.engine() == engine
        _check_plan(kind, cases, None, "plan")
        comp.set_scale(1.0 / 3.0)
        comp.start()
        comp.wait()
        _check_plan(kind, cases, 1.0 / 3.0, "scaled plan")
        if not peer:
            comp.start(each=True)
            comp.wait()
            _check_plan(kind, cases, 1.0 / 3.0, "scaled launch_each")
            comp.set_scale(None)
            comp.start(each=True)
            comp.wait()
            _check_plan(kind, cases, None, "launch_each")
        comp.set_scale(None)
        comp.enqueue()
        _check_plan(kind, cases, None, "enqueue after clear_scale")
    finally:
        comp.close()


@KINDS
def test_plan_refuses_an_overlapping_output_and_a_program(kind):
    comp = hiccl_amd.Compute(E.TORCH[kind], device=0, out_dtype=torch.float32)
    try:
        raw = torch.zeros(1024, dtype=torch.uint8, device=DEV)
        out = raw[:256].view(torch.float32)
        x = raw[128:128 + 64 * E.ESZ[kind]].view(E.TORCH[kind])
        with pytest.raises(hiccl_amd.HicclError, match="overlaps out"):
            comp.add([x], out, 64, compid=0)
        with pytest.raises(hiccl_amd.HicclError, match="overlaps out"):
            hiccl_amd.reduce_widened(out, [x], count=64)
        y = raw[512:512 + 64 * E.ESZ[kind]].view(E.TORCH[kind])
        comp.add([y], out, 64, compid=0)
        prog = hiccl_amd.Program(E.TORCH[kind], device=0)
        try:
            with pytest.raises(hiccl_amd.HicclError, match="widened"):
                prog.add_plan(comp)
        finally:
            prog.close()
    finally:
        comp.close()


# ------------------------------------------------------------------- 8. graph

@KINDS
def test_captured_and_replayed_call(kind):
    """A one-shot call with n = 8 captured into a graph and replayed once on
    new input values."""
    n, alpha = 8, 0.5
    x = E.inputs(kind, n, COUNT)
    y = np.roll(x, 5, axis=1)
    E.assert_nan_cap(E.widened(kind, y, alpha))
    ins = place_inputs(kind, x, in_offsets(kind, n))
    buf, out = new_output(COUNT, 1)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hiccl_amd.reduce_widened(out, ins, scale=alpha)  # warm-up outside capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        hiccl_amd.reduce_widened(out, ins, scale=alpha)
    for t, r in zip(ins, y):
        t.view(torch.uint8).copy_(torch.from_numpy(np.ascontiguousarray(r).view(np.uint8).copy()))
    out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    check_output(buf, 1, COUNT, E.widened(kind, y, alpha), f"{kind} replay")


# --------------------------------------------------------------------- 9. C++

@pytest.mark.parametrize("kind", ["bf16", "e4m3"])
def test_cpp_widen_compute_on_gpu(kind, tmp_path):
    """build/widen_sum_hip (tests/cpp/widen_sum.cpp built against
    include/hiccl.h by make): WidenCompute<bf16> / WidenCompute<f8e4m3> through the
    batched plan kernel, plain, scaled and after clear_scale, against the
    fixtures."""
    exe = os.path.join(ROOT, "build", "widen_sum_hip")
    assert os.path.exists(exe), "run make"
    n, alpha = 9, 1.0 / 3.0
    d = fixture(kind)[f"n{n}"]
    i = [a for _, a in E.ALPHAS].index(alpha)
    for exp in (d["s"], d[f"a{i}"]):
        E.assert_nan_cap(exp)
    inp, out = tmp_path / f"{kind}.in", tmp_path / f"{kind}.out"
    np.ascontiguousarray(E.inputs(kind, n)).tofile(inp)
    p = subprocess.run([exe, kind, str(inp), str(out), str(n), str(COUNT),
                        float(alpha).hex()], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "widen_sum: PASSED" in p.stdout, p.stdout + p.stderr
    E.assert_equal(np.fromfile(str(out) + ".plain", np.float32), d["s"], f"WidenCompute<{kind}> plain")
    E.assert_equal(np.fromfile(str(out), np.float32), d[f"a{i}"], f"WidenCompute<{kind}> scaled")
    E.assert_equal(np.fromfile(str(out) + ".cleared", np.float32), d["s"], f"WidenCompute<{kind}> cleared")


# ---------------------------------------------------------- 10. Python layer

def test_python_refusals_that_need_a_tensor():
    bf = torch.zeros(16, dtype=torch.bfloat16, device=DEV)
    hf = torch.zeros(16, dtype=torch.float16, device=DEV)
    f32 = torch.zeros(16, dtype=torch.float32, device=DEV)
    with pytest.raises(TypeError, match="dtype"):  # reduce() keeps refusing mixed dtypes
        hiccl_amd.reduce(f32, [bf])
    with pytest.raises(TypeError, match="writes torch.float32"):
        hiccl_amd.reduce_widened(bf, [bf])
    with pytest.raises(TypeError, match="writes torch.float32"):
        hiccl_amd.reduce_widened(torch.zeros(16, dtype=torch.float64, device=DEV), [bf])
    with pytest.raises(TypeError, match="widened sums take"):
        hiccl_amd.reduce_widened(f32, [torch.zeros(16, device=DEV)])
    with pytest.raises(TypeError, match="!= inputs"):
        hiccl_amd.reduce_widened(f32, [bf, hf])
    with pytest.raises(ValueError, match="at least one input"):
        hiccl_amd.reduce_widened(f32, [])
    with pytest.raises(ValueError, match="finite"):
        hiccl_amd.reduce_widened(f32, [bf], scale=float("nan"))
    with pytest.raises(ValueError, match="accumulates in f32"):
        hiccl_amd.reduce_widened(f32, [bf], config=dict(acc=L.HICCL_ACC_WIDE))
    with pytest.raises(ValueError, match="elements"):
        hiccl_amd.reduce_widened(f32, [bf[:8]])
    with pytest.raises(hiccl_amd.HicclError, match="unsupported config"):
        hiccl_amd.reduce_widened(f32, [bf], config=dict(engine=TILE, unroll=2))
    assert (f32 == 0).all()
