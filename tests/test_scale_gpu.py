"""GPU tier of the scaled sums (out = finish(sum, alpha): hiccl_reduce_scaled,
hiccl_reduce_plan_set_scale, hiccl_host_pipe_set_scale) on every layer that
takes them, bit for bit against the stored fixtures
(tests/golden/reduce_scale_*.npz: the reference's reduce_kernel, finished by the
generator) or the NumPy restatement the fixtures pin (tests/scale_expected.py);
a NaN output compares by NaN-ness.

  1. one-shot, per dtype: TILE and PHASE forced and AUTO, write-through by size
     and nt on request, both accumulators for the 2-byte types, output and
     inputs misaligned (scalar head and tail), n = 0, in place, n = 65 (the
     plan kernel); alpha = 1.0 equals the existing unscaled sum's words;
  2. plans: computes of mixed n in one launch, set_scale after the first
     launch, then clear_scale; launch_each; both peer policies;
  3. a scaled plan is refused by a program (the unscaled program tests of the
     existing suite stay as they are);
  4. the host pipe;  5. every 16-bit pattern times every alpha;
  6. one captured and twice-replayed one-shot call with n = 8;
  7. Compute<float> / Compute<bf16>::set_scale from tests/cpp/scale_compute.cpp;
  8. the Python refusals that need a tensor.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import hiccl_amd
import scale_expected as E
import test_ops_gpu as G
from conftest import GOLDEN, ROOT, load_golden
from hiccl_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = G.DEV
TILE, PHASE, AUTO = L.HICCL_ENGINE_TILE, L.HICCL_ENGINE_PHASE, L.HICCL_ENGINE_AUTO
WIDE = L.HICCL_ACC_WIDE
NT = 2  # hiccl_reduce_config_t.store_policy: nt stores whatever the launch's size
COUNT = E.COUNT
KINDS = {k: G.KINDS[k] for k in E.KINDS}
# (kind, wide): both accumulators for the 2-byte types
MODES = [pytest.param(k, w, id=f"{k}{'-wide' if w else ''}") for k in E.KINDS for w in ((False, True) if k in E.HALVES
                                                                                       else (False,))]
ENGINES3 = pytest.mark.parametrize("engine", [TILE, PHASE, AUTO], ids=["tile", "phase", "auto"])
per_packet, phase_chunk = G.per_packet, G.phase_chunk
to_dev, to_host, place_inputs, new_output, check_output = G.to_dev, G.to_host, G.place_inputs, G.new_output, G.check_output


@functools.lru_cache(maxsize=None)
def fixture(kind):
    """{case: {part: stored output}} of the kind's fixture."""
    return load_golden(f"reduce_scale_{kind}")


def stored(kind, n, i, wide):
    return fixture(kind)[f"hostile_n{n}"][f"{'w' if wide else 'a'}{i}"]


def config(engine, wide, store=0):
    cfg = dict(engine=engine)
    if wide:
        cfg["acc"] = WIDE
    if store:
        cfg["store_policy"] = store
    return cfg


def gpu_scaled(kind, alpha, x, exp, cfg, what, out_past=1, count=None, in_offs=None, ins=None):
    """One-shot scaled sum of the rows of x, the output `out_past` elements
    past a 16-byte boundary, input k at element offset k + 2 (or in_offs[k];
    `ins`: the rows already placed); checks the words and the guards around
    the output."""
    n = x.shape[0]
    count = x.shape[1] if count is None else count
    per = per_packet(kind)
    if ins is None:
        ins = place_inputs(kind, x, in_offs if in_offs is not None else G.in_offsets(n, per))
    ob = new_output(kind, count + 2 * per, 0)
    out_off = G.aligned_offset(ob, KINDS[kind][2]) + out_past
    hiccl_amd.reduce(ob[out_off:out_off + count], [b[o:o + count] for b, o in ins], count=count, config=cfg, scale=alpha)
    torch.cuda.synchronize()
    check_output(kind, ob, out_off, count, exp, what)


# ---------------------------------------------------------------- 1. one-shot

@pytest.mark.parametrize("store", [0, NT], ids=["wt-by-size", "nt"])
@ENGINES3
@pytest.mark.parametrize("kind,wide", MODES)
def test_one_shot_fixture_cases(kind, wide, engine, store):
    """Every stored case (n = 1, 2, 3, 8, 9, 17) under every alpha, the output
    one element past 16 bytes and input k offset by k + 2 elements, so head
    and tail run the scalar path; and n = 0, which writes finish(+0, alpha): a
    zero with alpha's sign."""
    cfg = config(engine, wide, store)
    for n in E.NS:
        x = E.hostile(kind, n)
        ins = place_inputs(kind, x, G.in_offsets(n, per_packet(kind)))
        for i, (name, alpha) in enumerate(E.ALPHAS):
            gpu_scaled(kind, alpha, x, stored(kind, n, i, wide), cfg, f"{kind} n={n} alpha {name} {cfg}", ins=ins)
    sign = 1 << (8 * KINDS[kind][2] - 1)
    for name, alpha in E.ALPHAS:
        exp = E.scaled(kind, np.zeros((0, 37), E.carrier(kind)), alpha, wide, count=37)
        assert (E.bits_of(kind, exp) == (sign if np.signbit(alpha) else 0)).all(), name
        gpu_scaled(kind, alpha, np.zeros((0, 37), E.carrier(kind)), exp, cfg, f"{kind} n=0 alpha {name}", count=37)


@pytest.mark.parametrize("kind,wide", MODES)
def test_alpha_one_gives_the_unscaled_sums_words(kind, wide):
    """alpha = 1.0 still multiplies, and gives the plain sum's words: the
    stored a0 / w0 outputs against the unscaled call on the GPU, and against
    the existing fixtures where they hold the same inputs (reduce_f16's
    hostile cases)."""
    cfg = config(AUTO, wide)
    for n in E.NS:
        x = E.hostile(kind, n)
        ins = [to_dev(kind, r) for r in x]
        out = new_output(kind, COUNT, 0)[:COUNT]
        hiccl_amd.reduce(out, ins, config=cfg)
        torch.cuda.synchronize()
        plain = to_host(kind, out)
        assert E.bits_equal(kind, plain, stored(kind, n, 0, wide)), f"{kind} n={n}: {E.first_mismatch(kind, plain, stored(kind, n, 0, wide))}"
        gpu_scaled(kind, 1.0, x, plain, cfg, f"{kind} n={n} alpha 1 against the unscaled call")
    if kind == "f16" and not wide:
        old = load_golden("reduce_f16")
        for n in E.NS:
            d = old[f"hostile_n{n}"]
            assert np.array_equal(d["in"], E.hostile("f16", n))
            assert E.bits_equal("f16", d["out"], stored("f16", n, 0, False))


@pytest.mark.parametrize("engine", [TILE, PHASE, AUTO], ids=["tile", "phase", "auto"])
@pytest.mark.parametrize("kind", E.KINDS)
def test_alpha_one_on_the_existing_sum_fixtures(kind, engine):
    """Every case of the EXISTING unscaled fixtures (reduce_f32 / _f64 / _bf16
    / _f16.npz: their own stored inputs -- rand_*, special_*, wide_*, tamed_*,
    hostile_*, every_pattern -- and the reference's stored sums): the GPU's
    reduce(..., scale=1.0) on the stored inputs gives the stored `out` words, a
    NaN by NaN-ness.  (Those fixtures hold the native accumulator's sums only;
    the f32 accumulator at alpha = 1 is checked against the unscaled wide call
    above.)"""
    cases = load_golden(f"reduce_{kind}")
    assert len(cases) >= 13
    ran = 0
    for name, d in cases.items():
        x, want = d["in"], d["out"]
        n, count = x.shape
        if count == 0:
            continue
        assert want.shape == (count,)
        ins = [to_dev(kind, r) for r in x]
        out = new_output(kind, count, 0)[:count]
        hiccl_amd.reduce(out, ins, count=count, config=dict(engine=engine), scale=1.0)
        torch.cuda.synchronize()
        got = to_host(kind, out)
        assert E.bits_equal(kind, got, want), f"{kind} {name}: {E.first_mismatch(kind, got, want)}"
        ran += 1
    assert ran >= 13


@pytest.mark.parametrize("engine", [TILE, PHASE], ids=["tile", "phase"])
@pytest.mark.parametrize("kind,wide", MODES)
def test_phase_two_chunks_in_place_and_65_inputs(kind, wide, engine):
    """More than one workgroup's unit (two phased chunks + 37 elements) with
    the output aliasing input 1 exactly; n = 65, which runs the plan kernel."""
    cfg = config(engine, wide)
    alpha = 0.7
    count = 2 * phase_chunk(kind) // (2 if wide else 1) + 37
    x = E.hostile(kind, 3, count)
    ins = [to_dev(kind, r) for r in x]
    hiccl_amd.reduce(ins[1], ins, config=cfg, scale=alpha)  # in place
    torch.cuda.synchronize()
    got, exp = to_host(kind, ins[1]), E.scaled(kind, x, alpha, wide)
    assert E.bits_equal(kind, got, exp), f"{kind} in place: {E.first_mismatch(kind, got, exp)}"
    n = 65
    count = COUNT if engine == TILE else phase_chunk(kind) + 37
    x = E.hostile(kind, n, count)
    gpu_scaled(kind, -1.0 / 1024.0, x, E.scaled(kind, x, -1.0 / 1024.0, wide), cfg, f"{kind} n=65")


@pytest.mark.parametrize("kind,wide", MODES)
def test_element_offsets_and_scalar_only_computes(kind, wide):
    """Output and inputs at element offsets 0-7 past a 16-byte boundary, and a
    compute shorter than one packet (the scalar path alone, sstore)."""
    cfg = config(TILE, wide)
    x = E.hostile(kind, 3)
    exp = E.scaled(kind, x, 0.1, wide)
    for off in range(0, 8, 3):
        gpu_scaled(kind, 0.1, x, exp, cfg, f"{kind} off={off}", in_offs=[(off + k) % 8 for k in range(3)], out_past=off)
    short = per_packet(kind) - 1
    for n in (2, 9):
        x = E.hostile(kind, n, 64)[:, :short]
        for name, alpha in E.ALPHAS:
            gpu_scaled(kind, alpha, x, E.scaled(kind, x, alpha, wide), cfg, f"{kind} scalar-only n={n} alpha {name}")


# ------------------------------------------------------------------ 2. plans

PLAN_N = (2, 1, 3, 9, 17)


@functools.lru_cache(maxsize=None)
def plan_batch(kind):
    counts = (per_packet(kind) - 1, 4097, 4102, 8200, phase_chunk(kind) + 5)
    return [E.hostile(kind, n, count) for n, count in zip(PLAN_N, counts)]


@pytest.mark.parametrize("variant", list(G.PLAN_VARIANTS))
@pytest.mark.parametrize("engine", [TILE, PHASE], ids=["tile", "phase"])
@pytest.mark.parametrize("kind,wide", MODES)
def test_plan_mixed_computes_set_and_clear_scale(kind, wide, engine, variant):
    """Five computes (n = 2, 1, 3, 9, 17; less than a packet to a phased chunk
    + 5 elements) in ONE launch: unscaled first, then set_scale on the
    launched plan, another alpha, and clear_scale; under every peer policy, and
    as one launch per compute (launch_each honours the scale)."""
    peer, each = G.PLAN_VARIANTS[variant]
    comp = hiccl_amd.Compute(KINDS[kind][0], device=0, engine=engine, acc=WIDE if wide else L.HICCL_ACC_NATIVE)
    if peer:
        comp.set_peer(peer)
    outs, per = [], per_packet(kind)
    for c, x in enumerate(plan_batch(kind)):
        n, count = x.shape
        ob = new_output(kind, count + per, 0)
        off = G.aligned_offset(ob, KINDS[kind][2]) + c % 2
        comp.add(place_inputs(kind, x, G.in_offsets(n, per)), (ob, off), count, compid=0)
        outs.append((ob, off, count))
    assert comp.scale() is None
    for step, alpha in enumerate((None, 1.0 / 3.0, 1e30, None, 0.0)):
        comp.set_scale(alpha)
        assert comp.scale() == alpha
        for ob, _, _ in outs:
            ob.view(torch.uint8).fill_(G.SENTINEL)
        comp.start(each=each)
        comp.wait()
        if not each:
            assert comp.engine() == engine
        for c, ((ob, off, count), x) in enumerate(zip(outs, plan_batch(kind))):
            exp = E.plain_sum(kind, x, wide) if alpha is None else E.scaled(kind, x, alpha, wide)
            check_output(kind, ob, off, count, exp, f"{kind} {variant} step {step} alpha {alpha} compute {c}")
    comp.close()


def test_plan_refusals_and_the_hosts_auto_answer():
    """A scaled plan refuses another operator, a plan under another operator
    refuses a scale, integer plans refuse it; an AUTO scaled plan takes the
    engine and store form hiccl_reduce_auto_choice_scaled answers."""
    comp = hiccl_amd.Compute(torch.float32, device=0, scale=0.5)
    with pytest.raises(hiccl_amd.HicclError, match="scaled plan sums"):
        comp.set_op(L.HICCL_OP_MAX)
    comp.set_scale(None)
    comp.set_op(L.HICCL_OP_MAX)
    with pytest.raises(ValueError, match="only sums"):
        comp.set_scale(2.0)
    a = ctypes.c_double(2.0)
    assert L.lib().hiccl_reduce_plan_set_scale(comp._plan, ctypes.byref(a)) == 1 and "HICCL_OP_SUM" in L.last_error()
    comp.close()
    with pytest.raises(TypeError, match="floating"):
        hiccl_amd.Compute(torch.int32, device=0, scale=0.5)
    # a config whose shape only the tuned sums have: refused by set_scale itself, not at the next launch
    for unroll in (1, 2, 8, 16):
        comp = hiccl_amd.Compute(torch.float32, device=0, config=dict(engine=TILE, unroll=unroll))
        with pytest.raises(hiccl_amd.HicclError, match="plan_set_scale.*shape the scaled kernels lack"):
            comp.set_scale(0.5)
        assert comp.scale() is None
        comp.set_config(dict(engine=TILE, unroll=4))
        comp.set_scale(0.5)
        with pytest.raises(hiccl_amd.HicclError, match="plan_set_config"):
            comp.set_config(dict(engine=TILE, unroll=unroll))
        comp.close()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for n, count in ((3, 4102), (2, 1 << 22)):
        x = E.hostile("f32", n, 4102)
        reps = -(-count // 4102)
        rows = [np.tile(r, reps)[:count] for r in x]
        comp = hiccl_amd.Compute(torch.float32, device=0, scale=0.5)
        out = new_output("f32", count, 0)[:count]
        comp.add([to_dev("f32", r) for r in rows], out, count, compid=0)
        comp.start()
        comp.wait()
        want = hiccl_amd.auto_choice(torch.float32, count, n, cus=cus, scale=True)
        assert (comp.engine(), comp.store_policy()) == (want["engine"], want["store_policy"]), (count, want)
        got, exp = to_host("f32", out), np.tile(E.scaled("f32", x, 0.5), reps)[:count]
        assert E.bits_equal("f32", got, exp), E.first_mismatch("f32", got, exp)
        comp.close()


# --------------------------------------------------------------- 3. programs

def test_program_refuses_a_scaled_plan():
    """hiccl_program_add_plan of a scaled plan is refused; the same plan with
    its scale cleared joins and the program gives the plain sums."""
    x = E.hostile("f32", 3)
    red = hiccl_amd.Compute(torch.float32, device=0, scale=0.25)
    out = new_output("f32", COUNT, 0)[:COUNT]
    red.add([to_dev("f32", r) for r in x], out, COUNT, compid=0)
    prog = hiccl_amd.Program(torch.float32, device=0)
    with pytest.raises(hiccl_amd.HicclError, match="scaled plan"):
        prog.add_plan(red)
    assert prog.units() == 0
    red.set_scale(None)
    prog.add_plan(red)
    prog.launch(timeout_s=5.0)
    torch.cuda.synchronize()
    got = to_host("f32", out)
    assert E.bits_equal("f32", got, E.plain_sum("f32", x)), E.first_mismatch("f32", got, E.plain_sum("f32", x))
    prog.close()
    red.close()


# -------------------------------------------------------------- 4. host pipe

def test_host_pipe_scaled():
    """3 pinned host inputs of 300,000 f32 at 256 KiB chunks, depth 2, scaled
    by 1/3; then the scale cleared."""
    n, count = 3, 300_000
    x = E.hostile("f32", n, count)
    ins = [torch.from_numpy(np.array(x[k])).pin_memory() for k in range(n)]
    out = torch.zeros(count, dtype=torch.float32).pin_memory()
    pipe = hiccl_amd.HostPipe(torch.float32, device=0, chunk_bytes=256 << 10, depth=2, scale=1.0 / 3.0)
    pipe.reduce(out, ins)
    exp = E.scaled("f32", x, 1.0 / 3.0)
    assert E.bits_equal("f32", out.numpy(), exp), E.first_mismatch("f32", out.numpy(), exp)
    pipe.set_scale(None)
    pipe.reduce(out, ins)
    assert E.bits_equal("f32", out.numpy(), E.plain_sum("f32", x))
    pipe.close()
    with pytest.raises(TypeError, match="floating"):
        hiccl_amd.HostPipe(torch.int32, device=0, scale=2.0)


# ------------------------------------------------------ 5. every bit pattern

@functools.lru_cache(maxsize=None)
def pattern_words(kind, wide):
    """The restatement's (11, 65536) words, checked against the generator's hash first."""
    with open(os.path.join(GOLDEN, "manifest_scale.json")) as fh:
        want = json.load(fh)["patterns"][f"{kind}{'_wide' if wide else ''}"]
    words = E.patterns_expected(kind, wide)
    assert E.words_hash(kind, words) == want, f"{kind}: scale_expected no longer gives the generator's words"
    return words


@pytest.mark.parametrize("engine", [TILE, PHASE], ids=["tile", "phase"])
@pytest.mark.parametrize("wide", [False, True], ids=["native", "wide"])
@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_every_pattern_times_every_alpha(kind, wide, engine):
    """One n = 1 launch per alpha over all 65,536 patterns."""
    words = pattern_words(kind, wide)
    pats = to_dev(kind, E.ALL_PATTERNS)
    for i, (name, alpha) in enumerate(E.ALPHAS):
        out = new_output(kind, 1 << 16, 0)[:1 << 16]
        hiccl_amd.reduce(out, [pats], config=config(engine, wide), scale=alpha)
        torch.cuda.synchronize()
        got = to_host(kind, out)
        assert E.bits_equal(kind, got, words[i]), f"{kind} alpha {name}: {E.first_mismatch(kind, got, words[i])}"


# ------------------------------------------------------------------ 6. graph

def test_captured_and_twice_replayed_scaled_call():
    """A scaled one-shot call with n = 8 captured into a graph (alpha travels
    in the kernel arguments) and replayed twice on new input values."""
    n, alpha = 8, 1.0 / 8.0
    x = E.hostile("f32", n)
    ins = [to_dev("f32", r) for r in x]
    out = torch.empty(COUNT, dtype=torch.float32, device=DEV)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hiccl_amd.reduce(out, ins, scale=alpha)  # warm-up outside capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        hiccl_amd.reduce(out, ins, scale=alpha)
    for rep in range(2):
        y = np.roll(x, rep + 1, axis=1)
        for t, r in zip(ins, y):
            t.copy_(to_dev("f32", r))
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        got, exp = to_host("f32", out), E.scaled("f32", y, alpha)
        assert E.bits_equal("f32", got, exp), f"replay {rep}: {E.first_mismatch('f32', got, exp)}"


# -------------------------------------------------------------------- 7. C++

def test_cpp_compute_set_scale_on_gpu(tmp_path):
    """build/scale_compute_hip (tests/cpp/scale_compute.cpp, built by make):
    Compute<float> and Compute<HiCCL::bf16> with set_scale / clear_scale on
    the GPU give the fixtures' words, as the host port does."""
    from test_scale_cpu import check_scale_compute
    for port in ("hip", "host"):
        exe = os.path.join(ROOT, "build", f"scale_compute_{port}")
        assert os.path.exists(exe), "run make"
        d = tmp_path / port
        d.mkdir()
        check_scale_compute(exe, d, timeout=60)


# ------------------------------------------------------- 8. Python refusals

def test_python_layer_refusals_on_tensors():
    f = torch.ones(64, dtype=torch.float32, device=DEV)
    out = torch.empty_like(f)
    i = torch.ones(64, dtype=torch.int32, device=DEV)
    with pytest.raises(TypeError, match="floating"):
        hiccl_amd.reduce(torch.empty_like(i), [i, i], scale=0.5)
    with pytest.raises(TypeError, match="floating"):
        hiccl_amd.reduce(torch.empty(64, dtype=torch.uint8, device=DEV), [torch.ones(64, dtype=torch.uint8, device=DEV)],
                         scale=0.5)
    with pytest.raises(ValueError, match="only sums"):
        hiccl_amd.reduce(out, [f, f], op=L.HICCL_OP_MAX, scale=0.5)
    for bad in (float("inf"), float("-inf"), float("nan")):
        with pytest.raises(ValueError, match="finite"):
            hiccl_amd.reduce(out, [f, f], scale=bad)
    with pytest.raises(TypeError, match="real number"):
        hiccl_amd.reduce(out, [f, f], scale="0.5")
    for half in (np.float32(0.5), np.float64(0.5), torch.tensor(0.5), 1 / np.float32(2)):  # any real scalar
        hiccl_amd.reduce(out, [f, f], scale=half)
        torch.cuda.synchronize()
        assert (out == 1.0).all()
    # finite as a double, infinite as a float: refused by the library for the 4-byte type
    with pytest.raises(hiccl_amd.HicclError, match="finite as a float"):
        hiccl_amd.reduce(out, [f, f], scale=1e300)
    d = torch.ones(64, dtype=torch.float64, device=DEV)
    od = torch.empty_like(d)
    hiccl_amd.reduce(od, [d, d], scale=1e300)  # f64 multiplies by the double itself
    torch.cuda.synchronize()
    assert od[0].item() == 2e300
    hiccl_amd.reduce(out, [f, f], scale=1e-60)  # underflows to zero as a float: allowed
    torch.cuda.synchronize()
    assert out.abs().max().item() == 0.0
