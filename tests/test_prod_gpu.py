"""GPU tier of the PROD / BAND / BOR / BXOR operators (hiccl_op_t) on every
layer that takes them, bit for bit against the stored fixtures
(tests/golden/reduce_prod_*.npz: the reference's reduce_kernel on prodof /
bandof / borof / bxorof) or the NumPy restatement the fixtures pin
(tests/prod_expected.py); a NaN output compares by NaN-ness, and at most 1/8 of
any hostile case's outputs are NaN (the classes one_nan and inf_times_zero).

  1. one-shot, TILE and PHASE forced, write-through by size and nt on request:
     the fixtures' cases (n in 1, 2, 3, 8, 9, 17 at 17 * 241 + 5 elements,
     integers 17 * 61 + 5) and n = 0 (the identity: 1 / all-ones / 0); two
     phased chunks + 37 elements under PHASE; element offsets 0-7 on inputs
     and output; every class on a compute shorter than one packet (the scalar
     head and tail alone); n = 65, the pointer-table path;
  2. plans: five ragged computes in one launch under every peer policy and one
     launch per compute, the op switched on a launched plan, engine and store
     form equal to the host's auto_choice answer;
  3. programs: a program whose first reducing plan is PROD; SUM refused;
  4. the host pipe;  5. every 16-bit pattern times 16 multipliers;
  6. the C++ wrappers: Compute<prodof<float>> / Compute<prodof<bf16>> and
     2-rank Comm<prodof<float>> / Comm<bxorof<uint64_t>>;
  7. the Python layer's refusals that need a tensor.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import hiccl_amd
import hostile_prod as HP
import prod_expected as E
import test_ops_gpu as G
from conftest import GOLDEN, ROOT, load_golden
from hiccl_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = G.DEV
TILE, PHASE = L.HICCL_ENGINE_TILE, L.HICCL_ENGINE_PHASE
SUM, MAX = L.HICCL_OP_SUM, L.HICCL_OP_MAX
PROD, BAND, BOR, BXOR = L.HICCL_OP_PROD, L.HICCL_OP_BAND, L.HICCL_OP_BOR, L.HICCL_OP_BXOR
NT = 2  # hiccl_reduce_config_t.store_policy: nt stores whatever the launch's size
NS = [0, 1, 2, 3, 8, 9, 17]
COUNT = 17 * 241 + 5
INT_COUNT = 17 * 61 + 5
NAN_CAP = 1.0 / 8
KINDS = G.KINDS
KIND_OP = [pytest.param(k, o, id=f"{k}-{o}") for k in KINDS for o in E.ops_of(k)]
ENGINES = G.ENGINES
per_packet, phase_chunk = G.per_packet, G.phase_chunk
to_dev, to_host, place_inputs, new_output, check_output = G.to_dev, G.to_host, G.place_inputs, G.new_output, G.check_output


def inputs(kind, n, count, shift=0, seed=0):
    """(n, count) product-hostile inputs of a floating kind, integer cases otherwise."""
    if kind in E.FLOATS:
        return HP.hostile(kind, n, count, shift=shift, seed=seed)
    return E.int_cases(kind, n, count, seed=seed + 31 * shift)


def assert_nan_cap(kind, exp):
    assert E.nan_share(kind, exp) <= NAN_CAP, f"{E.nan_share(kind, exp):.3f} of the expected outputs are NaN"


def expected(kind, op, x, count=None, cap=True):
    exp = E.fold(kind, op, x, count=count)
    if cap:
        assert_nan_cap(kind, exp)
    return exp


@functools.lru_cache(maxsize=None)
def fixture_cases(kind):
    """{n: (inputs, {op name: stored output})} of the kind's stored cases."""
    if kind in E.FLOATS:
        cases = load_golden(f"reduce_prod_{kind}")
        return {int(c.split("_n")[1]): (d["in"], {"prod": d["prod"]}) for c, d in cases.items()}
    cases = {c: d for c, d in load_golden("reduce_prod_int").items() if c.startswith(kind)}
    return {int(c.split("_n")[1]): (d["in"], {o: d[o] for o in E.OPS}) for c, d in cases.items()}


def gpu_reduce(kind, op, x, exp, cfg, what, in_offs=None, out_past=0, count=None):
    """One-shot reduction of the rows of x, the output `out_past` elements past
    a 16-byte boundary, input k at element offset in_offs[k]; checks the words
    and the guards around the output."""
    n = x.shape[0]
    count = x.shape[1] if count is None else count
    per = per_packet(kind)
    ins = place_inputs(kind, x, in_offs if in_offs is not None else G.in_offsets(n, per))
    ob = new_output(kind, count + 2 * per, 0)
    out_off = G.aligned_offset(ob, KINDS[kind][2]) + out_past
    hiccl_amd.reduce(ob[out_off:out_off + count], [b[o:o + count] for b, o in ins], count=count, config=cfg, op=op)
    torch.cuda.synchronize()
    check_output(kind, ob, out_off, count, exp, what)


# ---------------------------------------------------------------- 1. one-shot

@pytest.mark.parametrize("store", [0, NT], ids=["wt-by-size", "nt"])
@ENGINES
@pytest.mark.parametrize("kind,opname", KIND_OP)
def test_one_shot_fixture_cases(kind, opname, engine, store):
    """The stored cases (n = 1, 2, 3, 8, 9, 17) and n = 0, which writes the
    identity; the output 0 and 1 elements past 16 bytes, input k offset by
    k + 2 elements."""
    op = E.OPS[opname]
    cfg = dict(engine=engine)
    if store:
        cfg["store_policy"] = store
    count = COUNT if kind in E.FLOATS else INT_COUNT
    for n in NS:
        if n == 0:
            x, exp = np.zeros((0, count), E.carrier(kind)), np.full(count, E.identity(kind, op), E.carrier(kind))
        else:
            x, outs = fixture_cases(kind)[n]
            exp = outs[opname]
            assert x.shape == (n, count)
            assert_nan_cap(kind, exp)
        for out_past in (0, 1):
            gpu_reduce(kind, op, x, exp, cfg, f"{kind} {opname} n={n} out_past={out_past} {cfg}", out_past=out_past,
                       count=count)


def test_n0_writes_the_identity_words():
    """1 / all-ones / 0, as words."""
    for kind, opname, word in (("f32", "prod", 0x3F800000), ("f64", "prod", 0x3FF0000000000000), ("bf16", "prod", 0x3F80),
                               ("f16", "prod", 0x3C00), ("i32", "prod", 1), ("u64", "prod", 1),
                               ("i32", "band", 0xFFFFFFFF), ("u64", "band", (1 << 64) - 1), ("i32", "bor", 0),
                               ("u64", "bxor", 0)):
        out = new_output(kind, 37, 0)[:37]
        hiccl_amd.reduce(out, [], count=37, op=E.OPS[opname])
        torch.cuda.synchronize()
        got = to_host(kind, out)
        U = E.FLOATS[kind][1] if kind in E.FLOATS else E.UINT[kind]
        assert (got.view(U) == U(word)).all(), f"{kind} {opname}: {got.view(U)[:4]}"


@pytest.mark.parametrize("kind,opname", KIND_OP)
def test_phase_two_chunks_and_a_tail(kind, opname):
    """PHASE over more than one workgroup's chunk: two chunks + 37 elements,
    n on both sides of the input pairs."""
    op, count = E.OPS[opname], 2 * phase_chunk(kind) + 37
    for n in (1, 2, 9):
        x = inputs(kind, n, count, shift=n, seed=n)
        gpu_reduce(kind, op, x, expected(kind, op, x), dict(engine=PHASE), f"{kind} {opname} n={n}", out_past=1)


@ENGINES
@pytest.mark.parametrize("kind,opname", KIND_OP)
def test_element_offsets_0_to_7(kind, opname, engine):
    """Inputs and output at element offsets 0-7 past a 16-byte boundary
    (input k at (off + k) mod 8)."""
    op, n = E.OPS[opname], 3
    count = COUNT if kind in E.FLOATS else INT_COUNT
    x = inputs(kind, n, count, shift=6, seed=6)
    exp = expected(kind, op, x)
    for off in range(8):
        gpu_reduce(kind, op, x, exp, dict(engine=engine), f"{kind} {opname} off={off}",
                   in_offs=[(off + k) % 8 for k in range(n)], out_past=off)


@pytest.mark.parametrize("n", [3, 9])
@ENGINES
@pytest.mark.parametrize("kind,opname", KIND_OP)
def test_scalar_head_and_tail_every_class(kind, opname, engine, n):
    """A compute one element short of a packet, one element past 16 bytes, at
    every shift: no packet at all, so every class of every column goes through
    the scalar path (Op::sadd / sstore).  The NaN share is taken over the
    sweep."""
    op, count, exps = E.OPS[opname], per_packet(kind) - 1, []
    for shift in range(HP.NCLS):
        x = inputs(kind, n, count, shift=shift, seed=shift)
        exp = expected(kind, op, x, cap=False)
        gpu_reduce(kind, op, x, exp, dict(engine=engine), f"{kind} {opname} n={n} shift={shift}", out_past=1)
        exps.append(exp)
    assert_nan_cap(kind, np.concatenate(exps))


@ENGINES
@pytest.mark.parametrize("kind,opname", KIND_OP)
def test_65_inputs_run_on_the_plan_kernel(kind, opname, engine):
    op, n = E.OPS[opname], 65
    count = (COUNT if kind in E.FLOATS else INT_COUNT) if engine == TILE else phase_chunk(kind) + 37
    x = inputs(kind, n, count, shift=n, seed=n)
    gpu_reduce(kind, op, x, expected(kind, op, x), dict(engine=engine), f"{kind} {opname} n=65", out_past=1)


# ------------------------------------------------------------------ 2. plans

PLAN_N = (2, 2, 3, 9, 17)


@functools.lru_cache(maxsize=None)
def plan_batch(kind):
    counts = (per_packet(kind) - 1, 4097, 4102, 8200, phase_chunk(kind) + 5)
    return [inputs(kind, n, count, shift=c, seed=60 + c) for c, (n, count) in enumerate(zip(PLAN_N, counts))]


def plan_ops(kind):
    """The ops a plan of `kind` is switched through, each after a launch."""
    return (PROD, BXOR, BAND, BOR, PROD) if kind in E.INTS else (PROD, MAX, PROD)


@pytest.mark.parametrize("variant", list(G.PLAN_VARIANTS))
@ENGINES
@pytest.mark.parametrize("kind", list(KINDS))
def test_plan_five_ragged_computes_and_op_switch(kind, engine, variant):
    """Five computes (n = 2, 2, 3, 9, 17; less than a packet to a phased chunk
    + 5 elements) in ONE launch under PROD, then other operators set on the
    launched plan (the next launch re-uploads) and PROD again; under every peer
    policy, and as one launch per compute (launch_each honours the op)."""
    import ops_expected as EO
    peer, each = G.PLAN_VARIANTS[variant]
    comp = hiccl_amd.Compute(KINDS[kind][0], device=0, engine=engine, op=PROD)
    assert comp.op() == PROD
    if peer:
        comp.set_peer(peer)
    outs, per = [], per_packet(kind)
    for c, x in enumerate(plan_batch(kind)):
        n, count = x.shape
        ob = new_output(kind, count + per, 0)
        off = G.aligned_offset(ob, KINDS[kind][2]) + c % 2
        comp.add(place_inputs(kind, x, G.in_offsets(n, per)), (ob, off), count, compid=0)
        outs.append((ob, off, count))
    for step, op in enumerate(plan_ops(kind)):
        if step:
            comp.set_op(op)
        assert comp.op() == op
        for ob, _, _ in outs:
            ob.view(torch.uint8).fill_(G.SENTINEL)
        comp.start(each=each)
        comp.wait()
        if not each:
            assert comp.engine() == engine
        exps = []
        for c, ((ob, off, count), x) in enumerate(zip(outs, plan_batch(kind))):
            exps.append(EO.fold(kind, op, x) if op == MAX else expected(kind, op, x, cap=False))
            check_output(kind, ob, off, count, exps[-1], f"{kind} {variant} step {step} op {op} compute {c}")
        assert_nan_cap(kind, np.concatenate(exps))  # (the first compute alone is shorter than a packet)
    comp.close()


@pytest.mark.parametrize("kind,opname", KIND_OP)
def test_plan_engine_and_store_form_are_the_hosts_answer(kind, opname):
    """An AUTO plan under a new operator takes the engine and the store form
    hiccl_reduce_auto_choice_op answers on the host, small and large."""
    op = E.OPS[opname]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for n, count in ((3, 4102), (2, 1 << 22)):
        x = inputs(kind, n, 4102, shift=2, seed=70)
        reps = -(-count // 4102)
        rows = [np.tile(r, reps)[:count] for r in x]
        comp = hiccl_amd.Compute(KINDS[kind][0], device=0, op=op)
        out = new_output(kind, count, 0)[:count]
        comp.add([to_dev(kind, r) for r in rows], out, count, compid=0)
        comp.start()
        comp.wait()
        want = hiccl_amd.auto_choice(KINDS[kind][0], count, n, cus=cus, op=op)
        assert (comp.engine(), comp.store_policy()) == (want["engine"], want["store_policy"]), (kind, opname, count, want)
        got, exp = to_host(kind, out), np.tile(E.fold(kind, op, x), reps)[:count]
        assert E.bits_equal(kind, got, exp), f"{kind} {opname} count={count}: {E.first_mismatch(kind, got, exp)}"
        comp.close()


# --------------------------------------------------------------- 3. programs

@pytest.mark.parametrize("kind,opname", KIND_OP)
def test_program_whose_first_reducing_plan_is_a_new_op(kind, opname):
    """One k_program launch: a signal phase, a plan under the new operator and
    a HICCL_BYTES copy plan.  A second reducing plan under SUM is refused; one
    under the same operator joins."""
    op, per = E.OPS[opname], per_packet(kind)
    red = hiccl_amd.Compute(KINDS[kind][0], device=0, op=op)
    outs = []
    for c, x in enumerate(plan_batch(kind)[:4]):
        n, count = x.shape
        ob = new_output(kind, count + per, 0)
        off = G.aligned_offset(ob, KINDS[kind][2]) + 1
        red.add(place_inputs(kind, x, G.in_offsets(n, per)), (ob, off), count, compid=0)
        outs.append((ob, off, count, x))
    payload = np.frombuffer(np.ascontiguousarray(plan_batch(kind)[2]).tobytes(), np.uint8)[:12289]
    src = torch.from_numpy(payload.copy()).to(DEV)
    dst = torch.zeros(len(payload) + 64, dtype=torch.uint8, device=DEV)
    cp = hiccl_amd.Compute(torch.uint8, device=0)
    cp.add([(src, 1)], (dst, 3), len(payload) - 5, compid=0)
    x0 = plan_batch(kind)[1][:, :19]
    other = hiccl_amd.Compute(KINDS[kind][0], device=0)  # SUM
    oo = new_output(kind, 19 + per, 0)
    other.add(place_inputs(kind, x0, G.in_offsets(2, per)), (oo, 0), 19, compid=0)
    same = hiccl_amd.Compute(KINDS[kind][0], device=0, op=op)
    so = new_output(kind, 19 + per, 0)
    same.add(place_inputs(kind, x0, G.in_offsets(2, per)), (so, 0), 19, compid=0)

    flags = torch.zeros(4, dtype=torch.int32, device=DEV)
    prog = hiccl_amd.Program(KINDS[kind][0], device=0)
    prog.add_signal([flags.data_ptr()], [flags.data_ptr()])
    prog.add_plan(cp)
    prog.add_plan(red)
    with pytest.raises(hiccl_amd.HicclError, match="op"):
        prog.add_plan(other)
    prog.add_plan(same)
    assert prog.units() == 4 + 1 + 1 and prog.phases() == 1
    for launch in range(2):
        for ob, _, _, _ in outs:
            ob.view(torch.uint8).fill_(G.SENTINEL)
        so.view(torch.uint8).fill_(G.SENTINEL)
        dst.zero_()
        prog.launch(epochs=[21 + launch], timeout_s=5.0)
        torch.cuda.synchronize()
        assert flags[0].item() == 21 + launch
        exps = []
        for c, (ob, off, count, x) in enumerate(outs):
            exps.append(expected(kind, op, x, cap=False))
            check_output(kind, ob, off, count, exps[-1], f"{kind} {opname} launch {launch} compute {c}")
        assert_nan_cap(kind, np.concatenate(exps))
        check_output(kind, so, 0, 19, expected(kind, op, x0, cap=False), f"{kind} {opname} launch {launch} joined plan")
        d = dst.cpu().numpy()
        nb = len(payload) - 5
        assert np.array_equal(d[3:3 + nb], payload[1:1 + nb]) and not d[:3].any() and not d[3 + nb:].any()
    for o in (prog, red, cp, other, same):
        o.close()


# -------------------------------------------------------------- 4. host pipe

def test_host_pipe_prod():
    """3 pinned host inputs of 300,000 f32 at 256 KiB chunks, depth 2, PROD;
    the bitwise operators are refused on a floating pipe."""
    n, count = 3, 300_000
    x = HP.hostile("f32", n, count, shift=1, seed=21)
    exp = expected("f32", PROD, x)
    ins = [torch.from_numpy(np.array(x[k])).pin_memory() for k in range(n)]
    out = torch.zeros(count, dtype=torch.float32).pin_memory()
    pipe = hiccl_amd.HostPipe(torch.float32, device=0, chunk_bytes=256 << 10, depth=2, op=PROD)
    pipe.reduce(out, ins)
    got = out.numpy()
    assert E.bits_equal("f32", got, exp), E.first_mismatch("f32", got, exp)
    with pytest.raises(hiccl_amd.HicclError, match="HICCL_INT32"):
        L.check(L.lib().hiccl_host_pipe_set_op(pipe._pipe, BXOR), "host_pipe_set_op")
    pipe.close()
    ipipe = hiccl_amd.HostPipe(torch.int32, device=0, chunk_bytes=256 << 10, depth=2, op=BXOR)
    xi = E.int_cases("i32", n, 100_003, seed=5)
    iins = [torch.from_numpy(np.array(xi[k])).pin_memory() for k in range(n)]
    iout = torch.zeros(100_003, dtype=torch.int32).pin_memory()
    ipipe.reduce(iout, iins)
    assert np.array_equal(iout.numpy(), E.fold("i32", E.BXOR, xi))
    ipipe.close()


# ------------------------------------------------------ 5. every bit pattern

@functools.lru_cache(maxsize=None)
def pattern_words(kind):
    """The restatement's (16, 65536) words, checked against the reference's hash first."""
    with open(os.path.join(GOLDEN, "manifest_prod.json")) as fh:
        want = json.load(fh)["patterns"][kind]["sha256"]
    words = E.patterns_expected(kind)
    assert E.patterns_hash(kind, words) == want, f"{kind}: prod_expected no longer gives the reference's words"
    return words


@ENGINES
@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_every_pattern_times_each_multiplier(kind, engine):
    """One n = 2 launch per multiplier: input 0 every 16-bit pattern, input 1
    the multiplier.  The NaN multiplier gives all NaN."""
    words = pattern_words(kind)
    pats = to_dev(kind, E.ALL_PATTERNS)
    for a, m in enumerate(E.ADDENDS[kind]):
        exp = words[a]
        assert E.is_nan(kind, exp).all() if a == 15 else E.nan_share(kind, exp) <= NAN_CAP
        mul = to_dev(kind, np.full(1 << 16, m, np.uint16))
        out = new_output(kind, 1 << 16, 0)[:1 << 16]
        hiccl_amd.reduce(out, [pats, mul], config=dict(engine=engine), op=PROD)
        torch.cuda.synchronize()
        got = to_host(kind, out)
        assert E.bits_equal(kind, got, exp), f"{kind} multiplier {int(m):#06x}: {E.first_mismatch(kind, got, exp)}"


# -------------------------------------------------------------------- 6. C++

def test_cpp_compute_prod_on_gpu(tmp_path):
    """build/prod_compute_hip (tests/cpp/prod_compute.cpp, built by make):
    Compute<prodof<float>> and Compute<prodof<HiCCL::bf16>> on the GPU give the
    fixtures' words, as the host port does."""
    from test_prod_cpu import check_prod_compute
    for port in ("hip", "host"):
        exe = os.path.join(ROOT, "build", f"prod_compute_{port}")
        assert os.path.exists(exe), "run make"
        d = tmp_path / port
        d.mkdir()
        check_prod_compute(exe, d, timeout=60)


@pytest.mark.parametrize("streamed", [True, False], ids=["stream", "host"])
def test_cpp_comm_prod_and_bxor_two_ranks(streamed):
    """build/prod_comm_hip: Comm<prodof<float>> and Comm<bxorof<uint64_t>>
    reduce to root over 2 MPI ranks sharing the GPU, in fresh child processes
    under a time limit."""
    from test_prod_cpu import run_prod_comm
    exe = os.path.join(ROOT, "build", "prod_comm_hip")
    assert os.path.exists(exe), "run make"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", HICCL_STREAM_ORDERED="force" if streamed else "0",
               HICCL_FUSED_GATHER="0", HICCL_SIGNAL_TIMEOUT="10", HICCL_ENGINE="auto", HICCL_GRAPH="0")
    for k in ("HICCL_STEP_PROGRAM", "HICCL_PROG_FENCES"):
        env.pop(k, None)
    run_prod_comm(exe, env=env, timeout=120)


# ------------------------------------------------------- 7. Python refusals

def test_python_layer_refusals_on_tensors():
    f = torch.ones(64, dtype=torch.float32, device=DEV)
    out = torch.empty_like(f)
    for op in (BAND, BOR, BXOR):
        with pytest.raises(TypeError, match="integer"):
            hiccl_amd.reduce(out, [f, f], op=op)
        with pytest.raises(TypeError, match="integer"):
            hiccl_amd.Compute(torch.bfloat16, device=0, op=op)
    x = E.int_cases("u64", 3, 1000, seed=9)
    ins = [torch.from_numpy(r.view(np.int64).copy()).to(DEV) for r in x]  # torch.int64 tensors
    for op, name in ((PROD, "prod"), (BXOR, "bxor")):
        o = torch.empty(1000, dtype=torch.int64, device=DEV)
        hiccl_amd.reduce(o, ins, op=op)
        torch.cuda.synchronize()
        assert np.array_equal(o.cpu().numpy().view(np.uint64), E.fold("u64", E.OPS[name], x)), name
    with pytest.raises(TypeError, match="unsigned"):
        hiccl_amd.reduce(torch.empty(1000, dtype=torch.int64, device=DEV), ins, op=MAX)
