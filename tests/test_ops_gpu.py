"""GPU tier of the MAX / MIN operators (hiccl_op_t) on every layer that takes
them, all six arithmetic types, bit for bit against the stored fixtures
(tests/golden/reduce_ops_*.npz: the reference's reduce_kernel on maxof / minof)
or the NumPy restatement the fixtures pin (tests/ops_expected.py); a NaN output
compares by NaN-ness, and at most 1/16 of any hostile case's outputs are NaN.

  1. one-shot, TILE and PHASE forced: n on both sides of the three-operand
     fold and of the 8-input group (0 writes the identity), output 0 and 1
     elements past 16 bytes, input k offset by k + 2 elements, write-through
     by size and nt on request; every class on the scalar head and tail; in
     place into the first and the last input; the fixtures by default call;
  2. n = 65 and 100, the plan-kernel path of one-shot calls;
  3. plans: five computes in one launch, either engine, every peer policy,
     one launch per compute; the op switched on a launched plan, and SUM
     giving the sums again afterwards;
  4. programs: a signal phase, a MAX plan and a byte-copy plan in one launch;
     a second reducing plan with another op refused;
  5. the host pipe;  6. every 16-bit pattern against 16 addends;
  7. the C++ wrappers: Compute<maxof<float>> / Compute<minof<bf16>> and a
     2-rank Comm<maxof<float>>.

Shapes are the smallest that reach each path: 4,102 elements for TILE (a head,
a partial tile, a tail), two phased chunks plus 37 elements for PHASE.
"""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import hiccl_amd
import hostile as H32
import hostile_f16 as H16
import ops_expected as E
from conftest import ROOT, load_golden
from hiccl_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE, PHASE, AUTO = L.HICCL_ENGINE_TILE, L.HICCL_ENGINE_PHASE, L.HICCL_ENGINE_AUTO
SUM, MAX, MIN = L.HICCL_OP_SUM, L.HICCL_OP_MAX, L.HICCL_OP_MIN
NT = 2  # hiccl_reduce_config_t.store_policy: nt stores whatever the launch's size
NS = [0, 1, 2, 3, 8, 9, 17]
COUNT = 17 * 241 + 5  # 4,102
SENTINEL = 0xA5
NAN_CAP = 1.0 / 16

# kind -> (torch dtype the library is called with, integer dtype of the same width for moving bits, bytes, PHASE packets)
KINDS = {
    "f32": (torch.float32, torch.int32, 4, 16),
    "f64": (torch.float64, torch.int64, 8, 16),
    "bf16": (torch.bfloat16, torch.int16, 2, 16),
    "f16": (torch.float16, torch.int16, 2, 16),
    "i32": (torch.int32, torch.int32, 4, 8),
    "u64": (torch.uint64, torch.int64, 8, 16),
}
NP_INT = {torch.int16: np.int16, torch.int32: np.int32, torch.int64: np.int64}
OPS = {"max": MAX, "min": MIN}
KIND_OP = [pytest.param(k, o, id=f"{k}-{o}") for k in KINDS for o in OPS]
ENGINES = pytest.mark.parametrize("engine", [TILE, PHASE], ids=["tile", "phase"])


def per_packet(kind):
    return 16 // KINDS[kind][2]


def phase_chunk(kind):
    """Elements of one phased chunk: 512 lanes x P packets."""
    return 512 * KINDS[kind][3] * per_packet(kind)


def count_for(kind, engine):
    return COUNT if engine == TILE else 2 * phase_chunk(kind) + 37


# ------------------------------------------------------------------- inputs

def inputs(kind, n, count, shift=0, seed=0):
    """(n, count) hostile inputs of a floating kind, integer cases otherwise."""
    if kind == "f16":
        return H16.hostile(n, count, shift=shift, seed=seed)
    if kind in E.FLOATS:
        return H32.hostile(kind, n, count, shift=shift, seed=seed)
    return E.int_cases(kind, n, count, seed=seed + 31 * shift)


def assert_nan_cap(kind, exp):
    assert E.nan_share(kind, exp) <= NAN_CAP, f"{E.nan_share(kind, exp):.3f} of the expected outputs are NaN"


def expected(kind, op, x, count=None, cap=True):
    exp = E.fold(kind, op, x, count=count)
    if cap:
        assert_nan_cap(kind, exp)
    return exp


# ------------------------------------------------------------ device helpers

def to_dev(kind, a):
    """A carrier array -> a device tensor of the kind's torch dtype holding those bits."""
    tdt, idt, _, _ = KINDS[kind]
    a = np.ascontiguousarray(a, E.carrier(kind))
    return torch.from_numpy(a.view(NP_INT[idt]).copy()).to(DEV).view(tdt)


def to_host(kind, t):
    _, idt, _, _ = KINDS[kind]
    return t.view(idt).cpu().numpy().view(E.carrier(kind))


def place_inputs(kind, x, offsets):
    """Each input row at an element offset inside a buffer of its own."""
    tdt, idt, _, _ = KINDS[kind]
    ins = []
    for k in range(x.shape[0]):
        b = torch.empty(x.shape[1] + offsets[k] + 8, dtype=idt, device=DEV)
        b.view(torch.uint8).fill_(0x5A)
        b[offsets[k]:offsets[k] + x.shape[1]].copy_(to_dev(kind, x[k]).view(idt))
        ins.append((b.view(tdt), offsets[k]))
    return ins


def new_output(kind, count, out_off):
    tdt, idt, _, _ = KINDS[kind]
    ob = torch.empty(count + out_off + 8, dtype=idt, device=DEV)
    ob.view(torch.uint8).fill_(SENTINEL)
    return ob.view(tdt)


def check_output(kind, ob, out_off, count, exp, what):
    host = to_host(kind, ob)
    got = host[out_off:out_off + count]
    assert E.bits_equal(kind, got, exp), f"{what}: {E.first_mismatch(kind, got, exp)}"
    assert (host[:out_off].view(np.uint8) == SENTINEL).all(), f"{what}: guard before the output written"
    assert (host[out_off + count:].view(np.uint8) == SENTINEL).all(), f"{what}: guard after the output written"


def aligned_offset(t, esz):
    """Elements from t's start to its first 16-byte boundary."""
    return ((16 - t.data_ptr() % 16) % 16) // esz


def in_offsets(n, per):
    """Input k is offset by k + 2 elements."""
    return [(k + 2) % (2 * per) for k in range(n)]


def gpu_reduce(kind, op, x, out_past, cfg, what, count=None, cap=True):
    """One-shot reduction of the rows of x; the output starts `out_past`
    elements past a 16-byte boundary.  Checks the guards and the words."""
    n = x.shape[0]
    count = x.shape[1] if count is None else count
    esz = KINDS[kind][2]
    ins = place_inputs(kind, x, in_offsets(n, per_packet(kind)))
    ob = new_output(kind, count + per_packet(kind), 0)
    out_off = aligned_offset(ob, esz) + out_past
    hiccl_amd.reduce(ob[out_off:out_off + count], [b[o:o + count] for b, o in ins], count=count, config=cfg, op=op)
    torch.cuda.synchronize()
    exp = expected(kind, op, x, count=count, cap=cap)
    host = to_host(kind, ob)
    got = host[out_off:out_off + count]
    assert E.bits_equal(kind, got, exp), f"{what}: {E.first_mismatch(kind, got, exp)}"
    assert (host[:out_off].view(np.uint8) == SENTINEL).all(), f"{what}: guard before the output written"
    assert (host[out_off + count:].view(np.uint8) == SENTINEL).all(), f"{what}: guard after the output written"
    return exp


# ---------------------------------------------------------------- 1. one-shot

@pytest.mark.parametrize("store", [0, NT], ids=["wt-by-size", "nt"])
@ENGINES
@pytest.mark.parametrize("kind,opname", KIND_OP)
def test_one_shot(kind, opname, engine, store):
    """Every n (0 writes the identity), the output 0 and 1 elements past 16
    bytes, input k offset by k + 2 elements."""
    op, count = OPS[opname], count_for(kind, engine)
    cfg = dict(engine=engine)
    if store:
        cfg["store_policy"] = store
    for n in NS:
        x = inputs(kind, n, count, shift=n, seed=n)
        for out_past in (0, 1):
            exp = gpu_reduce(kind, op, x, out_past, cfg, f"{kind} {opname} n={n} out_past={out_past} {cfg}", count=count)
        if n == 0:
            assert (exp == E.identity(kind, op)).all()


@pytest.mark.parametrize("n", [3, 9])
@ENGINES
@pytest.mark.parametrize("kind,opname", KIND_OP)
def test_scalar_head_and_tail_every_class(kind, opname, engine, n):
    """A 19-element compute one element past 16 bytes at every shift: every
    hostile class reaches the scalar head and tail (Op::sadd / sstore).  The
    NaN share is taken over the sweep (19 of its 323 outputs)."""
    op, exps = OPS[opname], []
    for shift in range(H32.NCLS):
        x = inputs(kind, n, 19, shift=shift, seed=shift)
        exps.append(gpu_reduce(kind, op, x, 1, dict(engine=engine), f"{kind} {opname} n={n} shift={shift}", cap=False))
    assert_nan_cap(kind, np.concatenate(exps))


@ENGINES
@pytest.mark.parametrize("kind,opname", KIND_OP)
def test_in_place(kind, opname, engine):
    """The output is input 0, then the last input (exact aliasing)."""
    op, n, count = OPS[opname], 3, count_for(kind, engine)
    x = inputs(kind, n, count, shift=4, seed=4)
    exp = expected(kind, op, x)
    for target in (0, n - 1):
        ins = place_inputs(kind, x, in_offsets(n, per_packet(kind)))
        views = [b[o:o + count] for b, o in ins]
        hiccl_amd.reduce(views[target], views, count=count, config=dict(engine=engine), op=op)
        torch.cuda.synchronize()
        got = to_host(kind, views[target].contiguous())
        assert E.bits_equal(kind, got, exp), f"{kind} {opname} into input {target}: {E.first_mismatch(kind, got, exp)}"
        for k in range(n):
            if k != target:
                assert to_host(kind, views[k].contiguous()).tobytes() == np.ascontiguousarray(x[k]).tobytes(), \
                    f"input {k} changed"


@pytest.mark.parametrize("kind", list(KINDS))
def test_golden_fixtures_default_call(kind):
    """Every stored case through hiccl_reduce_op with no config (AUTO)."""
    if kind in E.FLOATS:
        cases = load_golden(f"reduce_ops_{kind}")
    else:
        cases = {c: d for c, d in load_golden("reduce_ops_int").items() if c.startswith(kind)}
    assert len(cases) == 6
    for case, d in cases.items():
        for opname, op in OPS.items():
            x, y = d["in"], d[opname]
            assert E.nan_share(kind, y) <= NAN_CAP
            ins = [to_dev(kind, r) for r in x]
            out = new_output(kind, x.shape[1], 0)[:x.shape[1]]
            hiccl_amd.reduce(out, ins, op=op)
            torch.cuda.synchronize()
            got = to_host(kind, out)
            assert E.bits_equal(kind, got, y), f"{kind} {case} {opname}: {E.first_mismatch(kind, got, y)}"


# --------------------------------------------------------- 2. n > 64 inputs

@pytest.mark.parametrize("n", [65, 100])
@ENGINES
@pytest.mark.parametrize("opname", list(OPS))
@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_more_than_64_inputs_run_on_the_plan_kernel(kind, opname, engine, n):
    count = COUNT if engine == TILE else phase_chunk(kind) + 37
    x = inputs(kind, n, count, shift=n, seed=n)
    for out_past in (0, 1):
        gpu_reduce(kind, OPS[opname], x, out_past, dict(engine=engine), f"{kind} {opname} n={n} out_past={out_past}")


# ------------------------------------------------------------------ 3. plans

PLAN_N = (2, 2, 3, 9, 17)


def plan_counts(kind):
    return (19, 4097, 4102, 8200, phase_chunk(kind) + 5)


@functools.lru_cache(maxsize=None)
def plan_batch(kind):
    return [inputs(kind, n, count, shift=c, seed=40 + c) for c, (n, count) in enumerate(zip(PLAN_N, plan_counts(kind)))]


def sum_expected(kind, x, oracle):
    """The SUM of a compute: the oracle's in-order sum (f16: NumPy's half sum,
    which the f16 fixture pins to the reference)."""
    if kind == "f16":
        return H16.native_sum(x)
    return oracle.reduce(x, dtype=E.carrier(kind))


def sum_equal(kind, got, exp):
    return E.bits_equal(kind, got, exp)  # NaN by NaN-ness, everything else bit for bit


PLAN_VARIANTS = {"plain": (0, False), "peer-stores": (L.HICCL_PEER_STORES, False), "peer-loads": (L.HICCL_PEER_LOADS, False),
                 "peer-both": (L.HICCL_PEER_STORES | L.HICCL_PEER_LOADS, False), "each": (0, True)}


@pytest.mark.parametrize("variant", list(PLAN_VARIANTS))
@ENGINES
@pytest.mark.parametrize("kind", list(KINDS))
def test_plan_five_computes_and_op_switch(kind, engine, variant, oracle):
    """Five computes (n = 2, 2, 3, 9, 17; 19 to a phased chunk + 5 elements) in
    ONE launch under MAX, then MIN set on the launched plan and launched again,
    then SUM: the sums the plan gave before operators existed."""
    peer, each = PLAN_VARIANTS[variant]
    comp = hiccl_amd.Compute(KINDS[kind][0], device=0, engine=engine, op=MAX)
    assert comp.op() == MAX
    if peer:
        comp.set_peer(peer)
    outs = []
    per = per_packet(kind)
    for c, x in enumerate(plan_batch(kind)):
        n, count = x.shape
        ob = new_output(kind, count + per, 0)
        off = aligned_offset(ob, KINDS[kind][2]) + c % 2
        comp.add(place_inputs(kind, x, in_offsets(n, per)), (ob, off), count, compid=0)
        outs.append((ob, off, count))
    assert comp.numcomp == 5
    for op in (MAX, MIN, SUM):
        if op != MAX:
            comp.set_op(op)
        assert comp.op() == op
        for ob, _, _ in outs:
            ob.view(torch.uint8).fill_(SENTINEL)
        comp.start(each=each)
        comp.wait()
        if not each:
            assert comp.engine() == engine
        for c, ((ob, off, count), x) in enumerate(zip(outs, plan_batch(kind))):
            what = f"{kind} {variant} op {op} compute {c}"
            if op == SUM:
                host = to_host(kind, ob)
                exp = sum_expected(kind, x, oracle)
                assert sum_equal(kind, host[off:off + count], exp), f"{what}: {E.first_mismatch(kind, host[off:off + count], exp)}"
            else:
                check_output(kind, ob, off, count, expected(kind, op, x), what)
    comp.close()


# --------------------------------------------------------------- 4. programs

@pytest.mark.parametrize("kind", list(KINDS))
def test_program_signal_phase_max_plan_and_byte_copies(kind):
    """One k_program launch: a signal phase on this rank's own flag, a MAX
    plan and a HICCL_BYTES copy plan.  A second reducing plan with MIN is
    refused; one with MAX joins."""
    per = per_packet(kind)
    red = hiccl_amd.Compute(KINDS[kind][0], device=0, op=MAX)
    outs = []
    for c, x in enumerate(plan_batch(kind)[:4]):
        n, count = x.shape
        ob = new_output(kind, count + per, 0)
        off = aligned_offset(ob, KINDS[kind][2]) + 1
        red.add(place_inputs(kind, x, in_offsets(n, per)), (ob, off), count, compid=0)
        outs.append((ob, off, count, x))
    payload = np.frombuffer(np.ascontiguousarray(plan_batch(kind)[2]).tobytes(), np.uint8)[:12289]
    src = torch.from_numpy(payload.copy()).to(DEV)
    dst = torch.zeros(len(payload) + 64, dtype=torch.uint8, device=DEV)
    cp = hiccl_amd.Compute(torch.uint8, device=0)
    cp.add([(src, 1)], (dst, 3), len(payload) - 5, compid=0)
    other = hiccl_amd.Compute(KINDS[kind][0], device=0, op=MIN)
    x0 = plan_batch(kind)[0]
    oo = new_output(kind, 19 + per, 0)
    other.add(place_inputs(kind, x0, in_offsets(2, per)), (oo, 0), 19, compid=0)
    same = hiccl_amd.Compute(KINDS[kind][0], device=0, op=MAX)
    so = new_output(kind, 19 + per, 0)
    same.add(place_inputs(kind, x0, in_offsets(2, per)), (so, 0), 19, compid=0)

    flags = torch.zeros(4, dtype=torch.int32, device=DEV)
    prog = hiccl_amd.Program(KINDS[kind][0], device=0)
    prog.add_signal([flags.data_ptr()], [flags.data_ptr()])
    prog.add_plan(cp)   # byte copies join a program before its op is known
    prog.add_plan(red)
    with pytest.raises(hiccl_amd.HicclError, match="op"):
        prog.add_plan(other)
    prog.add_plan(same)
    assert prog.units() == 4 + 1 + 1 and prog.phases() == 1
    for launch in range(2):
        for ob, _, _, _ in outs:
            ob.view(torch.uint8).fill_(SENTINEL)
        so.view(torch.uint8).fill_(SENTINEL)
        dst.zero_()
        prog.launch(epochs=[11 + launch], timeout_s=5.0)
        torch.cuda.synchronize()
        assert flags[0].item() == 11 + launch
        for c, (ob, off, count, x) in enumerate(outs):
            check_output(kind, ob, off, count, expected(kind, MAX, x), f"{kind} launch {launch} compute {c}")
        check_output(kind, so, 0, 19, expected(kind, MAX, x0), f"{kind} launch {launch} joined plan")
        d = dst.cpu().numpy()
        nb = len(payload) - 5
        assert np.array_equal(d[3:3 + nb], payload[1:1 + nb]) and not d[:3].any() and not d[3 + nb:].any()
    # a program whose first reducing plan is MIN takes MIN
    prog2 = hiccl_amd.Program(KINDS[kind][0], device=0)
    prog2.add_plan(other)
    with pytest.raises(hiccl_amd.HicclError, match="op"):
        prog2.add_plan(red)
    prog2.launch(timeout_s=5.0)
    torch.cuda.synchronize()
    check_output(kind, oo, 0, 19, expected(kind, MIN, x0), f"{kind} MIN program")
    for o in (prog, prog2, red, cp, other, same):
        o.close()


# -------------------------------------------------------------- 5. host pipe

def test_host_pipe_min():
    """3 host inputs of 300,000 f32 at 256 KiB chunks, depth 2, MIN."""
    n, count = 3, 300_000
    x = H32.hostile("f32", n, count, shift=1, seed=21)
    exp = expected("f32", MIN, x)
    ins = [torch.from_numpy(np.array(x[k])).pin_memory() for k in range(n)]
    out = torch.zeros(count, dtype=torch.float32).pin_memory()
    pipe = hiccl_amd.HostPipe(torch.float32, device=0, chunk_bytes=256 << 10, depth=2, op=MIN)
    pipe.reduce(out, ins)
    got = out.numpy()
    assert E.bits_equal("f32", got, exp), E.first_mismatch("f32", got, exp)
    with pytest.raises(hiccl_amd.HicclError, match="unknown op"):
        L.check(L.lib().hiccl_host_pipe_set_op(pipe._pipe, 9), "host_pipe_set_op")
    pipe.close()
    bytes_pipe = hiccl_amd.HostPipe(torch.uint8, device=0)
    with pytest.raises(hiccl_amd.HicclError, match="HICCL_BYTES"):
        L.check(L.lib().hiccl_host_pipe_set_op(bytes_pipe._pipe, MAX), "host_pipe_set_op")
    bytes_pipe.close()


# ------------------------------------------------------ 6. every bit pattern

@ENGINES
@pytest.mark.parametrize("opname", list(OPS))
@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_every_pattern_against_each_addend(kind, opname, engine):
    """One n = 2 launch per addend: input 0 every 16-bit pattern, input 1 the
    addend; against the stored fixture.  The NaN addend gives all NaN."""
    d = load_golden("reduce_ops_patterns")[kind]
    op = OPS[opname]
    pats = to_dev(kind, E.ALL_PATTERNS)
    for a, addend in enumerate(d["addends"]):
        exp = E.patterns_expected(kind, addend, d[f"{opname}_sel"][a])
        assert E.is_nan(kind, exp).all() if a == 15 else E.nan_share(kind, exp) <= NAN_CAP
        add = to_dev(kind, np.full(1 << 16, addend, np.uint16))
        out = new_output(kind, 1 << 16, 0)[:1 << 16]
        hiccl_amd.reduce(out, [pats, add], config=dict(engine=engine), op=op)
        torch.cuda.synchronize()
        got = to_host(kind, out)
        assert E.bits_equal(kind, got, exp), f"{kind} {opname} addend {int(addend):#06x}: {E.first_mismatch(kind, got, exp)}"


# -------------------------------------------------------------------- 7. C++

def test_cpp_compute_ops_on_gpu(tmp_path):
    """build/ops_compute_hip (tests/cpp/ops_compute.cpp, built by make):
    Compute<maxof<float>> and Compute<minof<HiCCL::bf16>> on the GPU give the
    words of the host port and of the restatement."""
    from test_ops_cpu import check_ops_compute
    outs = {}
    for port in ("hip", "host"):
        exe = os.path.join(ROOT, "build", f"ops_compute_{port}")
        assert os.path.exists(exe), "run make"
        d = tmp_path / port
        d.mkdir()
        outs[port] = check_ops_compute(exe, d, timeout=60)
    assert E.bits_equal("f32", outs["hip"][0], outs["host"][0]) and E.bits_equal("bf16", outs["hip"][1], outs["host"][1])


@pytest.mark.parametrize("streamed", [True, False], ids=["stream", "host"])
def test_cpp_comm_maxof_float_two_ranks(streamed):
    """build/ops_comm_hip: Comm<maxof<float>> reduce to root over 2 MPI ranks
    sharing the GPU, in fresh child processes under a time limit; the root
    checks NaN, -0 / +0 and -Inf / +Inf columns against the `+=` fold."""
    mpirun = shutil.which("mpirun") or "/opt/conda/bin/mpirun"
    exe = os.path.join(ROOT, "build", "ops_comm_hip")
    assert os.path.exists(exe), "run make"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", HICCL_STREAM_ORDERED="force" if streamed else "0",
               HICCL_FUSED_GATHER="0", HICCL_SIGNAL_TIMEOUT="10", HICCL_ENGINE="auto", HICCL_GRAPH="0")
    for k in ("HICCL_STEP_PROGRAM", "HICCL_PROG_FENCES"):
        env.pop(k, None)
    p = subprocess.run(["timeout", "-k", "10", "120", mpirun, "-np", "2", exe, "4099"], capture_output=True, text=True,
                       env=env, cwd="/tmp")
    out = p.stdout + p.stderr
    assert p.returncode == 0 and "maxof<float> reduce to root: PASSED" in out, out[-3000:]
