"""GPU tier: the host state machine that feeds the plan and program kernels.

The arithmetic of every kernel is pinned elsewhere (tests/test_hostile_gpu.py,
tests/test_uniform_desc_gpu.py, tests/test_reduce_gpu.py), always on a plan
built once and launched unchanged.  This file changes plans and programs
BETWEEN launches and checks the sums after every change:

  1. a plan that grows: the pointer stride (its largest n), every tile_begin
     and the unit_comp piece are rebuilt by the re-upload;
  2. one batch walked through ten configurations: the unit size goes from 256
     to 8,192 packets and back, with the kernel that reads the unit table;
  3. hiccl_reduce_plan_enqueue (the stream-ordered transport's entry), never
     plan_sync: re-upload and destroy with an enqueued launch outstanding;
  4. one uploaded plan enqueued from two host threads onto two streams;
  5. programs: the snapshot rule of add_plan, add_plan after a launch,
     set_max_workgroups, computes of n = 0 and n = 70;
  6. outputs that alias an input (the host pipe reduces in place on every
     chunk): every input group of tile_body, behind a scalar head, on the
     dynamic schedule, inside a plan and inside a program.

Expected values always come from the CPU oracle on the same host arrays,
compared bit for bit (a NaN by NaN-ness only: every floating expectation is
first held to the NaN cap of tests/hostile.py).  Outputs and their guard bytes
hold a sentinel before every launch; an output that aliases an input has the
input buffer's own guard bytes around it.  No program here has a signal phase:
nothing in this file can wait on a flag.
"""
import threading
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import hiccl_amd
import hostile as H
from conftest import bits_equal, first_mismatch
from hiccl_amd import _lib as L
from test_hostile_gpu import (DEFAULT_SHAPES, OPS, SENTINEL, cfg_of, check_output, full_count, new_output, offsets_for,
                              place_inputs, shapes_of, vec)
from test_reduce_gpu import DEV, TORCH_OF, to_host
from test_uniform_desc_gpu import tiles_count

pytestmark = pytest.mark.gpu

TILE, PHASE, AUTO = L.HICCL_ENGINE_TILE, L.HICCL_ENGINE_PHASE, L.HICCL_ENGINE_AUTO
WIDE = L.HICCL_ACC_WIDE
NT, WT = 2, 4  # hiccl_reduce_config_t.store_policy
INPUT_GUARD = 0x5A  # what place_inputs leaves around an input: the guard of an output that aliases one
TYPES = {"f32": np.float32, "bf16": np.uint16, "u64": np.uint64}  # hostile kind (u64: wrapping integers) -> carrier
# the dynamic schedule on two workgroups (tests/test_uniform_desc_gpu.py): 66 tickets of one 1,024-packet tile
DYN_CFG = dict(engine=TILE, unroll=4, grid=2, schedule=L.HICCL_SCHED_DYNAMIC, grab=1, store_policy=NT)


def ragged_count(V, off, pkts, tail):
    """Elements of a compute whose output starts `off` elements past a
    16-byte boundary: the scalar head, `pkts` packets, `tail` elements."""
    return (V - off) % V + pkts * V + tail


def data(tname, n, count, shift, seed):
    if tname == "u64":
        return H.wrapping("u64", n, count, seed=seed)
    return H.hostile(tname, n, count, shift=shift, seed=seed)


def expect(oracle, tname, x, count, wide=False):
    exp = oracle.reduce(list(x), count=count, dtype=TYPES[tname], wide=wide)
    if tname != "u64":
        H.assert_nan_cap(tname, exp)
    return exp


def add_compute(comp, oracle, tname, n, off, count, shift, seed):
    """One ragged compute on `comp`: hostile inputs on offsets_for's phases, a
    sentinel-filled output `off` elements past a boundary, the oracle's sum."""
    dt = TYPES[tname]
    tdt, V = TORCH_OF[np.dtype(dt)], vec(dt)
    x = data(tname, n, count, shift, seed)
    ins = place_inputs(x, offsets_for(n, V, off), tdt)
    ob = new_output(count, off, tdt)
    comp.add(ins, (ob, off), count, compid=0)
    return SimpleNamespace(n=n, off=off, count=count, x=x, ins=ins, ob=ob, exp=expect(oracle, tname, x, count))


def refill(recs):
    for r in recs:
        r.ob.view(torch.uint8).fill_(SENTINEL)


def check_all(recs, dt, what, exps=None):
    for c, r in enumerate(recs):
        check_output(r.ob, r.off, r.count, dt, r.exp if exps is None else exps[c],
                     f"{what} compute {c} (n, off, count = {r.n}, {r.off}, {r.count})")


def untouched(ob, what):
    assert (ob.view(torch.uint8).cpu().numpy() == SENTINEL).all(), f"{what}: written"


def c_numcomp(comp):
    return L.lib().hiccl_reduce_plan_numcomp(comp._plan)


# ------------------------------------------------- 1. a plan that grows

GROW_VARIANTS = {"auto": (AUTO, False), "tile": (TILE, False), "phase": (PHASE, False), "each": (AUTO, True)}
SCALAR_SHIFT = 4  # a compute shorter than the class list starts after the NaN classes (the cap holds per array)


def grow_stages(V):
    """(n, output offset, count, class shift) of the computes each stage adds."""
    return [[(2, 1, ragged_count(V, 1, 1025, 1), 0)],
            [(9, V - 1, ragged_count(V, V - 1, 255, V - 1), 1)],
            [(70, 1, ragged_count(V, 1, 2563, 1), 2), (0, 1, ragged_count(V, 1, 255, 1), 3),
             (3, 1, V - 1, SCALAR_SHIFT)]]


@pytest.mark.parametrize("variant", list(GROW_VARIANTS))
@pytest.mark.parametrize("tname", list(TYPES))
def test_plan_grows_between_launches(oracle, tname, variant):
    """Adds after a launch.  Would catch: a table without the unit_comp piece
    kept after the second add (every unit read as compute 0's), the old
    pointer stride after n grew from 2 to 9 to 70 (inputs of the neighbour
    compute summed), tile_begin of the earlier upload, a count = 0 add or an
    n = 0 compute shifting the computes after it, and plan_bytes / numcomp
    (C and Python) counting an add the plan dropped."""
    engine, each = GROW_VARIANTS[variant]
    dt = TYPES[tname]
    tdt, V, esz = TORCH_OF[np.dtype(dt)], vec(dt), np.dtype(dt).itemsize
    comp = hiccl_amd.Compute(tdt, device=0, engine=engine)
    recs = []
    # the count = 0 add of stage C: real buffers, which no launch may touch
    nothing = SimpleNamespace(x=data(tname, 2, 2 * V, 0, 99), ob=new_output(2 * V, 1, tdt))
    nothing.ins = place_inputs(nothing.x, offsets_for(2, V, 1), tdt)
    for s, (specs, launches) in enumerate(zip(grow_stages(V), (1, 1, 2))):
        for n, off, count, shift in specs:
            recs.append(add_compute(comp, oracle, tname, n, off, count, shift, seed=100 + len(recs)))
            if n == 0:
                assert not recs[-1].exp.view(np.uint8).any()  # +0 in every element
        if s == 2:
            comp.add(nothing.ins, (nothing.ob, 1), 0, compid=0)  # documented no-op
        assert comp.bytes() == sum(r.count * (r.n + 1) * esz for r in recs)
        assert c_numcomp(comp) == len(recs)
        assert comp.numcomp == c_numcomp(comp) and len(comp.count) == len(recs)
        for launch in range(launches):
            refill(recs)
            comp.start(each=each)
            comp.wait()
            if not each and engine != AUTO:
                assert comp.engine() == engine
            check_all(recs, dt, f"{tname} {variant} stage {'ABC'[s]} launch {launch}")
    untouched(nothing.ob, "the output of the count = 0 add")
    comp.close()


# ------------------------------- 2. one batch, reconfigured between launches

def batch_specs(V):
    """(n, output offset, packets, tail) of the six ragged computes."""
    return [(1, 0, 2563, 0), (3, 1, 1025, 1), (5, V - 1, 255, V - 1), (9, 2 % V, 2563, 1), (17, 1, 1, 0),
            (70, 3 % V, 1025, V - 1)]


def add_batch(comp, oracle, tname, specs, seed0):
    V = vec(TYPES[tname])
    return [add_compute(comp, oracle, tname, n, off, ragged_count(V, off, pkts, tail), shift=c, seed=seed0 + c)
            for c, (n, off, pkts, tail) in enumerate(specs)]


# (what is called, its argument) -> the plan's configuration and peer flags afterwards
RECONFIG = [
    ("none", None),
    ("config", dict(engine=TILE, unroll=1)),
    ("config", dict(unroll=16)),
    ("config", dict(engine=PHASE)),
    ("config", dict(engine=TILE, unroll=2)),
    ("config", dict(store_policy=NT)),
    ("peer", 3),
    ("peer", 0),
    ("config", dict(acc=WIDE)),
    ("config", {}),
    # the two single-field setters on top of a config, then a config that replaces them again
    ("setters", dict(engine=TILE, acc=WIDE)),
    ("config", {}),
]


def wide_expectations(oracle, xs):
    """The f32-accumulator sums of a bf16 batch; they differ from the native
    ones on non-NaN elements, so each mode's launch is told from the other's."""
    wide = [oracle.reduce(list(x), dtype=np.uint16, wide=True) for x in xs]
    native = [oracle.reduce(list(x), dtype=np.uint16) for x in xs]
    for w in wide:
        H.assert_nan_cap("bf16", w)
    differ = [int(((w != e) & ~H.is_nan("bf16", w) & ~H.is_nan("bf16", e)).sum()) for w, e in zip(wide, native)]
    assert max(differ) > 0, differ
    return wide


@pytest.mark.parametrize("tname", ["f32", "bf16"])
def test_plan_reconfigured_between_launches(oracle, tname):
    """One plan, twelve configurations in a row, two launches each.  Would
    catch: a unit table built for the previous unroll or engine (units of 256
    to 8,192 packets read by a kernel of another tile size), a set_config that
    keeps the earlier accumulator, engine or store form, peer flags that
    survive set_peer(0), and plan_engine / plan_peer / plan_store_policy
    reporting another state than the one launched."""
    dt = TYPES[tname]
    tdt, V = TORCH_OF[np.dtype(dt)], vec(dt)
    comp = hiccl_amd.Compute(tdt, device=0)
    recs = add_batch(comp, oracle, tname, batch_specs(V), seed0=200)
    wide_exps = wide_expectations(oracle, [r.x for r in recs]) if tname == "bf16" else None
    total = sum(r.count for r in recs)
    mean_n = sum(r.count * r.n for r in recs) / total
    cfg, peer = {}, 0
    for step, (call, arg) in enumerate(RECONFIG):
        if call == "config":
            comp.set_config(arg)
            cfg = arg
        elif call == "peer":
            comp.set_peer(arg)
            peer = arg
        elif call == "setters":
            comp.set_engine(arg["engine"])
            comp.set_acc(arg["acc"])
            cfg = arg
        what = f"{tname} step {step} ({call} {arg})"
        exps = wide_exps if cfg.get("acc") == WIDE and wide_exps else None  # the mode means something for bf16 only
        for launch in range(2):
            refill(recs)
            comp.start()
            comp.wait()
            check_all(recs, dt, f"{what} launch {launch}", exps)
        if cfg.get("engine"):
            assert comp.engine() == cfg["engine"], what
        assert comp.peer() == peer, what
        if peer & L.HICCL_PEER_STORES:
            want = WT
        elif cfg.get("store_policy") == NT:
            want = NT
        else:
            want = hiccl_amd.auto_choice(tdt, total, mean_n, config=cfg)["store_policy"]
        assert comp.store_policy() == want, what
    comp.close()


# ------------------------------------------------- 3. enqueue, never wait

def test_plan_enqueue_reupload_and_destroy(oracle):
    """hiccl_reduce_plan_enqueue on the current and on a second stream, a
    re-upload and a destroy while an enqueued launch is outstanding.  Would
    catch: a re-upload or destroy that frees the descriptor block under a
    running launch (the launch reads freed or rewritten memory: wrong sums or
    untouched sentinels), an enqueue that launches on another stream than the
    one given, and a plan_sync that fails after an enqueue."""
    tname, dt = "f32", np.float32
    V = vec(dt)
    comp = hiccl_amd.Compute(torch.float32, device=0)
    recs = add_batch(comp, oracle, tname, batch_specs(V)[:5], seed0=300)
    refill(recs)
    torch.cuda.synchronize()  # the uploads and fills precede the first enqueue
    comp.enqueue()
    comp.wait()  # nothing remembered: returns at once, without error
    torch.cuda.synchronize()
    check_all(recs, dt, "enqueue on the current stream")
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):  # fills, launch and read-back all ordered on `side`
        refill(recs)
        comp.enqueue(stream=side)
        side.synchronize()
        check_all(recs, dt, "enqueue on a second stream")
        # a launch left unsynchronised, an add, then the re-upload (it synchronises the device before it frees
        # the table that launch reads)
        refill(recs)
        comp.enqueue(stream=side)
        recs.append(add_compute(comp, oracle, tname, 4, 1, ragged_count(V, 1, 1025, 1), shift=5, seed=305))
        comp.enqueue(stream=side)
        side.synchronize()
        check_all(recs, dt, "enqueue after an add")
        refill(recs)  # and the new table alone, every output from the sentinel
        comp.enqueue(stream=side)
        side.synchronize()
        check_all(recs, dt, "second enqueue after an add")
    torch.cuda.synchronize()
    comp.set_config(dict(engine=PHASE))
    refill(recs)
    comp.enqueue()
    comp.close()  # destroy with the launch outstanding
    torch.cuda.synchronize()
    check_all(recs, dt, "enqueue, then destroy at once")


# ------------------------- 4. one plan, two streams, two host threads

def check_region(buf, off, count, dt, exp, guard, what):
    host = to_host(buf, dt)
    got = host[off:off + count]
    assert bits_equal(got, exp), f"{what}: {first_mismatch(got, exp)}"
    assert (host[:off].view(np.uint8) == guard).all(), f"{what}: bytes before the output written"
    assert (host[off + count:].view(np.uint8) == guard).all(), f"{what}: bytes after the output written"


@pytest.mark.parametrize("n", [3, 8])
@pytest.mark.parametrize("tname", ["f32", "bf16"])
def test_plan_enqueued_from_two_threads(oracle, tname, n):
    """An uploaded plan on the dynamic schedule, enqueued three times by each
    of two threads onto a stream of its own, as include/hiccl_reduce.h allows.
    Would catch: launches of two streams sharing one ticket counter (units
    skipped or run twice), an enqueue that writes plan state another thread
    reads, and a counter left non-zero -- the one-shot dynamic launches that
    follow on each stream would then skip units and leave their NaN prefill."""
    dt = TYPES[tname]
    tdt, V = TORCH_OF[np.dtype(dt)], vec(dt)
    count = tiles_count(65, dt)
    assert hiccl_amd.auto_choice(tdt, count, n, config=DYN_CFG)["dynamic"] == 1
    comp = hiccl_amd.Compute(tdt, device=0, config=DYN_CFG)
    rec = add_compute(comp, oracle, tname, n, 1, count, shift=n, seed=400 + n)
    comp.start()  # the upload, on the main thread
    comp.wait()
    check_all([rec], dt, f"{tname} n={n} first launch")
    streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
    refill([rec])
    torch.cuda.synchronize()
    errs = []

    def work(i):
        try:
            torch.cuda.set_device(0)
            for _ in range(3):
                comp.enqueue(stream=streams[i])
            streams[i].synchronize()
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    if any(t.is_alive() for t in threads):
        pytest.fail("a thread is still inside enqueue / synchronize after 60 s: nothing more is launched")
    assert not errs, errs
    torch.cuda.synchronize()
    check_all([rec], dt, f"{tname} n={n} after the threads")
    views = [b[o:o + count] for b, o in rec.ins]
    for i, s in enumerate(streams):
        with torch.cuda.stream(s):
            ob = torch.empty(count + 1 + 8, dtype=tdt, device=DEV)
            ob.view(torch.uint8).fill_(0xFF)  # NaN in both types
            hiccl_amd.reduce(ob[1:1 + count], views, count=count, stream=s, config=DYN_CFG)
            s.synchronize()
            check_region(ob, 1, count, dt, rec.exp, 0xFF, f"{tname} n={n} one-shot on stream {i}")
    torch.cuda.synchronize()
    comp.close()


# --------------------------------------------------------------- 5. programs

def launch_program(prog, recs, dt, what, copies=()):
    for launch in range(2):
        refill(recs)
        for cp in copies:
            cp.dst.zero_()
        prog.launch()
        torch.cuda.synchronize()
        check_all(recs, dt, f"{what} launch {launch}")
        for cp in copies:
            d = cp.dst.cpu().numpy()
            assert np.array_equal(d[cp.do:cp.do + cp.nb], cp.host[cp.so:cp.so + cp.nb]), f"{what} launch {launch}: copy"
            assert not d[:cp.do].any() and not d[cp.do + cp.nb:].any(), f"{what} launch {launch}: around the copy"


@pytest.mark.parametrize("tname", list(TYPES))
def test_program_snapshot_reupload_and_workgroup_caps(oracle, tname):
    """add_plan takes the plan's computes as of the call; a later add_plan and
    set_max_workgroups re-upload the program.  Would catch: a program that
    follows the plan's later adds, a re-upload that keeps the old unit_comp or
    unit count (the new computes never run: sentinels stay), a stale pointer
    stride after the new plan raised the largest n, and a capped grid whose
    grid-stride loop drops the units past the cap."""
    dt = TYPES[tname]
    tdt, V = TORCH_OF[np.dtype(dt)], vec(dt)
    red = hiccl_amd.Compute(tdt, device=0)
    recs = add_batch(red, oracle, tname, [(2, 1, 1025, 1), (9, V - 1, 2563, V - 1), (17, 0, 255, 1)], seed0=500)
    prog = hiccl_amd.Program(tdt, device=0)
    prog.add_plan(red)
    fourth = add_compute(red, oracle, tname, 24, 1, ragged_count(V, 1, 2563, 1), shift=3, seed=503)  # after the snapshot
    assert prog.units() == 3 and prog.phases() == 0 and c_numcomp(red) == 4
    refill(recs + [fourth])
    prog.launch()
    torch.cuda.synchronize()
    check_all(recs, dt, f"{tname} snapshot")
    untouched(fourth.ob, "the output of a compute added to the plan after add_plan")
    # re-upload after a launch: a second plan holding the fourth compute, and a byte copy at odd byte offsets
    red2 = hiccl_amd.Compute(tdt, device=0)
    red2.add(fourth.ins, (fourth.ob, fourth.off), fourth.count, compid=0)
    prog.add_plan(red2)
    host = np.frombuffer(H.wrapping("u64", 1, 520, seed=9).tobytes(), np.uint8)
    cp = SimpleNamespace(so=1, do=3, nb=4099, host=host, src=torch.from_numpy(host.copy()).to(DEV),
                         dst=torch.zeros(4099 + 64, dtype=torch.uint8, device=DEV),
                         plan=hiccl_amd.Compute(torch.uint8, device=0))
    cp.plan.add([(cp.src, cp.so)], (cp.dst, cp.do), cp.nb, compid=0)
    prog.add_plan(cp.plan)
    assert prog.units() == 5
    recs.append(fourth)
    launch_program(prog, recs, dt, f"{tname} after add_plan", [cp])
    # more units than workgroups: a 2,563-packet compute alone is 3 to 6 units
    for cap in (1, 3, 0):
        prog.set_max_workgroups(cap)
        launch_program(prog, recs, dt, f"{tname} max_workgroups {cap}", [cp])
    prog.close()
    for c in (red, red2, cp.plan):
        c.close()


@pytest.mark.parametrize("tname", list(TYPES))
def test_program_zero_and_seventy_inputs(oracle, tname):
    """A program of computes with n = 1, 0 and 70.  Would catch: a pointer
    stride capped at 64 or taken from the first plan, an n = 0 unit that reads
    its neighbour's pointers or leaves its output unwritten (+0 expected), and
    table rows of different n overlapping."""
    dt = TYPES[tname]
    tdt, V = TORCH_OF[np.dtype(dt)], vec(dt)
    red = hiccl_amd.Compute(tdt, device=0)
    recs = add_batch(red, oracle, tname, [(1, 1, 1025, 1), (0, V - 1, 255, V - 1), (70, 0, 2563, 1)], seed0=600)
    assert not recs[1].exp.view(np.uint8).any()
    prog = hiccl_amd.Program(tdt, device=0)
    prog.add_plan(red)
    assert prog.units() == 3
    launch_program(prog, recs, dt, f"{tname} n = 1, 0, 70")
    prog.close()
    red.close()


# ------------------------------------------------------ 6. in-place outputs

def alias_offsets(n, V, k):
    """The aliased buffer one element past a 16-byte boundary (a scalar head
    and a tail), the other inputs on offsets_for's phases."""
    offs = offsets_for(n, V, 1)
    offs[k] = 1
    return offs


def reduce_in_place(x, k, dt, exp, config, what, same_as_first=()):
    """A fresh device copy of the rows, out = input k; the inputs listed in
    `same_as_first` are input 0's buffer itself."""
    tdt, V = TORCH_OF[np.dtype(dt)], vec(dt)
    n, count = x.shape
    ins = place_inputs(x, alias_offsets(n, V, k), tdt)
    views = [b[o:o + count] for b, o in ins]
    for j in same_as_first:
        views[j] = views[0]
    hiccl_amd.reduce(views[k], views, count=count, config=config)
    torch.cuda.synchronize()
    check_region(ins[k][0], 1, count, dt, exp, INPUT_GUARD, what)


IN_PLACE_SHAPES = [pytest.param(op, cfg, unit, id=f"{op}-{sid}") for op in OPS for sid, cfg, unit in shapes_of(op)
                   if op != "f64" or sid in DEFAULT_SHAPES]


@pytest.mark.parametrize("op,cfg,unit", IN_PLACE_SHAPES)
def test_in_place_one_shot_every_group(oracle, op, cfg, unit):
    """n = 17, the output aliasing input 0, 7, 8 or 16: the first group of
    tile_body, its last member, the second and the third group (the wide
    tiles' groups of 4 and 2: later ones), with a scalar head and tail.
    Would catch: stores issued before a later input group's loads of the same
    packets, a scalar part that writes out[i] before every input's element i
    is read, and the phased engine writing a chunk before the aliased input's
    sweep."""
    kind, dt, wide = OPS[op][:3]
    n = 17
    x = H.hostile(kind, n, full_count(unit, vec(dt)), shift=n, seed=n)
    exp = oracle.reduce(list(x), dtype=dt, wide=wide)
    H.assert_nan_cap(kind, exp)
    for k in (0, 7, 8, 16):
        reduce_in_place(x, k, dt, exp, cfg, f"{op} {cfg} out = in[{k}]")


@pytest.mark.parametrize("engine", [TILE, PHASE], ids=["tile", "phase"])
@pytest.mark.parametrize("op", ["f32", "bf16", "bf16wide"])
def test_in_place_same_input_twice(oracle, op, engine):
    """in[0] is in[1] is out, n = 9.  Would catch: the output written between
    the two reads of the same buffer (the second read then sees the sum)."""
    kind, dt, wide, _, P = OPS[op]
    unit = 1024 if engine == TILE else 512 * P
    x = H.hostile(kind, 9, full_count(unit, vec(dt)), shift=9, seed=9).copy()
    x[1] = x[0]
    exp = oracle.reduce(list(x), dtype=dt, wide=wide)
    H.assert_nan_cap(kind, exp)
    reduce_in_place(x, 0, dt, exp, cfg_of(op, engine=engine), f"{op} engine {engine} in[0] is in[1] is out",
                    same_as_first=(1,))


@pytest.mark.parametrize("k", [0, 8])
@pytest.mark.parametrize("tname", ["f32", "bf16"])
def test_in_place_dynamic_schedule(oracle, tname, k):
    """In place on the dynamic schedule with interleaved unit order (order 2),
    65 tiles and a partial one, n = 9 (k = 8: the second input group).  Would
    catch: a unit run twice by two tickets (the second run adds the sum to
    itself) and a unit's stores overtaking another unit's loads."""
    dt = TYPES[tname]
    tdt, n = TORCH_OF[np.dtype(dt)], 9
    cfg = dict(DYN_CFG, order=2)
    count = tiles_count(65, dt)
    assert hiccl_amd.auto_choice(tdt, count, n, config=cfg)["dynamic"] == 1
    x = H.hostile(tname, n, count, shift=n, seed=700)
    reduce_in_place(x, k, dt, expect(oracle, tname, x, count), cfg, f"{tname} dynamic out = in[{k}]")


IN_PLACE_BATCH = [(3, 2, 1025), (9, 8, 2563), (17, 16, 255), (70, 69, 1)]  # n, the aliased input, packets


@pytest.mark.parametrize("mode", ["tile", "phase", "program"])
@pytest.mark.parametrize("tname", list(TYPES))
def test_in_place_plan_and_program(oracle, tname, mode):
    """Four computes, each reducing in place into its last input (n = 3, 9,
    17, 70), as a plan on either engine and as a program; one launch per
    fresh fill.  Would catch: the table path (pointers in device memory, n
    past 64) storing before its last group's loads, and a unit of one compute
    writing through another compute's row of the pointer table."""
    dt = TYPES[tname]
    tdt, V = TORCH_OF[np.dtype(dt)], vec(dt)
    engine = {"tile": TILE, "phase": PHASE, "program": AUTO}[mode]
    comp = hiccl_amd.Compute(tdt, device=0, engine=engine)
    recs = []
    for c, (n, k, pkts) in enumerate(IN_PLACE_BATCH):
        count = ragged_count(V, 1, pkts, 1)
        x = data(tname, n, count, shift=c, seed=800 + c)
        ins = place_inputs(x, alias_offsets(n, V, k), tdt)
        comp.add(ins, ins[k], count, compid=0)
        recs.append(SimpleNamespace(buf=ins[k][0], count=count, ins=ins, exp=expect(oracle, tname, x, count), n=n, k=k))
    if mode == "program":
        prog = hiccl_amd.Program(tdt, device=0)
        prog.add_plan(comp)
        assert prog.units() == len(recs)
        prog.launch()
        torch.cuda.synchronize()
        prog.close()
    else:
        comp.start()
        comp.wait()
        assert comp.engine() == engine
    for r in recs:
        check_region(r.buf, 1, r.count, dt, r.exp, INPUT_GUARD, f"{tname} {mode} n={r.n} out = in[{r.k}]")
    comp.close()
