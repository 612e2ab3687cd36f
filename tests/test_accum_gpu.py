"""GPU tier of the accumulating widened sums (out = out + alpha * sum of bf16,
f16, e4m3 or e5m2 inputs, the output f32: hiccl_reduce_accumulate,
hiccl_reduce_plan_set_accumulate) on every layer that takes them.  Every
comparison is bit-exact on the f32 words, a NaN by NaN-ness, against the stored
fixtures (tests/golden/reduce_accum_*.npz) or the restatement the fixtures pin
(tests/accum_expected.py); every expected array is checked on the CPU, before
any device call, to be at most hostile.NAN_CAP NaN; guard words stand around
every output.  The helpers that place inputs and outputs are
tests/test_widen_gpu.py's; the output here holds a prior before each launch.

  1. one-shot against the fixtures: every kind, n and alpha, TILE and PHASE
     forced and AUTO, write-through by size and nt; write-through on request;
  2. counts around every boundary of the layout, output offsets 0-3 (head and
     tail read the prior on the scalar path), mutually misaligned inputs;
  3. n = 0 ... 65 (n = 65 takes the table path), unscaled and under -1/1024;
  4. unscaled equals scale = 1.0 word for word;
  5. equal to the two-pass path of the existing entries (reduce_widened into a
     temporary, then reduce(out, [out, tmp])) wherever the prior is not -0;
  6. plans: five computes in one launch, plain and with HICCL_PEER_LOADS,
     launched twice, set_scale, set_accumulate off and on, launch_each, enqueue,
     bytes(), the PEER_STORES and program refusals;
  7. one captured call replayed three times: the three-step fold;
  8. WidenCompute<bf16> / <f8e4m3> with set_accumulate (tests/cpp/accum_sum.cpp);
  9. the Python refusals that need a tensor.
"""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import accum_expected as A
import hiccl_amd
import test_widen_gpu as WG
import widen_expected as E
from conftest import ROOT, load_golden
from hiccl_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = WG.DEV
TILE, PHASE, AUTO = WG.TILE, WG.PHASE, WG.AUTO
NT, WT = WG.NT, WG.WT
COUNT = A.COUNT
CHUNK_ELEMS = 16384  # a PHASE chunk of these ops: 512 x 8 packets (the widened sums': WG.CHUNK_ELEMS, twice that)
COUNTS = WG.COUNTS[:9] + (16383, 16384, 16385) + WG.COUNTS[9:]
KINDS = pytest.mark.parametrize("kind", A.KINDS)
ENGINES3 = pytest.mark.parametrize("engine", [TILE, PHASE, AUTO], ids=["tile", "phase", "auto"])
ENGINES2 = pytest.mark.parametrize("engine", [TILE, PHASE], ids=["tile", "phase"])
config, place_inputs, in_offsets, check_output = WG.config, WG.place_inputs, WG.in_offsets, WG.check_output


@functools.lru_cache(maxsize=None)
def fixture(kind):
    return load_golden(f"reduce_accum_{kind}")


def prior_output(p, count, off):
    """WG.new_output holding the prior's words (copied as integers: every NaN
    payload arrives): (buffer, view)."""
    buf, out = WG.new_output(count, off)
    if count:
        words = np.ascontiguousarray(p[:count], np.float32).view(np.int32)
        out.view(torch.int32)[:count].copy_(torch.from_numpy(words.copy()))
    return buf, out


def launch(kind, out, ins, count, cfg, alpha):
    if ins:
        hiccl_amd.reduce_widened(out, ins, count=count, config=cfg, scale=alpha, accumulate=True)
    else:  # n == 0: the pointer form names the input dtype
        with torch.cuda.device(DEV):
            hiccl_amd.reduce_widened_ptrs(E.CODE[kind], out.data_ptr(), [], count, config=cfg, scale=alpha, accumulate=True)


def run_accum(kind, x, p, exp, cfg, what, alpha=None, out_off=1, shift=0, ins=None, count=None, inf_of=None, times=1):
    """`times` one-shot calls on the rows of x into an output that holds p;
    checks the words and the guards."""
    count = x.shape[1] if count is None else count
    E.assert_nan_cap(exp, inf_of)
    if ins is None:
        ins = place_inputs(kind, x, in_offsets(kind, x.shape[0], shift))
    buf, out = prior_output(p, count, out_off)
    for _ in range(times):
        launch(kind, out, ins, count, cfg, alpha)
    torch.cuda.synchronize()
    check_output(buf, out_off, count, exp, what)


# ---------------------------------------------------------------- 1. fixtures

@pytest.mark.parametrize("store", [0, NT], ids=["wt-by-size", "nt"])
@ENGINES3
@KINDS
def test_one_shot_fixture_cases(kind, engine, store):
    """Every stored case (n = 0, 1, 2, 3, 8, 9, 17) under every alpha, the
    output one element past 16 bytes and the inputs mutually misaligned, and the
    hand-written zero case."""
    cfg = config(engine, store)
    for n in A.NS:
        x, d = E.inputs(kind, n), fixture(kind)[f"n{n}"]
        ins = place_inputs(kind, x, in_offsets(kind, n))
        s = E.widened(kind, x, count=COUNT)
        for i, (name, alpha) in enumerate(A.ALPHAS):
            exp = d["a0"] if i == 1 else d[f"a{i}"]
            run_accum(kind, x, d["p"], exp, cfg, f"{kind} n={n} alpha {name} {cfg}", alpha=alpha, ins=ins,
                      inf_of=s if alpha == 0.0 else None)
    z = fixture(kind)["zero"]
    assert (z["a0"].view(np.uint32) == 0).all() and (z["a4"].view(np.uint32) == A.NEG_ZERO).all()
    for off in (0, 1):  # the packet path and the scalar path
        run_accum(kind, z["x"], z["p"], z["a0"], cfg, f"{kind} zero case off={off}", out_off=off)
        run_accum(kind, z["x"], z["p"], z["a4"], cfg, f"{kind} zero case scaled off={off}", alpha=-1.0 / 1024.0, out_off=off)


@KINDS
def test_write_through_on_request(kind):
    """store_policy 4 on both engines (the system-scope write-through kernels)."""
    x, d = E.inputs(kind, 9), fixture(kind)["n9"]
    for engine in (TILE, PHASE):
        run_accum(kind, x, d["p"], d["a0"], config(engine, WT), f"{kind} wt engine {engine}")
        run_accum(kind, x, d["p"], d["a2"], config(engine, WT), f"{kind} wt engine {engine} scaled", alpha=A.ALPHAS[2][1])


# ------------------------------------------------------- 2. counts and offsets

@ENGINES2
@KINDS
def test_counts_around_every_boundary(kind, engine):
    """Every count around a packet, a tile and a chunk (16,384 elements here,
    and the widened sums' 32,768), the output 0-3 elements
    past a 16-byte boundary (head 0, 3, 2, 1 scalars that read the prior on the
    scalar path), the inputs at mutually different offsets that change from
    count to count; count 0 is a no-op that leaves the prior alone."""
    cfg = config(engine)
    n = 3
    big = E.inputs(kind, n, max(COUNTS) + 4)[:, 4:]  # (from column 4 on, as tests/test_widen_gpu.py)
    pbig = A.prior(kind, n, max(COUNTS) + 16)[12:]  # from a column past the first run of special words
    for i, count in enumerate(COUNTS):
        alpha = None if i % 2 else 0.5
        if count == 0:
            ins = place_inputs(kind, big[:, :4], in_offsets(kind, n))
            buf, out = prior_output(pbig, 4, 0)
            launch(kind, out, ins, 0, cfg, alpha)
            torch.cuda.synchronize()
            check_output(buf, 0, 4, pbig[:4], f"{kind} count=0 keeps the prior")
            continue
        x, p = big[:, :count], pbig[:count]
        run_accum(kind, x, p, A.accumulated(kind, x, p, alpha), cfg, f"{kind} count={count} off={i % 4}", out_off=i % 4,
                  shift=i, alpha=alpha)
        if count in (5, 4097, 32769):  # every output offset at a count that has a head, a body and a tail
            for off in range(4):
                run_accum(kind, x, p, A.accumulated(kind, x, p, 1.0 / 3.0), cfg, f"{kind} count={count} off={off} scaled",
                          alpha=1.0 / 3.0, out_off=off, shift=off + 3)


# ------------------------------------------------------------------ 3. inputs

@ENGINES2
@KINDS
def test_every_n(kind, engine):
    """n = 0 (keeps p, -0 becomes +0), 1, 2, 3, 8, 9, 17 and 65, which runs the
    plan kernel from an uploaded pointer table; unscaled and under -1/1024."""
    cfg = config(engine)
    count = COUNT if engine == TILE else WG.CHUNK_ELEMS + 37
    for n in (0, 1, 2, 3, 8, 9, 17, 65):
        x, p = E.inputs(kind, n, count), A.prior(kind, n, count)
        exp = A.accumulated(kind, x, p)
        if n == 0:
            keep = A.not_neg_zero(p)
            assert E.bits_equal(exp[keep], p[keep]) and (exp[~keep].view(np.uint32) == 0).all() and (~keep).any()
        run_accum(kind, x, p, exp, cfg, f"{kind} n={n}", count=count)
        run_accum(kind, x, p, A.accumulated(kind, x, p, -1.0 / 1024.0), cfg, f"{kind} n={n} scaled", alpha=-1.0 / 1024.0,
                  count=count)


# ------------------------------------------------------------- 4. scale = 1.0

@ENGINES3
@KINDS
def test_unscaled_equals_scale_one_word_for_word(kind, engine):
    """The unscaled form against scale = 1.0: the same words, NaN payloads
    included."""
    for n in (2, 9):
        x, p = E.inputs(kind, n, COUNT), A.prior(kind, n)
        E.assert_nan_cap(A.accumulated(kind, x, p))
        ins = place_inputs(kind, x, in_offsets(kind, n))
        words = []
        for alpha in (None, 1.0):
            buf, out = prior_output(p, COUNT, 1)
            launch(kind, out, ins, COUNT, config(engine), alpha)
            torch.cuda.synchronize()
            words.append(out.cpu().numpy()[:COUNT].view(np.uint32))
        assert np.array_equal(words[0], words[1]), f"{kind} n={n}: unscaled and scale=1.0 differ"
        E.assert_equal(words[0].view(np.float32), A.accumulated(kind, x, p), f"{kind} n={n}")


# ------------------------------------------------------- 5. the two-pass path

@ENGINES3
@KINDS
def test_equals_the_two_pass_path_of_the_existing_entries(kind, engine):
    """reduce_widened into a temporary, then hiccl_amd.reduce(out, [out, tmp])
    in f32 -- (+0 + p) + r -- gives the same word on every column whose prior is
    not -0, unscaled and scaled."""
    n, count = 8, WG.TILE_ELEMS + WG.CHUNK_ELEMS + 5
    x, p = E.inputs(kind, n, count), A.prior(kind, n, count)
    keep = A.not_neg_zero(p)
    assert keep.mean() > 0.9 and not keep.all()
    ins = place_inputs(kind, x, in_offsets(kind, n))
    for alpha in (None, 1.0 / 3.0):
        exp = A.accumulated(kind, x, p, alpha)
        E.assert_nan_cap(exp)
        tmp = torch.empty(count, dtype=torch.float32, device=DEV)
        two = torch.from_numpy(p.copy()).to(DEV)
        hiccl_amd.reduce_widened(tmp, ins, config=config(engine), scale=alpha)
        hiccl_amd.reduce(two, [two, tmp], config=config(engine))
        buf, out = prior_output(p, count, 2)
        launch(kind, out, ins, count, config(engine), alpha)
        torch.cuda.synchronize()
        check_output(buf, 2, count, exp, f"{kind} alpha {alpha}: one pass")
        got, want = out.cpu().numpy()[:count], two.cpu().numpy()
        E.assert_equal(got[keep], want[keep], f"{kind} alpha {alpha}: one pass against two passes")


# -------------------------------------------------------------------- 6. plans

def _plan_case(kind, comp):
    """Adds the five computes; returns [(buffer, out view, out offset, count, inputs as arrays, prior)]."""
    cases = []
    for j, (n, count) in enumerate(WG.PLAN_SHAPES):
        x, p = E.inputs(kind, n, count), A.prior(kind, n, count)
        ins = place_inputs(kind, x, in_offsets(kind, n, j))
        buf, out = prior_output(p, count, j % 4)
        comp.add(ins, out, count, compid=0)
        cases.append((buf, out, j % 4, count, x, p))
    return cases


def _restore(cases):
    for _, out, _, count, _, p in cases:
        out.view(torch.int32)[:count].copy_(torch.from_numpy(np.ascontiguousarray(p).view(np.int32).copy()))


def _check_plan(kind, cases, expected, what):
    torch.cuda.synchronize()
    for j, (buf, _, off, count, x, p) in enumerate(cases):
        check_output(buf, off, count, expected(x, p), f"{kind} {what} compute {j}")


@pytest.mark.parametrize("peer", [0, L.HICCL_PEER_LOADS], ids=["plain", "peer-loads"])
@ENGINES2
@KINDS
def test_plan_of_five_computes(kind, engine, peer):
    """Compute(out_dtype=torch.float32, accumulate=True): five computes of
    unequal n and count in one launch; launched twice (the fold of two adds);
    scaled; set_accumulate(False) (the widened words, the prior overwritten) and
    on again; launch_each and enqueue."""
    third = 1.0 / 3.0
    for n, count in WG.PLAN_SHAPES:
        x, p = E.inputs(kind, n, count), A.prior(kind, n, count)
        for alpha, times in ((None, 1), (None, 2), (third, 1)):
            E.assert_nan_cap(A.accumulated(kind, x, p, alpha, times))
    comp = hiccl_amd.Compute(E.TORCH[kind], device=0, out_dtype=torch.float32, engine=engine, accumulate=True)
    try:
        assert comp.accumulate() and L.lib().hiccl_reduce_plan_accumulate(comp._plan) == 1
        if peer:
            comp.set_peer(peer)
        cases = _plan_case(kind, comp)
        assert comp.numcomp == 5
        assert comp.bytes() == sum(c * (n * E.ESZ[kind] + 8) for n, c in WG.PLAN_SHAPES)
        comp.start()
        comp.wait()
        assert comp.engine() == engine
        _check_plan(kind, cases, lambda x, p: A.accumulated(kind, x, p), "plan")
        comp.start()  # every launch accumulates
        comp.wait()
        _check_plan(kind, cases, lambda x, p: A.accumulated(kind, x, p, times=2), "plan launched twice")
        _restore(cases)
        comp.set_scale(third)
        comp.start()
        comp.wait()
        _check_plan(kind, cases, lambda x, p: A.accumulated(kind, x, p, third), "scaled plan")
        comp.set_accumulate(False)
        assert not comp.accumulate()
        assert comp.bytes() == sum(c * (n * E.ESZ[kind] + 4) for n, c in WG.PLAN_SHAPES)
        comp.start()
        comp.wait()
        _check_plan(kind, cases, lambda x, p: E.widened(kind, x, third), "set_accumulate(False)")
        comp.set_accumulate(True)
        _restore(cases)
        if not peer:
            comp.start(each=True)
            comp.wait()
            _check_plan(kind, cases, lambda x, p: A.accumulated(kind, x, p, third), "scaled launch_each")
            _restore(cases)
        comp.set_scale(None)
        comp.enqueue()
        _check_plan(kind, cases, lambda x, p: A.accumulated(kind, x, p), "enqueue after clear_scale")
    finally:
        comp.close()


@KINDS
def test_plan_refusals(kind):
    """PEER_STORES from either side, an unwidened plan, an overlapping (even an
    exactly aliasing) output, and a program."""
    plain = hiccl_amd.Compute(E.TORCH[kind], device=0)
    try:
        with pytest.raises(ValueError, match="only a widened sum accumulates"):
            plain.set_accumulate(True)
        rc = L.lib().hiccl_reduce_plan_set_accumulate(plain._plan, 1)
        assert rc == 1 and "only a widened plan accumulates" in L.last_error()
    finally:
        plain.close()
    comp = hiccl_amd.Compute(E.TORCH[kind], device=0, out_dtype=torch.float32)
    try:
        comp.set_peer(L.HICCL_PEER_STORES)
        with pytest.raises(ValueError, match="HICCL_PEER_STORES"):
            comp.set_accumulate(True)
        rc = L.lib().hiccl_reduce_plan_set_accumulate(comp._plan, 1)
        assert rc == 1 and "HICCL_PEER_STORES" in L.last_error() and not comp.accumulate()
        comp.set_peer(L.HICCL_PEER_LOADS)
        # a config whose shape the kernels about to run lack, in either direction: PHASE 512 x 16 is the widened
        # kernels' chunk, 512 x 8 the accumulating ones'
        comp.set_config(dict(engine=PHASE, block=512, unroll=16))
        with pytest.raises(hiccl_amd.HicclError, match="shape the accumulating kernels lack.*block 512, unroll 8"):
            comp.set_accumulate(True)
        assert not comp.accumulate()
        comp.set_config({})
        comp.set_accumulate(True)
        assert comp.accumulate()
        with pytest.raises(hiccl_amd.HicclError, match="plan_set_config"):
            comp.set_config(dict(engine=PHASE, block=512, unroll=16))
        comp.set_config(dict(engine=PHASE, block=512, unroll=8))
        with pytest.raises(hiccl_amd.HicclError, match="shape the widened kernels lack.*block 512, unroll 16"):
            comp.set_accumulate(False)
        assert comp.accumulate()
        comp.set_config({})
        with pytest.raises(ValueError, match="HICCL_PEER_STORES"):
            comp.set_peer(L.HICCL_PEER_STORES | L.HICCL_PEER_LOADS)
        rc = L.lib().hiccl_reduce_plan_set_peer(comp._plan, L.HICCL_PEER_STORES)
        assert rc == 1 and "plan_set_peer" in L.last_error() and comp.peer() == L.HICCL_PEER_LOADS
        raw = torch.zeros(1024, dtype=torch.uint8, device=DEV)
        out = raw[:256].view(torch.float32)
        for lo in (0, 128):
            x = raw[lo:lo + 64 * E.ESZ[kind]].view(E.TORCH[kind])
            with pytest.raises(hiccl_amd.HicclError, match="overlaps out"):
                comp.add([x], out, 64, compid=0)
            with pytest.raises(hiccl_amd.HicclError, match="overlaps out"):
                hiccl_amd.reduce_widened(out, [x], count=64, accumulate=True)
        y = raw[512:512 + 64 * E.ESZ[kind]].view(E.TORCH[kind])
        comp.add([y], out, 64, compid=0)
        prog = hiccl_amd.Program(E.TORCH[kind], device=0)
        try:
            with pytest.raises(hiccl_amd.HicclError, match="widened"):
                prog.add_plan(comp)
        finally:
            prog.close()
        assert (raw == 0).all()
    finally:
        comp.close()


# ------------------------------------------------------------------- 7. graph

@KINDS
def test_captured_call_replayed_three_times(kind):
    """A one-shot call with n = 8 and alpha = 1/3 captured into a graph and
    replayed three times: every replay accumulates, so the words are the
    three-step fold fl32(fl32(fl32(p + r) + r) + r), not p + 3r."""
    n, alpha = 8, 1.0 / 3.0
    x, p = E.inputs(kind, n, COUNT), fixture(kind)["n8"]["p"]
    exp = A.accumulated(kind, x, p, alpha, times=3)
    E.assert_nan_cap(exp)
    assert len(E.mismatches(A.thrice_at_once(kind, x, p, alpha), exp)) >= 1
    ins = place_inputs(kind, x, in_offsets(kind, n))
    buf, out = prior_output(p, COUNT, 1)
    words = torch.from_numpy(np.ascontiguousarray(p).view(np.int32).copy()).to(DEV)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hiccl_amd.reduce_widened(out, ins, count=COUNT, scale=alpha, accumulate=True)  # warm-up outside capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        hiccl_amd.reduce_widened(out, ins, count=COUNT, scale=alpha, accumulate=True)
    out.view(torch.int32)[:COUNT].copy_(words)  # the prior again: capture ran nothing, the warm-up did
    torch.cuda.synchronize()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    check_output(buf, 1, COUNT, exp, f"{kind} three replays")


# --------------------------------------------------------------------- 8. C++

@pytest.mark.parametrize("kind", ["bf16", "e4m3"])
def test_cpp_accumulating_compute_on_gpu(kind, tmp_path):
    """build/accum_sum_hip (tests/cpp/accum_sum.cpp built against
    include/hiccl.h by make): WidenCompute<bf16> / WidenCompute<f8e4m3> with
    set_accumulate through the batched plan kernel: plain, scaled, launched
    twice, and after set_accumulate(false)."""
    exe = os.path.join(ROOT, "build", "accum_sum_hip")
    assert os.path.exists(exe), "run make"
    n, alpha = 9, 1.0 / 3.0
    d, x = fixture(kind)[f"n{n}"], E.inputs(kind, n)
    i = [a for _, a in A.ALPHAS].index(alpha)
    twice = A.accumulated(kind, x, d["p"], alpha, times=2)
    for exp in (d["a0"], d[f"a{i}"], twice, E.widened(kind, x, alpha)):
        E.assert_nan_cap(exp)
    inp, pri, out = tmp_path / f"{kind}.in", tmp_path / f"{kind}.prior", tmp_path / f"{kind}.out"
    np.ascontiguousarray(x).tofile(inp)
    np.ascontiguousarray(d["p"]).tofile(pri)
    p = subprocess.run([exe, kind, str(inp), str(pri), str(out), str(n), str(COUNT), float(alpha).hex()],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "accum_sum: PASSED" in p.stdout, p.stdout + p.stderr
    E.assert_equal(np.fromfile(str(out) + ".plain", np.float32), d["a0"], f"WidenCompute<{kind}> accumulate")
    E.assert_equal(np.fromfile(str(out), np.float32), d[f"a{i}"], f"WidenCompute<{kind}> accumulate scaled")
    E.assert_equal(np.fromfile(str(out) + ".twice", np.float32), twice, f"WidenCompute<{kind}> two launches")
    E.assert_equal(np.fromfile(str(out) + ".off", np.float32), E.widened(kind, x, alpha), f"WidenCompute<{kind}> off")


# ----------------------------------------------------------- 9. Python layer

def test_python_refusals_that_need_a_tensor():
    bf = torch.zeros(16, dtype=torch.bfloat16, device=DEV)
    hf = torch.zeros(16, dtype=torch.float16, device=DEV)
    f32 = torch.ones(16, dtype=torch.float32, device=DEV)
    with pytest.raises(TypeError, match="accumulate must be a bool"):
        hiccl_amd.reduce_widened(f32, [bf], accumulate=1)
    with pytest.raises(TypeError, match="writes torch.float32"):
        hiccl_amd.reduce_widened(bf, [bf], accumulate=True)
    with pytest.raises(TypeError, match="widened sums take"):
        hiccl_amd.reduce_widened(f32, [torch.zeros(16, device=DEV)], accumulate=True)
    with pytest.raises(TypeError, match="!= inputs"):
        hiccl_amd.reduce_widened(f32, [bf, hf], accumulate=True)
    with pytest.raises(ValueError, match="at least one input"):
        hiccl_amd.reduce_widened(f32, [], accumulate=True)
    with pytest.raises(ValueError, match="finite"):
        hiccl_amd.reduce_widened(f32, [bf], scale=float("nan"), accumulate=True)
    with pytest.raises(ValueError, match="accumulates in f32"):
        hiccl_amd.reduce_widened(f32, [bf], config=dict(acc=L.HICCL_ACC_WIDE), accumulate=True)
    with pytest.raises(ValueError, match="elements"):
        hiccl_amd.reduce_widened(f32, [bf[:8]], accumulate=True)
    with pytest.raises(hiccl_amd.HicclError, match="unsupported config"):
        hiccl_amd.reduce_widened(f32, [bf], config=dict(engine=TILE, unroll=2), accumulate=True)
    assert (f32 == 1).all()
    hiccl_amd.reduce_widened(f32, [bf + 2, bf + 3], scale=0.5, accumulate=True)  # 1 + 0.5 * 5
    torch.cuda.synchronize()
    assert (f32 == 3.5).all()
