"""GPU tier of the weighted widened sums (out = sum of w[k] * x[k], bf16, f16,
e4m3 or e5m2 inputs, one f32 weight per input read from device memory, the
output f32, overwritten or accumulated into: hiccl_reduce_weighted,
hiccl_reduce_plan_set_weighted) on every layer that takes them.  Every
comparison is bit-exact on the f32 words, a NaN by NaN-ness, against the stored
fixtures (tests/golden/reduce_weighted_*.npz) or the restatement the fixtures
pin (tests/weighted_expected.py); every expected array is checked on the CPU to
be at most hostile.NAN_CAP NaN; guard words stand around every output.  The
helpers that place inputs and outputs are tests/test_widen_gpu.py's and
tests/test_accum_gpu.py's.

  1. one-shot against the fixtures: every kind, n, weight set and alpha, TILE
     and PHASE forced and AUTO, write-through by size and nt; write-through on
     request at n = 9;
  2. counts around every boundary of the layout, output offsets 0-3;
  3. n = 0 ... 65 (n = 65 takes the table path with the caller's weight
     pointer); n = 7, 8, 9, 16 on TILE (a full group plus remainders);
  4. all-ones weights equal the unweighted calls word for word;
  5. freshness: weights written by a kernel just before the call, overwritten in
     place between two launches of a plan, and between replays of captured
     graphs; accumulating, two launches add twice;
  6. plans: five computes with weight tensors of their own in one launch, plain
     and with HICCL_PEER_LOADS, and launch_each;
  7. equal to what a caller does today: x.float() * w[k] copies, then reduce;
  8. the refusals that need tensors;
  9. WidenCompute<bf16> / <f8e4m3> with weights (tests/cpp/weighted_sum.cpp).
"""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import accum_expected as A
import hiccl_amd
import test_accum_gpu as AG
import test_widen_gpu as WG
import weighted_expected as X
import widen_expected as E
from conftest import ROOT, load_golden
from hiccl_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = WG.DEV
TILE, PHASE, AUTO = WG.TILE, WG.PHASE, WG.AUTO
NT, WT = WG.NT, WG.WT
COUNT = X.COUNT
THIRD = X.THIRD
KINDS = pytest.mark.parametrize("kind", X.KINDS)
ACCUM = pytest.mark.parametrize("accum", [False, True], ids=["over", "accum"])
ENGINES3 = pytest.mark.parametrize("engine", [TILE, PHASE, AUTO], ids=["tile", "phase", "auto"])
ENGINES2 = pytest.mark.parametrize("engine", [TILE, PHASE], ids=["tile", "phase"])
config, place_inputs, in_offsets, check_output = WG.config, WG.place_inputs, WG.in_offsets, WG.check_output


@functools.lru_cache(maxsize=None)
def fixture(kind):
    return load_golden(f"reduce_weighted_{kind}")


def dev_weights(w):
    """The weights as a device tensor of their own (the words copied as they are)."""
    return torch.from_numpy(np.ascontiguousarray(w, np.float32).copy()).to(DEV)


def output_for(p, count, off):
    """An overwriting call's output (sentinels) or an accumulating one's (the prior)."""
    return WG.new_output(count, off) if p is None else AG.prior_output(p, count, off)


def launch(kind, out, ins, w, count, cfg=None, alpha=None, accum=False):
    if ins:
        hiccl_amd.reduce_widened(out, ins, count=count, config=cfg, scale=alpha, accumulate=accum, weights=w)
    else:  # n == 0: the pointer form names the input dtype
        with torch.cuda.device(DEV):
            hiccl_amd.reduce_widened_ptrs(E.CODE[kind], out.data_ptr(), [], count, config=cfg, scale=alpha,
                                          accumulate=accum, weights=w)


def run_weighted(kind, x, w, exp, cfg, what, alpha=None, p=None, out_off=1, shift=0, ins=None, count=None):
    """One one-shot call on the rows of x with weights w (a NumPy array);
    checks the words and the guards."""
    count = x.shape[1] if count is None else count
    E.assert_nan_cap(exp)
    if ins is None:
        ins = place_inputs(kind, x, in_offsets(kind, x.shape[0], shift))
    buf, out = output_for(p, count, out_off)
    launch(kind, out, ins, dev_weights(w), count, cfg, alpha, p is not None)
    torch.cuda.synchronize()
    check_output(buf, out_off, count, exp, what)


# ---------------------------------------------------------------- 1. fixtures

@pytest.mark.parametrize("store", [0, NT], ids=["wt-by-size", "nt"])
@ENGINES3
@KINDS
def test_one_shot_fixture_cases(kind, engine, store):
    """Every stored case: n = 1, 2, 3, 8, 9, 17, the five weight sets, unscaled
    and under 1/3, overwriting and accumulating; the output one element past 16
    bytes and the inputs mutually misaligned."""
    cfg = config(engine, store)
    for n in X.NS:
        x, d, p = E.inputs(kind, n), fixture(kind)[f"n{n}"], A.prior(kind, n)
        ins = place_inputs(kind, x, in_offsets(kind, n))
        for name, alpha in X.OVER_CASES:
            key = f"{name}.{X.alpha_name(alpha)}"
            run_weighted(kind, x, X.weights(name, n), d[key], cfg, f"{kind} n={n} {key} {cfg}", alpha=alpha, ins=ins)
        for name, alpha in X.ACCUM_CASES:
            key = f"acc.{name}.{X.alpha_name(alpha)}"
            run_weighted(kind, x, X.weights(name, n), d[key], cfg, f"{kind} n={n} {key} {cfg}", alpha=alpha, ins=ins, p=p)


@KINDS
def test_write_through_on_request(kind):
    """store_policy 4 on both engines (the system-scope write-through kernels), n = 9."""
    x, d, p = E.inputs(kind, 9), fixture(kind)["n9"], A.prior(kind, 9)
    w = X.weights("dequant", 9)
    for engine in (TILE, PHASE):
        run_weighted(kind, x, w, d["dequant.none"], config(engine, WT), f"{kind} wt engine {engine}")
        run_weighted(kind, x, w, d["dequant.third"], config(engine, WT), f"{kind} wt engine {engine} scaled", alpha=THIRD)
        run_weighted(kind, x, w, d["acc.dequant.third"], config(engine, WT), f"{kind} wt engine {engine} accumulating",
                     alpha=THIRD, p=p)


# ------------------------------------------------------- 2. counts and offsets

@ACCUM
@ENGINES2
@KINDS
def test_counts_around_every_boundary(kind, engine, accum):
    """Every count around a packet, a tile and a chunk (32,768 elements, the
    accumulating ops' 16,384), the output 0-3 elements past a 16-byte boundary,
    n = 3 with the `signs` weights; head, body and tail use the same weights.
    count 0 is a no-op."""
    cfg = config(engine)
    n = 3
    w = X.weights("signs", n)
    counts = AG.COUNTS if accum else WG.COUNTS
    big = E.inputs(kind, n, max(counts) + 4)[:, 4:]
    pbig = A.prior(kind, n, max(counts) + 16)[12:]
    for i, count in enumerate(counts):
        if count == 0:
            ins = place_inputs(kind, big[:, :4], in_offsets(kind, n))
            buf, out = AG.prior_output(pbig, 4, 0)
            launch(kind, out, ins, dev_weights(w), 0, cfg, None, accum)
            torch.cuda.synchronize()
            check_output(buf, 0, 4, pbig[:4], f"{kind} count=0 writes nothing")
            continue
        x = big[:, :count]
        p = pbig[:count] if accum else None
        run_weighted(kind, x, w, X.expected(kind, x, w, None, p), cfg, f"{kind} count={count} off={i % 4}", p=p,
                     out_off=i % 4, shift=i)
        if count in (5, 4097, 32769):  # every output offset at a count that has a head, a body and a tail
            for off in range(4):
                run_weighted(kind, x, w, X.expected(kind, x, w, THIRD, p), cfg, f"{kind} count={count} off={off} scaled",
                             alpha=THIRD, p=p, out_off=off, shift=off + 3)


# ------------------------------------------------------------------ 3. inputs

@ACCUM
@ENGINES2
@KINDS
def test_every_n(kind, engine, accum):
    """n = 0, 1, 2, 3, 8, 9, 17 and 65 with `dequant`: 65 runs the plan kernel
    from an uploaded pointer table with the caller's weight pointer.  On TILE
    also n = 7, 16: a full group of 8 plus remainders, so a weight indexed
    relative to its group and not to the input list shows."""
    cfg = config(engine)
    count = COUNT if engine == TILE else WG.CHUNK_ELEMS + 37
    ns = (0, 1, 2, 3, 7, 8, 9, 16, 17, 65) if engine == TILE else (0, 1, 2, 3, 8, 9, 17, 65)
    for n in ns:
        x, w = E.inputs(kind, n, count), X.weights("dequant", n)
        p = A.prior(kind, n, count) if accum else None
        exp = X.expected(kind, x, w, None, p)
        if n >= 9:  # a weight taken relative to its group of 8 would repeat w[0:8]
            again = X.expected(kind, x, np.resize(w[:8], n), None, p)
            assert len(E.mismatches(again, exp)) >= 1
        run_weighted(kind, x, w, exp, cfg, f"{kind} n={n}", p=p, count=count)


# ---------------------------------------------------------- 4. all-ones weights

@ACCUM
@ENGINES3
@KINDS
def test_ones_equal_the_unweighted_call(kind, engine, accum):
    """All-ones weights against reduce_widened / accumulate=True of the same
    call: the same words, NaN by NaN-ness."""
    for n in (2, 9):
        x = E.inputs(kind, n, COUNT)
        p = A.prior(kind, n) if accum else None
        exp = A.accumulated(kind, x, p, THIRD) if accum else E.widened(kind, x, THIRD)
        E.assert_nan_cap(exp)
        ins = place_inputs(kind, x, in_offsets(kind, n))
        got = []
        for w in (None, torch.ones(n, dtype=torch.float32, device=DEV)):
            buf, out = output_for(p, COUNT, 1)
            launch(kind, out, ins, w, COUNT, config(engine), THIRD, accum)
            torch.cuda.synchronize()
            check_output(buf, 1, COUNT, exp, f"{kind} n={n} weights {'ones' if w is not None else 'none'}")
            got.append(out.cpu().numpy()[:COUNT])
        E.assert_equal(got[1], got[0], f"{kind} n={n}: all-ones weights against the unweighted call")


# ---------------------------------------------------------------- 5. freshness

@ACCUM
@KINDS
def test_weights_written_on_the_stream_just_before(kind, accum):
    """The weights are produced by a torch kernel on the same stream
    immediately before the call: no synchronisation, and the call sees them."""
    n = 8
    x, w = E.inputs(kind, n), X.weights("dequant", n)
    p = A.prior(kind, n) if accum else None
    exp = X.expected(kind, x, w, None, p)
    E.assert_nan_cap(exp)
    ins = place_inputs(kind, x, in_offsets(kind, n))
    buf, out = output_for(p, COUNT, 1)
    half = dev_weights(w * np.float32(0.5))  # exact: the doubling below restores every word
    wd = torch.zeros(n, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    torch.mul(half, 2.0, out=wd)
    launch(kind, out, ins, wd, COUNT, None, None, accum)
    torch.cuda.synchronize()
    assert np.array_equal(wd.cpu().numpy().view(np.uint32), w.view(np.uint32))
    check_output(buf, 1, COUNT, exp, f"{kind} weights from the kernel before")


@ENGINES2
@KINDS
def test_plan_follows_weights_overwritten_in_place(kind, engine):
    """One plan launched twice, the weights tensor overwritten in place in
    between: the second result follows the new weights (nothing is uploaded
    again).  Then accumulating: two launches add twice."""
    n = 9
    x = E.inputs(kind, n)
    w1, w2 = X.weights("dequant", n), X.weights("signs", n)
    e1, e2 = X.weighted(kind, x, w1), X.weighted(kind, x, w2)
    E.assert_nan_cap(e1), E.assert_nan_cap(e2)
    assert len(E.mismatches(e1, e2)) >= 1
    ins = place_inputs(kind, x, in_offsets(kind, n))
    wd = dev_weights(w1)
    comp = hiccl_amd.Compute(E.TORCH[kind], device=0, out_dtype=torch.float32, engine=engine, weighted=True)
    try:
        assert comp.weighted()
        buf, out = WG.new_output(COUNT, 1)
        comp.add(ins, out, COUNT, compid=0, weights=wd)
        comp.enqueue()
        torch.cuda.synchronize()
        check_output(buf, 1, COUNT, e1, f"{kind} plan, first weights")
        wd.copy_(dev_weights(w2))
        comp.enqueue()
        torch.cuda.synchronize()
        check_output(buf, 1, COUNT, e2, f"{kind} plan, weights overwritten in place")
    finally:
        comp.close()
    p = A.prior(kind, n)
    twice = X.accumulated(kind, x, w2, p, THIRD, times=2)
    E.assert_nan_cap(twice)
    comp = hiccl_amd.Compute(E.TORCH[kind], device=0, out_dtype=torch.float32, engine=engine, weighted=True,
                             accumulate=True, scale=THIRD)
    try:
        buf, out = AG.prior_output(p, COUNT, 1)
        comp.add(ins, out, COUNT, compid=0, weights=wd)
        comp.enqueue()
        comp.enqueue()
        torch.cuda.synchronize()
        check_output(buf, 1, COUNT, twice, f"{kind} accumulating plan launched twice")
    finally:
        comp.close()


@KINDS
def test_captured_launches_replay_with_new_weights(kind):
    """A captured one-shot call and a captured plan enqueue, each replayed
    after the weights changed in place: each follows the new weights."""
    n = 8
    x = E.inputs(kind, n)
    w1, w2 = X.weights("dequant", n), X.weights("signs", n)
    e2 = X.weighted(kind, x, w2)
    E.assert_nan_cap(e2)
    assert len(E.mismatches(X.weighted(kind, x, w1), e2)) >= 1
    ins = place_inputs(kind, x, in_offsets(kind, n))
    wd = dev_weights(w1)
    buf1, out1 = WG.new_output(COUNT, 1)
    buf2, out2 = WG.new_output(COUNT, 2)
    comp = hiccl_amd.Compute(E.TORCH[kind], device=0, out_dtype=torch.float32, weighted=True)
    try:
        comp.add(ins, out2, COUNT, compid=0, weights=wd)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):  # warm-up outside capture: the plan uploads here
            hiccl_amd.reduce_widened(out1, ins, count=COUNT, weights=wd)
            comp.enqueue(s)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(g1):
            hiccl_amd.reduce_widened(out1, ins, count=COUNT, weights=wd)
        with torch.cuda.graph(g2):
            comp.enqueue(torch.cuda.current_stream())
        wd.copy_(dev_weights(w2))
        torch.cuda.synchronize()
        g1.replay()
        g2.replay()
        torch.cuda.synchronize()
        check_output(buf1, 1, COUNT, e2, f"{kind} captured one-shot call, new weights")
        check_output(buf2, 2, COUNT, e2, f"{kind} captured plan enqueue, new weights")
    finally:
        comp.close()


# -------------------------------------------------------------------- 6. plans

PLAN_SETS = ("dequant", "signs", "extreme", "onezero", "dequant")  # the weight set of each of WG.PLAN_SHAPES' computes


@pytest.mark.parametrize("peer", [0, L.HICCL_PEER_LOADS], ids=["plain", "peer-loads"])
@ENGINES2
@KINDS
def test_plan_of_five_computes(kind, engine, peer):
    """Five computes of unequal n and count (one of 5 elements: scalar only),
    each with a weight tensor of its own, in one launch; scaled; launch_each."""
    shapes = list(WG.PLAN_SHAPES)
    shapes[1] = (shapes[1][0], 3)  # a scalar-only compute of 3 elements
    comp = hiccl_amd.Compute(E.TORCH[kind], device=0, out_dtype=torch.float32, engine=engine, weighted=True)
    try:
        if peer:
            comp.set_peer(peer)
        cases = []
        for j, ((n, count), name) in enumerate(zip(shapes, PLAN_SETS)):
            x, w = E.inputs(kind, n, count + 4)[:, 4:], X.weights(name, n)  # (from column 4 on, as test_counts_...)
            for alpha in (None, THIRD):
                E.assert_nan_cap(X.weighted(kind, x, w, alpha))
            ins = place_inputs(kind, x, in_offsets(kind, n, j))
            buf, out = WG.new_output(count, j % 4)
            comp.add(ins, out, count, compid=0, weights=dev_weights(w))
            cases.append((buf, j % 4, count, x, w))
        assert comp.numcomp == 5
        assert comp.bytes() == sum(c * (n * E.ESZ[kind] + 4) for n, c in shapes)

        def check(alpha, what):
            torch.cuda.synchronize()
            for j, (buf, off, count, x, w) in enumerate(cases):
                check_output(buf, off, count, X.weighted(kind, x, w, alpha), f"{kind} {what} compute {j}")

        comp.start()
        comp.wait()
        assert comp.engine() == engine
        check(None, "plan")
        comp.set_scale(THIRD)
        comp.start()
        comp.wait()
        check(THIRD, "scaled plan")
        if not peer:
            comp.set_scale(None)
            comp.start(each=True)
            comp.wait()
            check(None, "launch_each")
    finally:
        comp.close()


# ------------------------------------------------- 7. what a caller does today

@ENGINES3
@KINDS
def test_equals_dequantise_then_reduce(kind, engine):
    """x.float() * w[k] into f32 copies on the GPU, then hiccl_amd.reduce of the
    copies: the same words, NaN by NaN-ness -- the two-pass path end to end."""
    n, count = 8, WG.TILE_ELEMS + WG.CHUNK_ELEMS + 5
    x, w = E.inputs(kind, n, count), X.weights("dequant", n)
    exp = X.weighted(kind, x, w)
    E.assert_nan_cap(exp)
    ins = place_inputs(kind, x, in_offsets(kind, n))
    wd = dev_weights(w)
    copies = [ins[k].float() * wd[k] for k in range(n)]
    two = torch.empty(count, dtype=torch.float32, device=DEV)
    hiccl_amd.reduce(two, copies)
    buf, out = WG.new_output(count, 2)
    launch(kind, out, ins, wd, count, config(engine))
    torch.cuda.synchronize()
    check_output(buf, 2, count, exp, f"{kind}: one pass")
    E.assert_equal(out.cpu().numpy()[:count], two.cpu().numpy(), f"{kind}: one pass against dequantise-then-reduce")


# ---------------------------------------------------------------- 8. refusals

def test_refusals_that_need_tensors():
    bf = torch.zeros(16, dtype=torch.bfloat16, device=DEV)
    f32 = torch.ones(16, dtype=torch.float32, device=DEV)
    w = torch.ones(2, dtype=torch.float32, device=DEV)
    with pytest.raises(TypeError, match="torch.float32 tensor"):
        hiccl_amd.reduce_widened(f32, [bf, bf], weights=[1.0, 1.0])
    with pytest.raises(TypeError, match="must be torch.float32"):
        hiccl_amd.reduce_widened(f32, [bf, bf], weights=w.double())
    with pytest.raises(ValueError, match="device memory"):
        hiccl_amd.reduce_widened(f32, [bf, bf], weights=w.cpu())
    with pytest.raises(ValueError, match="3 weights for 2 inputs"):
        hiccl_amd.reduce_widened(f32, [bf, bf], weights=torch.ones(3, dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError, match="contiguous"):
        hiccl_amd.reduce_widened(f32, [bf, bf], weights=torch.ones(4, dtype=torch.float32, device=DEV)[::2])
    with pytest.raises(ValueError, match="overlap the output"):
        hiccl_amd.reduce_widened(f32, [bf, bf], weights=f32[4:6])
    rc = L.lib().hiccl_reduce_weighted(L.HICCL_BFLOAT16, L.HICCL_FLOAT32, None, 0, f32.data_ptr(),
                                       hiccl_amd.compute._ptr_table([bf.data_ptr()] * 2), f32.data_ptr() + 16, 2, 16, None,
                                       None)
    assert rc == 1 and "weights overlap the output" in L.last_error()
    plain = hiccl_amd.Compute(torch.bfloat16, device=0, out_dtype=torch.float32)
    try:
        with pytest.raises(ValueError, match="not weighted"):
            plain.add([bf], f32, 16, compid=0, weights=w[:1])
    finally:
        plain.close()
    comp = hiccl_amd.Compute(torch.bfloat16, device=0, out_dtype=torch.float32, weighted=True)
    try:
        with pytest.raises(ValueError, match="weighted computes only"):
            comp.add([bf], f32, 16, compid=0)
        with pytest.raises(ValueError, match="overlap the output"):
            comp.add([bf, bf], f32, 16, compid=0, weights=f32[:2])
        comp.set_accumulate(True)
        with pytest.raises(ValueError, match="HICCL_PEER_STORES"):
            comp.set_peer(L.HICCL_PEER_STORES)
        prog = hiccl_amd.Program(torch.bfloat16, device=0)
        try:
            comp.add([bf, bf], f32, 16, compid=0, weights=w)
            with pytest.raises(hiccl_amd.HicclError, match="widened"):
                prog.add_plan(comp)
        finally:
            prog.close()
    finally:
        comp.close()
    torch.cuda.synchronize()
    assert (f32 == 1).all()
    hiccl_amd.reduce_widened(f32, [bf + 2, bf + 3], scale=0.5, accumulate=True,
                             weights=torch.tensor([2.0, -1.0], dtype=torch.float32, device=DEV))  # 1 + 0.5 * (4 - 3)
    torch.cuda.synchronize()
    assert (f32 == 1.5).all()


# --------------------------------------------------------------------- 9. C++

@pytest.mark.parametrize("kind", ["bf16", "e4m3"])
def test_cpp_weighted_compute_on_gpu(kind, tmp_path):
    """build/weighted_sum_hip (tests/cpp/weighted_sum.cpp built against
    include/hiccl.h by make): WidenCompute<bf16> / WidenCompute<f8e4m3> with
    weights through the batched plan kernel, overwriting and accumulating."""
    exe = os.path.join(ROOT, "build", "weighted_sum_hip")
    assert os.path.exists(exe), "run make"
    n = 9
    d, x, p = fixture(kind)[f"n{n}"], E.inputs(kind, n), A.prior(kind, n)
    for key in ("dequant.third", "acc.dequant.third"):
        E.assert_nan_cap(d[key])
    inp, wts, pri, out = (tmp_path / f"{kind}.{s}" for s in ("in", "w", "prior", "out"))
    np.ascontiguousarray(x).tofile(inp)
    X.weights("dequant", n).tofile(wts)
    np.ascontiguousarray(p).tofile(pri)
    r = subprocess.run([exe, kind, str(inp), str(wts), str(pri), str(out), str(n), str(COUNT), float(THIRD).hex()],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "weighted_sum: PASSED" in r.stdout, r.stdout + r.stderr
    E.assert_equal(np.fromfile(str(out), np.float32), d["dequant.third"], f"WidenCompute<{kind}> weighted")
    E.assert_equal(np.fromfile(str(out) + ".accum", np.float32), d["acc.dequant.third"],
                   f"WidenCompute<{kind}> weighted, accumulating")
