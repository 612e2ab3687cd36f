"""CPU tier of the accumulating widened sums (hiccl_reduce_accumulate and its
kin: out = out + alpha * sum of bf16, f16 or FP8 inputs, the output f32): the
ABI and every refusal, AUTO's answers, the restatement (tests/accum_expected.py)
against the stored fixtures and the conditions the generator recorded, the
Python layer's checks and the C++ layer on the host (WidenCompute<T> with
set_accumulate on the host port, plain and under sanitizers).  No test here
needs the reference; the fixtures pin the restatement to the reference's own
reduce_kernel<float> (tests/golden/make_golden_accum.py).  The tests of a
plan's entries need a device to bind the plan to and skip without one, as the
other plans' do; tests/test_accum_gpu.py repeats those refusals.
"""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import accum_expected as A
import hiccl_amd
import widen_expected as E
from conftest import GOLDEN, ROOT, load_golden, make
from hiccl_amd import _lib as L

IN_DTYPES = {k: E.CODE[k] for k in E.KINDS}
NEW_SYMBOLS = ("hiccl_reduce_accumulate", "hiccl_reduce_auto_choice_accumulate", "hiccl_reduce_plan_set_accumulate",
               "hiccl_reduce_plan_accumulate")
F32 = L.HICCL_FLOAT32
T, P = L.HICCL_ENGINE_TILE, L.HICCL_ENGINE_PHASE


def _tab(ptrs):
    return (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs)


def _accumulate(in_dtype, out_dtype=F32, alpha=None, cfg=None, ins=(0x200000,), out=0x100000, count=4):
    a = ctypes.byref(ctypes.c_double(alpha)) if alpha is not None else None
    return L.lib().hiccl_reduce_accumulate(in_dtype, out_dtype, a, ctypes.c_void_p(out), _tab(list(ins)), len(ins),
                                           count, None, ctypes.byref(cfg) if cfg is not None else None)


def _refused(rc, *words):
    msg = L.last_error()
    assert rc == 1 and msg and all(w in msg for w in words), (rc, msg, words)


# ----------------------------------------------------------------------- ABI

def test_new_symbols_are_declared_bound_and_exported():
    declared = L.header_functions()
    for name in NEW_SYMBOLS:
        assert name in declared and name in L._SIGS and hasattr(L.lib(), name), name
    assert L.lib().hiccl_version() >= 800  # 0.7.0 had no accumulating sums
    import inspect
    for fn in (hiccl_amd.reduce_widened, hiccl_amd.reduce_widened_ptrs, hiccl_amd.auto_choice, hiccl_amd.Compute.__init__):
        assert inspect.signature(fn).parameters["accumulate"].default is False, fn
    assert callable(hiccl_amd.Compute.set_accumulate)


def test_one_shot_refusals_return_invalid_value_with_a_message():
    """hiccl_reduce_accumulate applies hiccl_reduce_widened's checks, before any
    device work -- the pointers here are not device memory -- with return code
    1 and a message that names the entry."""
    for kind, dt in IN_DTYPES.items():
        esz = E.ESZ[kind]
        for bad_out in (L.HICCL_FLOAT64, L.HICCL_BFLOAT16, L.HICCL_FLOAT16, dt, L.HICCL_INT32, 42):
            _refused(_accumulate(dt, bad_out), "hiccl_reduce_accumulate", "HICCL_FLOAT32 only")
        _refused(_accumulate(dt, cfg=L.ReduceConfig(acc=L.HICCL_ACC_WIDE)), "hiccl_reduce_accumulate",
                 "always accumulates in f32")
        for mis in (1, 2, 3):
            _refused(_accumulate(dt, out=0x100000 + mis), "out is not aligned")
        if esz == 2:
            _refused(_accumulate(dt, ins=(0x200001,)), "in[0] is not element-aligned")
        # no overlap of out with any input, exact aliasing included
        count, o0 = 64, 0x100000
        o1, span = o0 + 4 * count, esz * count
        for p in (o0, o0 + 2 * esz, o0 + 128, o1 - esz, o0 - span + esz, o0 - 2 * esz):
            _refused(_accumulate(dt, ins=(0x300000, p), count=count), "in[1] overlaps out")
        for count in ((1 << 62), (1 << 64) - 1):
            _refused(_accumulate(dt, count=count), "count overflows")
        for bad in (float("inf"), float("-inf"), float("nan")):
            _refused(_accumulate(dt, alpha=bad), "hiccl_reduce_accumulate", "alpha must be finite")
        for bad in (1e300, -3.5e38):
            _refused(_accumulate(dt, alpha=bad), "finite as a float")
        _refused(_accumulate(dt, out=0), "out is NULL")
        _refused(_accumulate(dt, ins=(0,)), "in[0] is NULL")
        _refused(_accumulate(dt, cfg=L.ReduceConfig(engine=9)), "bad engine")
        # count 0 is a no-op once the arguments are valid
        for alpha in (None, 0.0, 1e-60, 0.5):
            assert _accumulate(dt, alpha=alpha, count=0) == 0, L.last_error()
    for bad_in in (L.HICCL_FLOAT32, L.HICCL_FLOAT64, L.HICCL_INT32, L.HICCL_UINT64, L.HICCL_BYTES, 7, 42):
        _refused(_accumulate(bad_in), "hiccl_reduce_accumulate", "widened sums take")
        out = [ctypes.c_int() for _ in range(5)]
        rc = L.lib().hiccl_reduce_auto_choice_accumulate(bad_in, None, 1024, 2.0, 256, *[ctypes.byref(v) for v in out])
        _refused(rc, "auto_choice_accumulate", "widened sums take")
    lib = L.lib()
    assert lib.hiccl_reduce_plan_set_accumulate(None, 1) == 1 and "plan is NULL" in L.last_error()
    assert lib.hiccl_reduce_plan_accumulate(None) == -1


def test_unsupported_shapes_are_refused_never_replaced():
    """The accumulating kernels cover what the widened ones cover: TILE 256 x 4
    and PHASE's default chunk, which is 8 packets per lane for these ops (the
    widened sums' 16 is refused), nt loads, nt or write-through stores."""
    for kind, dt in IN_DTYPES.items():
        for cfg in (dict(engine=T, unroll=1), dict(engine=T, unroll=2), dict(engine=T, unroll=8),
                    dict(engine=T, unroll=16), dict(engine=T, block=512, unroll=4), dict(engine=P, block=512, unroll=16),
                    dict(engine=P, block=1024, unroll=4), dict(nontemporal=1), dict(store_policy=1),
                    dict(store_policy=3)):
            with pytest.raises(hiccl_amd.HicclError, match="no kernel"):
                hiccl_amd.auto_choice(dt, 1 << 20, 3, config=cfg, out_dtype=F32, accumulate=True)
            rc = _accumulate(dt, cfg=L.ReduceConfig(**cfg), ins=(0x200000, 0x300000, 0x400000), count=1 << 12)
            _refused(rc, "unsupported config")
        for cfg in (dict(engine=T, unroll=4), dict(engine=P), dict(engine=P, block=512, unroll=8),
                    dict(store_policy=2), dict(store_policy=4)):
            got = hiccl_amd.auto_choice(dt, 1 << 20, 3, config=cfg, out_dtype=F32, accumulate=True)
            assert (got["engine"], got["unroll"]) in ((T, 4), (P, 8))


def _plan(dtype):
    import torch
    if not torch.cuda.is_available() or torch.cuda.device_count() < 1:
        pytest.skip("no HIP device to bind a plan to")
    h = ctypes.c_void_p()
    assert L.lib().hiccl_reduce_plan_create(ctypes.byref(h), dtype, 0) == 0, L.last_error()
    return h


@pytest.mark.parametrize("kind", E.KINDS)
def test_plan_entries_and_their_refusals(kind):
    """set_accumulate / accumulate, their refusals and hiccl_reduce_plan_bytes.
    Nothing is launched: the pointers are not device memory."""
    lib, dt, esz = L.lib(), IN_DTYPES[kind], E.ESZ[kind]
    h = _plan(dt)
    try:
        assert lib.hiccl_reduce_plan_accumulate(h) == 0
        _refused(lib.hiccl_reduce_plan_set_accumulate(h, 1), "plan_set_accumulate", "only a widened plan accumulates")
        assert lib.hiccl_reduce_plan_set_accumulate(h, 0) == 0  # off is what it is already
        assert lib.hiccl_reduce_plan_set_out_dtype(h, F32) == 0, L.last_error()
        # PEER_STORES is refused from either side; PEER_LOADS is taken
        assert lib.hiccl_reduce_plan_set_peer(h, L.HICCL_PEER_STORES) == 0
        _refused(lib.hiccl_reduce_plan_set_accumulate(h, 1), "plan_set_accumulate", "HICCL_PEER_STORES")
        assert lib.hiccl_reduce_plan_accumulate(h) == 0
        assert lib.hiccl_reduce_plan_set_peer(h, L.HICCL_PEER_LOADS) == 0
        # a config whose shape the accumulating kernels lack: the widened sums' PHASE shape, 512 x 16, which the
        # widened plan takes, names a chunk these kernels do not have (theirs is 512 x 8)
        wide_chunk = L.ReduceConfig(engine=P, block=512, unroll=16)
        assert lib.hiccl_reduce_plan_set_config(h, ctypes.byref(wide_chunk)) == 0, L.last_error()
        _refused(lib.hiccl_reduce_plan_set_accumulate(h, 1), "plan_set_accumulate",
                 "the plan's config names a shape the accumulating kernels lack", "block 512, unroll 8")
        assert lib.hiccl_reduce_plan_accumulate(h) == 0
        assert lib.hiccl_reduce_plan_set_config(h, None) == 0
        assert lib.hiccl_reduce_plan_set_accumulate(h, 1) == 0, L.last_error()
        assert lib.hiccl_reduce_plan_accumulate(h) == 1
        # and back: the accumulating plan takes 512 x 8 and refuses 512 x 16; switching off is then refused, because
        # the widened kernels lack 512 x 8 -- refused, never replaced -- and the plan stays accumulating
        _refused(lib.hiccl_reduce_plan_set_config(h, ctypes.byref(wide_chunk)), "plan_set_config", "unroll 8")
        half_chunk = L.ReduceConfig(engine=P, block=512, unroll=8)
        assert lib.hiccl_reduce_plan_set_config(h, ctypes.byref(half_chunk)) == 0, L.last_error()
        _refused(lib.hiccl_reduce_plan_set_accumulate(h, 0), "plan_set_accumulate",
                 "the plan's config names a shape the widened kernels lack", "block 512, unroll 16")
        assert lib.hiccl_reduce_plan_accumulate(h) == 1
        assert lib.hiccl_reduce_plan_set_accumulate(h, 1) == 0  # on is what it is already
        assert lib.hiccl_reduce_plan_set_config(h, None) == 0
        assert lib.hiccl_reduce_plan_set_accumulate(h, 0) == 0 and lib.hiccl_reduce_plan_accumulate(h) == 0
        assert lib.hiccl_reduce_plan_set_accumulate(h, 1) == 0 and lib.hiccl_reduce_plan_accumulate(h) == 1
        for flags in (L.HICCL_PEER_STORES, L.HICCL_PEER_STORES | L.HICCL_PEER_LOADS):
            _refused(lib.hiccl_reduce_plan_set_peer(h, flags), "plan_set_peer", "HICCL_PEER_STORES")
        assert lib.hiccl_reduce_plan_peer(h) == L.HICCL_PEER_LOADS
        assert lib.hiccl_reduce_plan_set_peer(h, 0) == 0
        # the shapes are the widened kernels': refused by set_config on the accumulating plan
        for unroll in (1, 2, 8, 16):
            cfg = L.ReduceConfig(engine=T, unroll=unroll)
            _refused(lib.hiccl_reduce_plan_set_config(h, ctypes.byref(cfg)), "plan_set_config")
        for cfg in (L.ReduceConfig(engine=T, unroll=4), L.ReduceConfig(engine=P), L.ReduceConfig()):
            assert lib.hiccl_reduce_plan_set_config(h, ctypes.byref(cfg)) == 0, L.last_error()
        half, got = ctypes.c_double(0.5), ctypes.c_double()
        assert lib.hiccl_reduce_plan_set_scale(h, ctypes.byref(half)) == 0, L.last_error()
        assert lib.hiccl_reduce_plan_scale(h, ctypes.byref(got)) == 1 and got.value == 0.5
        # add: the widened buffer rules, exact aliasing refused
        o0, count = 0x100000, 64
        for p in (o0, o0 + 128, o0 + 4 * count - esz):
            _refused(lib.hiccl_reduce_plan_add(h, ctypes.c_void_p(o0), _tab([0x300000, p]), 2, count), "overlaps out")
        assert lib.hiccl_reduce_plan_add(h, ctypes.c_void_p(o0), _tab([0x200000, 0x300000, 0x400000]), 3, 1000) == 0
        assert lib.hiccl_reduce_plan_add(h, ctypes.c_void_p(0x500000), _tab([0x600000]), 1, 77) == 0
        assert lib.hiccl_reduce_plan_bytes(h) == 1000 * (3 * esz + 8) + 77 * (esz + 8)
        assert lib.hiccl_reduce_plan_set_accumulate(h, 0) == 0 and lib.hiccl_reduce_plan_accumulate(h) == 0
        assert lib.hiccl_reduce_plan_bytes(h) == 1000 * (3 * esz + 4) + 77 * (esz + 4)
        assert lib.hiccl_reduce_plan_set_accumulate(h, 7) == 0 and lib.hiccl_reduce_plan_accumulate(h) == 1
        prog = ctypes.c_void_p()
        assert lib.hiccl_program_create(ctypes.byref(prog), dt, 0) == 0, L.last_error()
        try:
            _refused(lib.hiccl_program_add_plan(prog, h), "program_add_plan", "widened")
        finally:
            lib.hiccl_program_destroy(prog)
    finally:
        lib.hiccl_reduce_plan_destroy(h)


def test_set_accumulate_refuses_a_plan_of_another_dtype():
    """A plan that cannot be widened cannot accumulate either: "not widened"
    comes before every other check.  (The shape refusal of set_accumulate, in
    both directions, is in test_plan_entries_and_their_refusals.)"""
    for dt in (L.HICCL_FLOAT32, L.HICCL_FLOAT64, L.HICCL_INT32):
        h = _plan(dt)
        try:
            _refused(L.lib().hiccl_reduce_plan_set_accumulate(h, 1), "plan_set_accumulate", "only a widened plan")
            assert L.lib().hiccl_reduce_plan_accumulate(h) == 0
        finally:
            L.lib().hiccl_reduce_plan_destroy(h)


# ---------------------------------------------------------------------- AUTO

def _same_choice(got, want):
    """The widened answer, except the PHASE chunk: 8 packets per lane, not 16."""
    want = dict(want)
    if want["engine"] == P:
        assert want["unroll"] == 16
        want["unroll"] = 8
    return got == want


def _answers(dt, count, n, cfg, accumulate):
    try:
        return hiccl_amd.auto_choice(dt, count, n, config=cfg, out_dtype=F32, accumulate=accumulate)
    except hiccl_amd.HicclError as e:
        assert "no kernel" in str(e), e
        return None


def _named_phase_shape(dt, count, n, cfg):
    """A config that names a PHASE unroll: 16 answers for the widened sum only,
    8 for the accumulating one only, anything else for neither."""
    widened, mine = _answers(dt, count, n, cfg, False), _answers(dt, count, n, cfg, True)
    u = cfg["unroll"]
    assert (widened is not None) == (u == 16 and cfg.get("block", 512) == 512), (dt, count, n, cfg, widened)
    assert (mine is not None) == (u == 8 and cfg.get("block", 512) == 512), (dt, count, n, cfg, mine)


def test_auto_choice_accumulate_equals_the_widened_answer():
    """hiccl_reduce_auto_choice_accumulate answers what
    hiccl_reduce_auto_choice_widened answers -- engine, workgroups per CU,
    schedule and store form, by the widened sum's own thresholds -- row for row
    of tests/auto_table.py.  One field differs by construction: where the
    engine is PHASE the kernels' chunk is 8 packets per lane (the widened
    sums': 16), so `unroll` says 8.  A config that names a PHASE unroll names
    the shape of at most one of the two sums: 16 is the widened sum's and
    refused here, 8 is this sum's and refused there, anything else is refused
    by both; the two named shapes answer alike in every other field."""
    import auto_table as AT
    rows = [(count, n, None) for (_, count, n), _ in AT.RULE_CASES]
    rows += [(k[1], k[2], k[3]) for k, _ in AT.all_engine_rows()] + [(k[1], k[2], k[3]) for k, _ in AT.all_store_rows()]
    seen, engines = 0, set()
    for count, n, cfg in rows:
        if cfg and cfg.get("acc"):
            continue
        if cfg and cfg.get("engine") == P and cfg.get("unroll"):
            for dt in IN_DTYPES.values():
                _named_phase_shape(dt, count, n, cfg)
            continue
        for dt in IN_DTYPES.values():
            try:
                want = hiccl_amd.auto_choice(dt, count, n, config=cfg, out_dtype=F32)
            except hiccl_amd.HicclError:
                with pytest.raises(hiccl_amd.HicclError):
                    hiccl_amd.auto_choice(dt, count, n, config=cfg, out_dtype=F32, accumulate=True)
                continue
            got = hiccl_amd.auto_choice(dt, count, n, config=cfg, out_dtype=F32, accumulate=True)
            assert _same_choice(got, want), (dt, count, n, cfg, got, want)
            engines.add(got["engine"])
            seen += 1
    assert seen > 80 and engines == {T, P}
    for dt in IN_DTYPES.values():  # the two named PHASE shapes, whether or not the table has such a row
        for count, n in ((1 << 24, 3), (1 << 26, 8)):
            for unroll in (8, 16, 4):
                _named_phase_shape(dt, count, n, dict(engine=P, block=512, unroll=unroll))
            mine = hiccl_amd.auto_choice(dt, count, n, config=dict(engine=P, block=512, unroll=8), out_dtype=F32, accumulate=True)
            theirs = hiccl_amd.auto_choice(dt, count, n, config=dict(engine=P, block=512, unroll=16), out_dtype=F32)
            assert _same_choice(mine, theirs), (dt, count, n, mine, theirs)
    for dt in IN_DTYPES.values():  # the store form counts the bytes WRITTEN: 4 * count
        assert hiccl_amd.auto_choice(dt, 1 << 26, 8, out_dtype=F32, accumulate=True)["store_policy"] == 4
        assert hiccl_amd.auto_choice(dt, (1 << 26) + 4, 8, out_dtype=F32, accumulate=True)["store_policy"] == 2
        got = hiccl_amd.auto_choice(dt, 1 << 16, 100, out_dtype=F32, accumulate=True)  # n > 64: the plan kernel
        assert _same_choice(got, hiccl_amd.auto_choice(dt, 1 << 16, 100, out_dtype=F32))


# -------------------------------------------------------------- Python layer

def test_python_layer_refuses_before_any_device_work():
    import torch
    ptrs = hiccl_amd.reduce_widened_ptrs
    with pytest.raises(TypeError, match="accumulate must be a bool"):
        ptrs(L.HICCL_BFLOAT16, 0x100000, [0x200000], 4, accumulate=1)
    with pytest.raises(TypeError, match="widened sums take"):
        ptrs(L.HICCL_FLOAT32, 0x100000, [0x200000], 4, accumulate=True)
    with pytest.raises(TypeError, match="writes torch.float32"):
        ptrs(L.HICCL_BFLOAT16, 0x100000, [0x200000], 4, out_dtype_code=L.HICCL_BFLOAT16, accumulate=True)
    with pytest.raises(ValueError, match="finite"):
        ptrs(L.HICCL_BFLOAT16, 0x100000, [0x200000], 4, scale=float("inf"), accumulate=True)
    with pytest.raises(ValueError, match="accumulates in f32"):
        ptrs(L.HICCL_FLOAT8_E4M3, 0x100000, [0x200000], 4, config=dict(acc=L.HICCL_ACC_WIDE), accumulate=True)
    # what the Python layer lets through, the library still refuses with a message: no aliasing at all
    with pytest.raises(hiccl_amd.HicclError, match="overlaps out"):
        ptrs(L.HICCL_BFLOAT16, 0x100000, [0x100000], 4, stream=0, accumulate=True)
    with pytest.raises(ValueError, match="only a widened sum accumulates"):
        hiccl_amd.auto_choice(torch.bfloat16, 1024, 2, accumulate=True)
    with pytest.raises(TypeError, match="accumulate must be a bool"):
        hiccl_amd.auto_choice(torch.bfloat16, 1024, 2, out_dtype=torch.float32, accumulate="yes")
    with pytest.raises(TypeError, match="widened sums take"):
        hiccl_amd.auto_choice(torch.float32, 1024, 2, out_dtype=torch.float32, accumulate=True)
    x, out = torch.zeros(8, dtype=torch.bfloat16), torch.zeros(8)
    with pytest.raises(ValueError, match="device tensor"):
        hiccl_amd.reduce_widened(out, [x], accumulate=True)
    # the Compute constructor checks before it creates a plan
    for kw, exc, match in ((dict(dtype=torch.bfloat16, accumulate=True), ValueError, "only a widened sum accumulates"),
                           (dict(dtype=torch.float32, accumulate=True), ValueError, "only a widened sum accumulates"),
                           (dict(dtype=torch.bfloat16, out_dtype=torch.float32, accumulate=1), TypeError, "must be a bool"),
                           (dict(dtype=torch.float32, out_dtype=torch.float32, accumulate=True), TypeError,
                            "widened sums take")):
        with pytest.raises(exc, match=match):
            hiccl_amd.Compute(device=0, **kw)


# ----------------------------------------------- restatement against fixtures

def _manifest():
    with open(os.path.join(GOLDEN, "manifest_accum.json")) as fh:
        return json.load(fh)


def test_manifest_records_files_inputs_priors_and_conditions():
    m = _manifest()
    assert len(m["files"]) >= 4
    for fname, info in m["files"].items():
        path = os.path.join(GOLDEN, fname)
        assert os.path.getsize(path) == info["bytes"] < (1 << 20)
        assert hashlib.sha256(open(path, "rb").read()).hexdigest() == info["sha256"]
    assert [[name, None if a is None else float(a).hex()] for name, a in A.ALPHAS] == m["alphas"]
    assert [a for _, a in A.ALPHAS] == [None, 1.0, 1 / 3, 0.7, -1 / 1024, 0.0]
    assert A.COUNT == 4102 and A.NS == (0, 1, 2, 3, 8, 9, 17)
    for kind in A.KINDS:
        for n in A.NS:  # neither is taken from the files by the generator: both must still be what it used
            assert E.array_hash(E.inputs(kind, n)) == m["inputs"][f"{kind}/n{n}"], (kind, n)
            assert E.array_hash(A.prior(kind, n)) == m["priors"][f"{kind}/n{n}"], (kind, n)
    c = m["conditions"]
    assert len(c["fusion"]) == 4 * 6 * 2 and len(c["order"]) == 4 * 5 and len(c["repeat"]) == 4
    assert all(v >= 1 for part in c.values() for v in part.values())


def test_the_prior_holds_every_special_word():
    for kind in A.KINDS:
        p = A.prior(kind, 8)
        w, col = p.view(np.uint32), np.arange(A.COUNT) % 61
        for i, word in enumerate(A.SPECIALS):
            assert (w[col == 3 + i] == word).all()
        rest = p[(col < 3) | (col > 11)]
        assert np.isfinite(rest).all() and (np.abs(rest) < 2.0 ** 13).all() and (rest != 0).mean() > 0.99
        assert not np.array_equal(p, A.prior(kind, 9))


@pytest.mark.parametrize("kind", A.KINDS)
def test_restatement_gives_the_stored_outputs(kind):
    """accum_expected.accumulated on the generated inputs and the stored prior =
    the stored words, for every n and alpha; the NaN cap; alpha = 1 gives the
    unscaled words; and the conditions the manifest records, counted again."""
    cases, m = load_golden(f"reduce_accum_{kind}"), _manifest()["conditions"]
    assert sorted(cases) == sorted([f"n{n}" for n in A.NS] + ["zero"])
    stored = ["p"] + [f"a{i}" for i in range(len(A.ALPHAS)) if i != 1]
    for n in A.NS:
        d, x = cases[f"n{n}"], E.inputs(kind, n)
        assert sorted(d) == sorted(stored)
        p = d["p"]
        assert np.array_equal(p.view(np.uint32), A.prior(kind, n).view(np.uint32))
        s = E.widened(kind, x, count=A.COUNT)
        for i, (name, alpha) in enumerate(A.ALPHAS):
            exp = d["a0"] if i == 1 else d[f"a{i}"]
            E.assert_nan_cap(exp, s if alpha == 0.0 else None)
            E.assert_equal(A.accumulated(kind, x, p, alpha), exp, f"{kind} n={n} alpha {name}")
            keep = A.not_neg_zero(p)  # the two-pass path of the existing entries gives the same words there
            E.assert_equal(A.two_pass(p, A.contribution(kind, x, alpha, A.COUNT))[keep], exp[keep], f"{kind} n={n} two-pass")
            if n >= 1 and name in ("third", "0.7"):
                assert len(E.mismatches(A.fused(kind, x, p, alpha), exp)) == m["fusion"][f"{kind}/n{n}/{name}"] >= 1
        if n >= 2:
            assert len(E.mismatches(A.prior_first(kind, x, p), d["a0"])) == m["order"][f"{kind}/n{n}"] >= 1
        if n == 0:  # p is kept, except that -0 + +0 is +0; under a negative alpha -0 stays
            keep = A.not_neg_zero(p)
            E.assert_equal(d["a0"][keep], p[keep], f"{kind} n=0 keeps p")
            assert (d["a0"][~keep].view(np.uint32) == 0).all() and (~keep).any()
            assert (d["a4"][~keep].view(np.uint32) == A.NEG_ZERO).all()
    x8, p8 = E.inputs(kind, 8), cases["n8"]["p"]
    three = A.accumulated(kind, x8, p8, 1 / 3, times=3)
    assert len(E.mismatches(A.thrice_at_once(kind, x8, p8, 1 / 3), three)) == m["repeat"][f"{kind}/n8/third"] >= 1
    E.assert_equal(A.add_prior(A.add_prior(cases["n8"]["a2"], A.contribution(kind, x8, 1 / 3)), A.contribution(kind, x8, 1 / 3)),
                   three, f"{kind}: the fold of three adds")
    # the zero rules, written by hand
    z = cases["zero"]
    zx, zp = A.zero_case(kind)
    assert np.array_equal(z["x"], zx) and (z["p"].view(np.uint32) == A.NEG_ZERO).all()
    assert (z["a0"].view(np.uint32) == 0).all() and (z["a4"].view(np.uint32) == A.NEG_ZERO).all()
    E.assert_equal(A.accumulated(kind, zx, zp), z["a0"], f"{kind} zero case")
    assert np.array_equal(A.accumulated(kind, zx, zp, -1 / 1024).view(np.uint32), z["a4"].view(np.uint32))


def test_fused_restatement_is_a_single_rounding():
    """accum_expected.fused against exact rational arithmetic on a sample."""
    from fractions import Fraction
    x, p = E.inputs("bf16", 3), A.prior("bf16", 3)
    s, a = E.acc_sum("bf16", x), E.a32(1 / 3)
    got = A.fused("bf16", x, p, 1 / 3)
    checked = 0
    for i in range(0, A.COUNT, 5):  # 821 columns, about two thirds of them finite
        if not (np.isfinite(s[i]) and np.isfinite(p[i])):
            continue
        exact = Fraction(float(s[i])) * Fraction(float(a)) + Fraction(float(p[i]))
        with np.errstate(all="ignore"):
            lo = np.nextafter(got[i], np.float32(-np.inf))
            hi = np.nextafter(got[i], np.float32(np.inf))
        if not (np.isfinite(got[i]) and np.isfinite(lo) and np.isfinite(hi)):
            continue
        d = abs(exact - Fraction(float(got[i])))
        assert d <= abs(exact - Fraction(float(lo))) and d <= abs(exact - Fraction(float(hi))), i
        checked += 1
    assert checked > 400


# ------------------------------------------------------------- the C++ layer

def _run_accum_sum(exe, tmp_path, tag, env=None):
    n, alpha = 9, 1.0 / 3.0
    i = [a for _, a in A.ALPHAS].index(alpha)
    for kind in A.KINDS:
        x = E.inputs(kind, n)
        d = load_golden(f"reduce_accum_{kind}")[f"n{n}"]
        inp, pri, out = tmp_path / f"{tag}_{kind}.in", tmp_path / f"{tag}_{kind}.prior", tmp_path / f"{tag}_{kind}.out"
        np.ascontiguousarray(x).tofile(inp)
        np.ascontiguousarray(d["p"]).tofile(pri)
        p = subprocess.run([str(exe), kind, str(inp), str(pri), str(out), str(n), str(A.COUNT), float(alpha).hex()],
                           capture_output=True, text=True, env=env)
        assert p.returncode == 0 and "accum_sum: PASSED" in p.stdout, p.stdout + p.stderr
        assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr
        E.assert_equal(np.fromfile(str(out) + ".plain", np.float32), d["a0"], f"WidenCompute<{kind}> accumulate")
        E.assert_equal(np.fromfile(str(out), np.float32), d[f"a{i}"], f"WidenCompute<{kind}> accumulate scaled")
        E.assert_equal(np.fromfile(str(out) + ".twice", np.float32), A.accumulated(kind, x, d["p"], alpha, times=2),
                       f"WidenCompute<{kind}> two launches")
        E.assert_equal(np.fromfile(str(out) + ".off", np.float32), E.widened(kind, x, alpha),
                       f"WidenCompute<{kind}> set_accumulate(false)")


def test_accumulating_compute_on_the_host_port(tmp_path):
    """tests/cpp/accum_sum.cpp built with HICCL_PORT_HOST: WidenCompute<T> with
    set_accumulate for the four types on the fixtures' inputs and priors."""
    make(ROOT, "build/accum_sum")
    _run_accum_sum(os.path.join(ROOT, "build", "accum_sum"), tmp_path, "plain")


def test_accumulating_compute_host_port_under_sanitizers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined and
    run as a program (no preload), as tests/test_widen_cpu.py runs widen_sum."""
    inc = os.environ.get("MPI_INC", "/opt/conda/include")
    lib = os.environ.get("MPI_LIB", "/opt/conda/lib")
    exe = tmp_path / "accum_sum_san"
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-DHICCL_PORT_HOST", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"), "-I", inc,
                         os.path.join(ROOT, "tests", "cpp", "accum_sum.cpp"), "-o", str(exe),
                         os.path.join(lib, "libmpi.so"), f"-Wl,-rpath,/usr/lib/x86_64-linux-gnu:{lib}"],
                        capture_output=True, text=True)
    if cc.returncode != 0 and ("asan" in cc.stderr or "ubsan" in cc.stderr or "sanitize" in cc.stderr):
        pytest.skip("g++ has no sanitizer runtimes here: " + cc.stderr.strip()[-200:])
    assert cc.returncode == 0, cc.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    _run_accum_sum(exe, tmp_path, "san", env)
