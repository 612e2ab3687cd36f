"""CPU tier of the widened sums (hiccl_reduce_widened and its kin: bf16, f16 or
FP8 inputs summed into an f32 output): the ABI and every refusal, AUTO's
answers, the restatement (tests/widen_expected.py) against the stored fixtures
and the pattern hashes, the Python layer's checks and the C++ layer on the host
(HiCCL::WidenCompute<T> on the host port, plain and under sanitizers).  No test
here needs the reference; the fixtures pin the restatement to the reference's
own reduce_kernel<float> on the widened inputs
(tests/golden/make_golden_widen.py).  The tests of a plan's entries need a
device to bind the plan to and skip without one, as the other plans' do.
"""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import hiccl_amd
import widen_expected as E
from conftest import GOLDEN, ROOT, load_golden, make
from hiccl_amd import _lib as L

IN_DTYPES = {k: E.CODE[k] for k in E.KINDS}
NEW_SYMBOLS = ("hiccl_reduce_widened", "hiccl_reduce_auto_choice_widened", "hiccl_reduce_plan_set_out_dtype",
               "hiccl_reduce_plan_out_dtype")
F32 = L.HICCL_FLOAT32
T, P = L.HICCL_ENGINE_TILE, L.HICCL_ENGINE_PHASE


def _tab(ptrs):
    return (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs)


def _widened(in_dtype, out_dtype=F32, alpha=None, cfg=None, ins=(0x200000,), out=0x100000, count=4):
    a = ctypes.byref(ctypes.c_double(alpha)) if alpha is not None else None
    return L.lib().hiccl_reduce_widened(in_dtype, out_dtype, a, ctypes.c_void_p(out), _tab(list(ins)), len(ins), count,
                                        None, ctypes.byref(cfg) if cfg is not None else None)


def _refused(rc, *words):
    msg = L.last_error()
    assert rc == 1 and msg and all(w in msg for w in words), (rc, msg, words)


# ----------------------------------------------------------------------- ABI

def test_new_symbols_are_declared_bound_and_exported():
    declared = L.header_functions()
    for name in NEW_SYMBOLS:
        assert name in declared and name in L._SIGS and hasattr(L.lib(), name), name
    assert L.lib().hiccl_version() >= 700  # 0.6.0 had no widened sums
    for name in ("reduce_widened", "reduce_widened_ptrs"):
        assert callable(getattr(hiccl_amd, name))


def test_one_shot_refusals_return_invalid_value_with_a_message():
    """Every refusal of hiccl_reduce_widened comes before any device work --
    the pointers here are not device memory -- with return code 1 and a
    message."""
    for kind, dt in IN_DTYPES.items():
        esz = E.ESZ[kind]
        for bad_out in (L.HICCL_FLOAT64, L.HICCL_BFLOAT16, L.HICCL_FLOAT16, dt, L.HICCL_INT32, 42):
            _refused(_widened(dt, bad_out), "HICCL_FLOAT32 only")
        _refused(_widened(dt, cfg=L.ReduceConfig(acc=L.HICCL_ACC_WIDE)), "always accumulates in f32")
        # out misaligned by 2 bytes (and by 1, 3)
        for mis in (1, 2, 3):
            _refused(_widened(dt, out=0x100000 + mis), "out is not aligned")
        if esz == 2:
            _refused(_widened(dt, ins=(0x200001,)), "in[0] is not element-aligned")
        # out [0x100000, 0x100000 + 4 * 64) against an input of 64 elements that
        # overlaps it at its start, in its middle and on its last byte only, and
        # an input whose last byte is out's first; touching ranges are allowed
        count, o0 = 64, 0x100000
        o1, span = o0 + 4 * count, esz * count
        for p in (o0, o0 + 2 * esz, o0 + 128, o1 - esz, o0 - span + esz, o0 - 2 * esz):
            _refused(_widened(dt, ins=(0x300000, p), count=count), "in[1] overlaps out")
        # 4 * count wraps a size_t
        for count in ((1 << 62), (1 << 62) + 5, (1 << 64) - 1):
            _refused(_widened(dt, count=count), "count overflows")
        for bad in (float("inf"), float("-inf"), float("nan")):
            _refused(_widened(dt, alpha=bad), "alpha must be finite")
        for bad in (1e300, -3.5e38):
            _refused(_widened(dt, alpha=bad), "finite as a float")
        _refused(_widened(dt, out=0), "out is NULL")
        _refused(_widened(dt, ins=(0,)), "in[0] is NULL")
        _refused(_widened(dt, cfg=L.ReduceConfig(acc=7)), "always accumulates in f32")
        _refused(_widened(dt, cfg=L.ReduceConfig(engine=9)), "bad engine")
        # count 0 is a no-op once the arguments are valid; alpha 0 and one that underflows are allowed
        for alpha in (None, 0.0, 1e-60, 0.5):
            assert _widened(dt, alpha=alpha, count=0) == 0, L.last_error()
    for bad_in in (L.HICCL_FLOAT32, L.HICCL_FLOAT64, L.HICCL_INT32, L.HICCL_UINT64, L.HICCL_BYTES, 7, 42):
        _refused(_widened(bad_in), "widened sums take")
        out = [ctypes.c_int() for _ in range(5)]
        rc = L.lib().hiccl_reduce_auto_choice_widened(bad_in, None, 1024, 2.0, 256, *[ctypes.byref(v) for v in out])
        _refused(rc, "widened sums take")
    lib = L.lib()
    assert lib.hiccl_reduce_plan_set_out_dtype(None, F32) == 1 and "plan is NULL" in L.last_error()
    assert lib.hiccl_reduce_plan_out_dtype(None) == -1


def test_unsupported_shapes_are_refused_never_replaced():
    """The widened kernels are untuned: TILE 256 x 4 and PHASE 512 x 16, nt
    loads, nt or write-through stores.  Any other shape is refused by
    auto_choice_widened (and so by the call, which resolves the same way)."""
    for kind, dt in IN_DTYPES.items():
        for cfg in (dict(engine=T, unroll=1), dict(engine=T, unroll=2), dict(engine=T, unroll=8),
                    dict(engine=T, unroll=16), dict(engine=T, block=512, unroll=4), dict(engine=P, block=512, unroll=8),
                    dict(engine=P, block=1024, unroll=4), dict(nontemporal=1), dict(store_policy=1),
                    dict(store_policy=3)):
            with pytest.raises(hiccl_amd.HicclError, match="no kernel"):
                hiccl_amd.auto_choice(dt, 1 << 20, 3, config=cfg, out_dtype=F32)
            # the call itself, on pointers that are not device memory: refused before any launch
            rc = _widened(dt, cfg=L.ReduceConfig(**cfg), ins=(0x200000, 0x300000, 0x400000), count=1 << 12)
            _refused(rc, "unsupported config")
        for cfg in (dict(engine=T, unroll=4), dict(engine=P), dict(engine=P, block=512, unroll=16),
                    dict(store_policy=2), dict(store_policy=4)):
            hiccl_amd.auto_choice(dt, 1 << 20, 3, config=cfg, out_dtype=F32)


def _plan(dtype):
    import torch
    if not torch.cuda.is_available() or torch.cuda.device_count() < 1:
        pytest.skip("no HIP device to bind a plan to")
    h = ctypes.c_void_p()
    assert L.lib().hiccl_reduce_plan_create(ctypes.byref(h), dtype, 0) == 0, L.last_error()
    return h


@pytest.mark.parametrize("kind", E.KINDS)
def test_plan_entries_and_their_refusals(kind):
    """set_out_dtype / out_dtype, the refusals of a widened plan, its buffer
    rules and hiccl_reduce_plan_bytes.  Nothing is launched: the pointers are
    not device memory."""
    lib, dt, esz = L.lib(), IN_DTYPES[kind], E.ESZ[kind]
    h = _plan(dt)
    half, got = ctypes.c_double(0.5), ctypes.c_double()
    try:
        assert lib.hiccl_reduce_plan_out_dtype(h) == dt
        for bad in (L.HICCL_FLOAT64, dt, 42):
            _refused(lib.hiccl_reduce_plan_set_out_dtype(h, bad), "plan_set_out_dtype", "HICCL_FLOAT32 only")
        # refused while the plan's acc is WIDE, its op not SUM, or its config a shape the kernels lack
        assert lib.hiccl_reduce_plan_set_acc(h, L.HICCL_ACC_WIDE) == 0
        _refused(lib.hiccl_reduce_plan_set_out_dtype(h, F32), "always accumulates in f32")
        assert lib.hiccl_reduce_plan_set_acc(h, L.HICCL_ACC_NATIVE) == 0
        assert lib.hiccl_reduce_plan_set_op(h, L.HICCL_OP_MAX) == 0
        _refused(lib.hiccl_reduce_plan_set_out_dtype(h, F32), "only sums are widened")
        assert lib.hiccl_reduce_plan_set_op(h, L.HICCL_OP_SUM) == 0
        if kind in E.HALVES:  # only the tuned types have a TILE unroll 2 to name
            tuned = L.ReduceConfig(engine=T, unroll=2)
            assert lib.hiccl_reduce_plan_set_config(h, ctypes.byref(tuned)) == 0, L.last_error()
            _refused(lib.hiccl_reduce_plan_set_out_dtype(h, F32), "shape the widened kernels lack")
            assert lib.hiccl_reduce_plan_set_config(h, None) == 0
        assert lib.hiccl_reduce_plan_out_dtype(h) == dt
        assert lib.hiccl_reduce_plan_set_out_dtype(h, F32) == 0, L.last_error()
        assert lib.hiccl_reduce_plan_out_dtype(h) == F32
        # a widened plan: SUM only, never WIDE, TILE 256 x 4 only; it takes a scale and peer flags
        for op in (L.HICCL_OP_MAX, L.HICCL_OP_MIN, L.HICCL_OP_PROD):
            _refused(lib.hiccl_reduce_plan_set_op(h, op), "plan_set_op")
        assert lib.hiccl_reduce_plan_set_op(h, L.HICCL_OP_SUM) == 0 and lib.hiccl_reduce_plan_op(h) == L.HICCL_OP_SUM
        _refused(lib.hiccl_reduce_plan_set_acc(h, L.HICCL_ACC_WIDE), "always accumulates in f32")
        wide = L.ReduceConfig(acc=L.HICCL_ACC_WIDE)
        _refused(lib.hiccl_reduce_plan_set_config(h, ctypes.byref(wide)), "plan_set_config", "always accumulates in f32")
        for unroll in (1, 2, 8, 16):
            cfg = L.ReduceConfig(engine=T, unroll=unroll)
            _refused(lib.hiccl_reduce_plan_set_config(h, ctypes.byref(cfg)), "plan_set_config")
        for cfg in (L.ReduceConfig(engine=T, unroll=4), L.ReduceConfig(engine=P), L.ReduceConfig()):
            assert lib.hiccl_reduce_plan_set_config(h, ctypes.byref(cfg)) == 0, L.last_error()
        assert lib.hiccl_reduce_plan_set_scale(h, ctypes.byref(half)) == 0, L.last_error()
        assert lib.hiccl_reduce_plan_scale(h, ctypes.byref(got)) == 1 and got.value == 0.5
        bad = ctypes.c_double(float("inf"))
        _refused(lib.hiccl_reduce_plan_set_scale(h, ctypes.byref(bad)), "finite")
        assert lib.hiccl_reduce_plan_set_scale(h, None) == 0 and lib.hiccl_reduce_plan_scale(h, None) == 0
        for flags in (L.HICCL_PEER_STORES, L.HICCL_PEER_LOADS, L.HICCL_PEER_STORES | L.HICCL_PEER_LOADS, 0):
            assert lib.hiccl_reduce_plan_set_peer(h, flags) == 0 and lib.hiccl_reduce_plan_peer(h) == flags
        # add: the widened buffer rules
        o0, count = 0x100000, 64
        _refused(lib.hiccl_reduce_plan_add(h, ctypes.c_void_p(o0 + 2), _tab([0x200000]), 1, count), "out is not aligned")
        for p in (o0, o0 + 128, o0 + 4 * count - esz):
            _refused(lib.hiccl_reduce_plan_add(h, ctypes.c_void_p(o0), _tab([0x300000, p]), 2, count), "overlaps out")
        _refused(lib.hiccl_reduce_plan_add(h, ctypes.c_void_p(o0), _tab([0x200000]), 1, 1 << 62), "count overflows")
        assert lib.hiccl_reduce_plan_numcomp(h) == 0 and lib.hiccl_reduce_plan_bytes(h) == 0
        assert lib.hiccl_reduce_plan_add(h, ctypes.c_void_p(o0), _tab([0x200000]), 1, 0) == 0  # count 0: dropped
        assert lib.hiccl_reduce_plan_add(h, ctypes.c_void_p(o0), _tab([0x200000, 0x300000, 0x400000]), 3, 1000) == 0
        assert lib.hiccl_reduce_plan_add(h, ctypes.c_void_p(0x500000), _tab([0x600000]), 1, 77) == 0
        assert lib.hiccl_reduce_plan_numcomp(h) == 2
        assert lib.hiccl_reduce_plan_bytes(h) == 1000 * (3 * esz + 4) + 77 * (esz + 4)
        # set_out_dtype after add
        _refused(lib.hiccl_reduce_plan_set_out_dtype(h, F32), "before the first add")
        assert lib.hiccl_reduce_plan_out_dtype(h) == F32
        # a program takes no widened plan
        prog = ctypes.c_void_p()
        assert lib.hiccl_program_create(ctypes.byref(prog), dt, 0) == 0, L.last_error()
        try:
            _refused(lib.hiccl_program_add_plan(prog, h), "program_add_plan", "widened")
        finally:
            lib.hiccl_program_destroy(prog)
    finally:
        lib.hiccl_reduce_plan_destroy(h)
    # an unwidened plan with computes refuses set_out_dtype too, and prices as before
    b = _plan(dt)
    try:
        assert lib.hiccl_reduce_plan_add(b, ctypes.c_void_p(0x100000), _tab([0x200000, 0x300000]), 2, 10) == 0
        _refused(lib.hiccl_reduce_plan_set_out_dtype(b, F32), "before the first add")
        assert lib.hiccl_reduce_plan_bytes(b) == 10 * 3 * esz and lib.hiccl_reduce_plan_out_dtype(b) == dt
    finally:
        lib.hiccl_reduce_plan_destroy(b)


def test_set_out_dtype_takes_the_four_input_dtypes_only():
    lib = L.lib()
    for dt in (L.HICCL_FLOAT32, L.HICCL_FLOAT64, L.HICCL_INT32, L.HICCL_UINT64, L.HICCL_BYTES):
        h = _plan(dt)
        try:
            _refused(lib.hiccl_reduce_plan_set_out_dtype(h, F32), "plan_set_out_dtype", "widened sums take")
            assert lib.hiccl_reduce_plan_out_dtype(h) == dt
        finally:
            lib.hiccl_reduce_plan_destroy(h)


# ---------------------------------------------------------------------- AUTO

def _rows():
    import auto_table as A
    rows = [(dt, count, n, None) for (dt, count, n), _ in A.RULE_CASES]
    rows += [k for k, _ in A.all_engine_rows()] + [k for k, _ in A.all_store_rows()]
    return rows


def test_auto_choice_widened_is_the_untuned_rule_on_output_packets():
    """The widened kernels have no tuning table and count their units in
    packets of the f32 output.  (a) The rows tests/auto_table.py has for f64:
    a widened sum that writes the same bytes (twice the elements) answers the
    table's own entry.  (b) Every row of the table, whatever its dtype: a
    widened sum of `count` elements answers what the f64 SUM -- untuned, the
    same 16-packet chunk -- answers for count / 2 elements, i.e. for the same
    output packets, bytes written and n; a shape the kernels lack is refused."""
    import auto_table as A
    f64_rows = [(count, n, want) for (dt, count, n), want in A.RULE_CASES if dt == A.F64]
    assert len(f64_rows) >= 2
    for dt in IN_DTYPES.values():
        for count, n, want in f64_rows:
            got = hiccl_amd.auto_choice(dt, 2 * count, n, out_dtype=F32)
            assert (got["engine"], got["unroll"], got["blocks_per_cu"], got["dynamic"]) == want, (dt, count, n, got)
    seen, rows = set(), 0
    for _, count, n, cfg in _rows():
        if cfg and cfg.get("acc"):
            continue  # a widened sum refuses WIDE
        count -= count % 2
        for dt in IN_DTYPES.values():
            try:
                want = hiccl_amd.auto_choice(L.HICCL_FLOAT64, count // 2, n, config=cfg)
            except hiccl_amd.HicclError:
                with pytest.raises(hiccl_amd.HicclError):
                    hiccl_amd.auto_choice(dt, count, n, config=cfg, out_dtype=F32)
                continue
            got = hiccl_amd.auto_choice(dt, count, n, config=cfg, out_dtype=F32)
            assert got == want, (dt, count, n, cfg, got, want)
            assert (got["engine"], got["unroll"]) in ((T, 4), (P, 16)) and got["store_policy"] in (2, 4)
            seen.add((got["engine"], got["store_policy"]))
            rows += 1
    assert {e for e, _ in seen} == {T, P} and {s for _, s in seen} == {2, 4} and rows > 80
    # the store form counts the bytes WRITTEN: 4 * count against the 256 MiB cap of sums
    for dt in IN_DTYPES.values():
        assert hiccl_amd.auto_choice(dt, 1 << 26, 8, out_dtype=F32)["store_policy"] == 4  # 256 MiB written
        assert hiccl_amd.auto_choice(dt, (1 << 26) + 4, 8, out_dtype=F32)["store_policy"] == 2
        got = hiccl_amd.auto_choice(dt, 1 << 16, 100, out_dtype=F32)  # n > 64: the plan kernel's default shapes
        assert (got["engine"], got["unroll"]) in ((T, 4), (P, 16))


# -------------------------------------------------------------- Python layer

def test_python_layer_refuses_before_any_device_work():
    import torch
    check = hiccl_amd.compute._check_widened
    for dt in (torch.bfloat16, torch.float16, torch.float8_e4m3fn, torch.float8_e5m2) + tuple(IN_DTYPES.values()):
        check(dt, torch.float32)
        check(dt, F32)
        for bad in (torch.float64, torch.bfloat16, torch.float16, L.HICCL_FLOAT64, L.HICCL_BFLOAT16):
            with pytest.raises(TypeError, match="writes torch.float32"):
                check(dt, bad)
    for bad in (torch.float32, torch.float64, torch.int32, torch.uint8, L.HICCL_FLOAT32, L.HICCL_INT32, L.HICCL_BYTES):
        with pytest.raises(TypeError, match="widened sums take"):
            check(bad, torch.float32)
    ptrs = hiccl_amd.reduce_widened_ptrs
    with pytest.raises(TypeError, match="widened sums take"):
        ptrs(L.HICCL_FLOAT32, 0x100000, [0x200000], 4)
    with pytest.raises(TypeError, match="writes torch.float32"):
        ptrs(L.HICCL_BFLOAT16, 0x100000, [0x200000], 4, out_dtype_code=L.HICCL_BFLOAT16)
    with pytest.raises(ValueError, match="finite"):
        ptrs(L.HICCL_BFLOAT16, 0x100000, [0x200000], 4, scale=float("inf"))
    with pytest.raises(TypeError, match="real number"):
        ptrs(L.HICCL_FLOAT16, 0x100000, [0x200000], 4, scale="2")
    with pytest.raises(ValueError, match="accumulates in f32"):
        ptrs(L.HICCL_FLOAT8_E4M3, 0x100000, [0x200000], 4, config=dict(acc=L.HICCL_ACC_WIDE))
    # what the Python layer lets through, the library still refuses with a message
    with pytest.raises(hiccl_amd.HicclError, match="overlaps out"):
        ptrs(L.HICCL_BFLOAT16, 0x100000, [0x100000], 4, stream=0)
    with pytest.raises(hiccl_amd.HicclError, match="finite as a float"):
        ptrs(L.HICCL_BFLOAT16, 0x100000, [0x200000], 4, scale=1e300, stream=0)
    with pytest.raises(TypeError, match="widened sums take"):
        hiccl_amd.auto_choice(torch.float32, 1024, 2, out_dtype=torch.float32)
    with pytest.raises(TypeError, match="writes torch.float32"):
        hiccl_amd.auto_choice(torch.bfloat16, 1024, 2, out_dtype=torch.float64)
    with pytest.raises(ValueError, match="only sums"):
        hiccl_amd.auto_choice(torch.bfloat16, 1024, 2, out_dtype=torch.float32, op=L.HICCL_OP_MAX)
    with pytest.raises(ValueError, match="accumulates in f32"):
        hiccl_amd.auto_choice(torch.bfloat16, 1024, 2, out_dtype=torch.float32, config=dict(acc=L.HICCL_ACC_WIDE))
    # host tensors: refused by reduce_widened as by reduce; reduce() keeps refusing mixed dtypes
    x, out = torch.zeros(8, dtype=torch.bfloat16), torch.zeros(8)
    with pytest.raises(ValueError, match="device tensor"):
        hiccl_amd.reduce_widened(out, [x])
    # the Compute constructor checks before it creates a plan
    for kw, exc, match in ((dict(dtype=torch.float32, out_dtype=torch.float32), TypeError, "widened sums take"),
                           (dict(dtype=torch.bfloat16, out_dtype=torch.float16), TypeError, "writes torch.float32"),
                           (dict(dtype=torch.bfloat16, out_dtype=torch.float32, op=L.HICCL_OP_MAX), ValueError, "only sums"),
                           (dict(dtype=torch.float16, out_dtype=torch.float32, acc=L.HICCL_ACC_WIDE), ValueError,
                            "accumulates in f32")):
        with pytest.raises(exc, match=match):
            hiccl_amd.Compute(device=0, **kw)


# ----------------------------------------------- restatement against fixtures

def _manifest():
    with open(os.path.join(GOLDEN, "manifest_widen.json")) as fh:
        return json.load(fh)


def test_manifest_records_files_inputs_and_alphas():
    m = _manifest()
    assert len(m["files"]) >= 4
    for fname, info in m["files"].items():
        path = os.path.join(GOLDEN, fname)
        assert os.path.getsize(path) == info["bytes"] < (1 << 20)
        assert hashlib.sha256(open(path, "rb").read()).hexdigest() == info["sha256"]
    assert [[name, float(a).hex()] for name, a in E.ALPHAS] == m["alphas"]
    assert [a for _, a in E.ALPHAS] == [1.0, 0.5, 1 / 3, -1 / 1024, 2.0 ** -20, 1e30, 0.0]
    assert E.COUNT == 4102 and E.NS == (1, 2, 3, 8, 9, 17)
    for kind in E.KINDS:
        for n in E.NS:  # the inputs are not stored: the generators must still give what the fixtures were made from
            assert E.array_hash(E.inputs(kind, n)) == m["inputs"][f"{kind}/n{n}"], (kind, n)
    assert set(m["patterns"]) == set(E.KINDS)


@pytest.mark.parametrize("kind", E.KINDS)
def test_restatement_gives_the_stored_outputs(kind):
    """widen_expected.widened on the generated inputs = the stored words of the
    reference's f32 reduce_kernel on the widened inputs, for every n and alpha;
    at most NAN_CAP of any array is NaN; alpha = 1 gives the sum's words."""
    cases = load_golden(f"reduce_widen_{kind}")
    assert sorted(cases) == sorted(f"n{n}" for n in E.NS)
    for n in E.NS:
        d, x = cases[f"n{n}"], E.inputs(kind, n)
        assert sorted(d) == sorted(["s"] + [f"a{i}" for i in range(1, len(E.ALPHAS))])
        s = E.widened(kind, x)
        E.assert_nan_cap(d["s"])
        E.assert_equal(s, d["s"], f"{kind} n={n}")
        E.assert_equal(E.widened(kind, x, 1.0), d["s"], f"{kind} n={n} alpha 1")
        for i, (name, alpha) in enumerate(E.ALPHAS):
            if i == 0:
                continue
            E.assert_nan_cap(d[f"a{i}"], d["s"] if alpha == 0.0 else None)
            E.assert_equal(E.widened(kind, x, alpha), d[f"a{i}"], f"{kind} n={n} alpha {name}")
            nan = np.isnan(d[f"a{i}"])
            assert np.array_equal(nan, ~np.isfinite(d["s"]) if alpha == 0.0 else np.isnan(d["s"])), (kind, n, name)
        if n >= 2 and kind in E.HALVES:  # the hostile classes are all there: NaN, Inf and subnormal sums
            assert np.isnan(d["s"]).any() and np.isinf(d["s"]).any()
        if n >= 2 and kind == "bf16":  # bf16's subnormals are f32's: the sums stay subnormal
            assert ((np.abs(d["s"]) < np.float32(2.0 ** -126)) & (d["s"] != 0)).any()


@pytest.mark.parametrize("kind", E.KINDS)
def test_semantics_of_the_definition(kind):
    """The rules of the contract on the restatement: all -0 inputs give +0,
    n == 0 gives +0 (scaled: a zero with alpha's sign), Inf + -Inf and an e4m3
    NaN code give NaN, nothing is clamped, subnormals are kept, and s32 is the
    f32-accumulating sum before its final rounding."""
    neg0 = {"bf16": 0x8000, "f16": 0x8000, "e4m3": 0x80, "e5m2": 0x80}[kind]
    x = np.full((3, 8), neg0, E.CARRIER[kind])
    assert (E.widen(kind, x) == 0).all() and np.signbit(E.widen(kind, x)).all()
    s = E.widened(kind, x)
    assert (s.view(np.uint32) == 0).all()
    z = E.widened(kind, np.empty((0, 5), E.CARRIER[kind]), count=5)
    assert (z.view(np.uint32) == 0).all()
    assert (E.widened(kind, np.empty((0, 5), E.CARRIER[kind]), -0.5, count=5).view(np.uint32) == 0x80000000).all()
    if kind == "e4m3":
        assert np.isnan(E.widen(kind, np.array([0x7F, 0xFF], np.uint8))).all()
        big = np.full((17, 4), 0x7E, np.uint8)  # 17 x 448: no clamp
        assert (E.widened(kind, big) == np.float32(17 * 448)).all()
    else:
        inf = {"bf16": (0x7F80, 0xFF80), "f16": (0x7C00, 0xFC00), "e5m2": (0x7C, 0xFC)}[kind]
        assert np.isnan(E.widened(kind, np.array([[inf[0]], [inf[1]]], E.CARRIER[kind]))).all()
    sub = np.array([[1], [1], [1]], E.CARRIER[kind])  # three times the smallest subnormal: exact in f32
    unit = float(E.widen(kind, np.array([1], E.CARRIER[kind]))[0])
    assert unit > 0 and float(E.widened(kind, sub)[0]) == 3 * unit


@pytest.mark.parametrize("kind", E.KINDS)
def test_every_pattern_against_sixteen_addends(kind):
    """Every 16-bit pattern (bf16, f16) or byte (FP8) plus each of 16 addends:
    the restatement's words hash to what the reference gave
    (manifest_widen.json)."""
    exp = E.patterns_expected(kind)
    assert exp.shape == (16, 1 << (8 * E.ESZ[kind]))
    assert E.words_hash(exp) == _manifest()["patterns"][kind]


# ------------------------------------------------------------- the C++ layer

def _run_widen_sum(exe, tmp_path, tag, env=None):
    n, alpha = 9, 1.0 / 3.0
    for kind in E.KINDS:
        x = E.inputs(kind, n)
        inp, out = tmp_path / f"{tag}_{kind}.in", tmp_path / f"{tag}_{kind}.out"
        np.ascontiguousarray(x).tofile(inp)
        p = subprocess.run([str(exe), kind, str(inp), str(out), str(n), str(E.COUNT), float(alpha).hex()],
                           capture_output=True, text=True, env=env)
        assert p.returncode == 0 and "widen_sum: PASSED" in p.stdout, p.stdout + p.stderr
        assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr
        cases = load_golden(f"reduce_widen_{kind}")[f"n{n}"]
        i = [a for _, a in E.ALPHAS].index(alpha)
        E.assert_equal(np.fromfile(str(out) + ".plain", np.float32), cases["s"], f"WidenCompute<{kind}> plain")
        E.assert_equal(np.fromfile(str(out), np.float32), cases[f"a{i}"], f"WidenCompute<{kind}> scaled")
        E.assert_equal(np.fromfile(str(out) + ".cleared", np.float32), cases["s"], f"WidenCompute<{kind}> cleared")


def test_widen_compute_on_the_host_port(tmp_path):
    """tests/cpp/widen_sum.cpp built with HICCL_PORT_HOST: WidenCompute<T> for
    the four types on the fixtures' inputs gives the fixtures' words, plain,
    scaled and after clear_scale."""
    make(ROOT, "build/widen_sum")
    _run_widen_sum(os.path.join(ROOT, "build", "widen_sum"), tmp_path, "plain")


def _mpi():
    inc = os.environ.get("MPI_INC", "/opt/conda/include")
    lib = os.environ.get("MPI_LIB", "/opt/conda/lib")
    return inc, lib


def test_widen_compute_host_port_under_sanitizers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined and
    run as a program (no preload), as tests/test_f8_cpu.py runs f8_add.cpp."""
    inc, lib = _mpi()
    exe = tmp_path / "widen_sum_san"
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-DHICCL_PORT_HOST", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"), "-I", inc,
                         os.path.join(ROOT, "tests", "cpp", "widen_sum.cpp"), "-o", str(exe),
                         os.path.join(lib, "libmpi.so"), f"-Wl,-rpath,/usr/lib/x86_64-linux-gnu:{lib}"],
                        capture_output=True, text=True)
    if cc.returncode != 0 and ("asan" in cc.stderr or "ubsan" in cc.stderr or "sanitize" in cc.stderr):
        pytest.skip("g++ has no sanitizer runtimes here: " + cc.stderr.strip()[-200:])
    assert cc.returncode == 0, cc.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    _run_widen_sum(exe, tmp_path, "san", env)


def test_widen_compute_rejects_other_types_at_compile_time(tmp_path):
    inc = ["-I", os.path.join(ROOT, "include"), "-I", _mpi()[0], "-DHICCL_PORT_HOST"]
    ok = tmp_path / "ok.cpp"
    ok.write_text('#include "hiccl/compute.h"\nusing namespace HiCCL;\n'
                  "void f() { WidenCompute<bf16> a; a.set_scale(0.5); a.clear_scale(); WidenCompute<f16> b; (void)b;\n"
                  "           WidenCompute<f8e4m3> c; (void)c; WidenCompute<f8e5m2> d; (void)d;\n"
                  "#ifdef __FLT16_MANT_DIG__\n           WidenCompute<_Float16> e; (void)e;\n#endif\n}\n"
                  "int main() { return 0; }\n")
    cc = subprocess.run(["g++", "-std=c++17", "-fsyntax-only"] + inc + [str(ok)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    for t in ("float", "double", "int32_t", "uint64_t", "maxof<bf16>"):
        bad = tmp_path / "bad.cpp"
        bad.write_text(f'#include "hiccl/compute.h"\nusing namespace HiCCL;\nWidenCompute<{t}> x;\nint main() {{ return 0; }}\n')
        cc = subprocess.run(["g++", "-std=c++17", "-fsyntax-only"] + inc + [str(bad)], capture_output=True, text=True)
        assert cc.returncode != 0 and "static assertion failed" in cc.stderr and "WidenCompute" in cc.stderr, \
            t + cc.stderr[-2000:]
