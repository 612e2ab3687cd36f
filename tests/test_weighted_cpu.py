"""CPU tier of the weighted widened sums (hiccl_reduce_weighted,
hiccl_reduce_plan_set_weighted / _add_weighted, Python weights=,
WidenCompute<T>::add with weights on the host port, plain and under
sanitizers).  No test here launches a kernel: the one-shot refusals come before
any device work and take pointers that are not device memory; the plan's
entries need a device to bind the plan to and skip without one, as the
accumulating sums' do (tests/test_accum_cpu.py).

The fixtures (tests/golden/reduce_weighted_*.npz) are the reference's
reduce_kernel<float> on pre-multiplied rows; here the restatement
(tests/weighted_expected.py) is pinned to the stored words again, without the
reference, and the manifest's counts are recomputed.
"""
import ctypes
import inspect
import json
import os
import subprocess

import numpy as np
import pytest

import accum_expected as A
import hiccl_amd
import weighted_expected as X
import widen_expected as E
from conftest import GOLDEN, ROOT, load_golden, make
from hiccl_amd import _lib as L

IN_DTYPES = {k: E.CODE[k] for k in E.KINDS}
NEW_SYMBOLS = ("hiccl_reduce_weighted", "hiccl_reduce_auto_choice_weighted", "hiccl_reduce_plan_set_weighted",
               "hiccl_reduce_plan_weighted", "hiccl_reduce_plan_add_weighted")
F32 = L.HICCL_FLOAT32
T, P = L.HICCL_ENGINE_TILE, L.HICCL_ENGINE_PHASE
OUT, IN0, WTS = 0x100000, 0x200000, 0x400000  # not device memory: every call below is refused before it matters


def _tab(ptrs):
    return (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs)


def _weighted(in_dtype, out_dtype=F32, alpha=None, accumulate=0, cfg=None, ins=(IN0,), weights=WTS, out=OUT, count=4):
    a = ctypes.byref(ctypes.c_double(alpha)) if alpha is not None else None
    return L.lib().hiccl_reduce_weighted(in_dtype, out_dtype, a, accumulate, ctypes.c_void_p(out), _tab(list(ins)),
                                         ctypes.c_void_p(weights), len(ins), count, None,
                                         ctypes.byref(cfg) if cfg is not None else None)


def _refused(rc, *words):
    msg = L.last_error()
    assert rc == 1 and msg and all(w in msg for w in words), (rc, msg, words)


# ----------------------------------------------------------------------- ABI

def test_new_symbols_are_declared_bound_and_exported():
    declared = L.header_functions()
    for name in NEW_SYMBOLS:
        assert name in declared and name in L._SIGS and hasattr(L.lib(), name), name
    assert L.lib().hiccl_version() >= 1000  # 0.9.0 had no weighted sums
    for fn in (hiccl_amd.reduce_widened, hiccl_amd.reduce_widened_ptrs, hiccl_amd.Compute.add):
        assert inspect.signature(fn).parameters["weights"].default is None, fn
    for fn in (hiccl_amd.auto_choice, hiccl_amd.Compute.__init__):
        assert inspect.signature(fn).parameters["weighted"].default is False, fn


def test_one_shot_refusals_return_invalid_value_with_a_message():
    """hiccl_reduce_weighted applies hiccl_reduce_widened's checks and its own
    -- weights NULL, misaligned, overlapping the output -- before any device
    work, with return code 1 and a message."""
    for kind, dt in IN_DTYPES.items():
        esz = E.ESZ[kind]
        for accumulate in (0, 1):
            for bad_out in (L.HICCL_FLOAT64, L.HICCL_BFLOAT16, dt, 42):
                _refused(_weighted(dt, bad_out, accumulate=accumulate), "hiccl_reduce_weighted", "HICCL_FLOAT32 only")
            _refused(_weighted(dt, cfg=L.ReduceConfig(acc=L.HICCL_ACC_WIDE), accumulate=accumulate), "hiccl_reduce_weighted",
                     "always accumulates in f32")
            _refused(_weighted(dt, out=OUT + 2, accumulate=accumulate), "out is not aligned")
            _refused(_weighted(dt, ins=(IN0, OUT + 4), count=64, accumulate=accumulate), "in[1] overlaps out")
            _refused(_weighted(dt, alpha=float("nan"), accumulate=accumulate), "alpha must be finite")
            _refused(_weighted(dt, out=0, accumulate=accumulate), "out is NULL")
            # the weights: NULL, misaligned, overlapping the count f32 outputs (n floats from `weights` on)
            _refused(_weighted(dt, weights=0, accumulate=accumulate), "hiccl_reduce_weighted", "weights is NULL")
            for mis in (1, 2, 3):
                _refused(_weighted(dt, weights=WTS + mis, accumulate=accumulate), "weights must be 4-byte aligned")
            count, n = 64, 3
            ins = tuple(IN0 + k * 0x10000 for k in range(n))
            for w in (OUT, OUT + 4, OUT + 4 * count - 4, OUT - 4 * n + 4, OUT - 4):
                _refused(_weighted(dt, ins=ins, weights=w, count=count, accumulate=accumulate), "weights overlap the output")
            # n == 0: the weights may be NULL; count 0 is a no-op once the arguments are valid
            assert _weighted(dt, ins=(), weights=0, count=0, accumulate=accumulate) == 0, L.last_error()
            assert _weighted(dt, count=0, accumulate=accumulate) == 0, L.last_error()
            if esz == 2:
                _refused(_weighted(dt, ins=(IN0 + 1,), accumulate=accumulate), "in[0] is not element-aligned")
    for bad_in in (L.HICCL_FLOAT32, L.HICCL_FLOAT64, L.HICCL_INT32, L.HICCL_BYTES, 42):
        _refused(_weighted(bad_in), "hiccl_reduce_weighted", "widened sums take")
        out = [ctypes.c_int() for _ in range(5)]
        rc = L.lib().hiccl_reduce_auto_choice_weighted(bad_in, 0, None, 1024, 2.0, 256, *[ctypes.byref(v) for v in out])
        _refused(rc, "auto_choice_weighted", "widened sums take")
    lib = L.lib()
    assert lib.hiccl_reduce_plan_set_weighted(None, 1) == 1 and "plan is NULL" in L.last_error()
    assert lib.hiccl_reduce_plan_weighted(None) == -1
    assert lib.hiccl_reduce_plan_add_weighted(None, None, None, None, 0, 0) == 1 and "plan is NULL" in L.last_error()


def test_unsupported_shapes_are_refused_never_replaced():
    """The weighted kernels cover what their unweighted families cover: TILE 256
    x 4 and PHASE's default chunk -- 16 packets per lane overwriting, 8
    accumulating -- nt loads, nt or write-through stores."""
    for dt in IN_DTYPES.values():
        for accumulate, mine, other in ((False, 16, 8), (True, 8, 16)):
            for cfg in (dict(engine=T, unroll=1), dict(engine=T, unroll=2), dict(engine=T, unroll=8),
                        dict(engine=T, block=512, unroll=4), dict(engine=P, block=512, unroll=other),
                        dict(engine=P, block=1024, unroll=4), dict(nontemporal=1), dict(store_policy=1)):
                with pytest.raises(hiccl_amd.HicclError, match="no kernel"):
                    hiccl_amd.auto_choice(dt, 1 << 20, 3, config=cfg, out_dtype=F32, accumulate=accumulate, weighted=True)
                rc = _weighted(dt, cfg=L.ReduceConfig(**cfg), accumulate=int(accumulate), ins=(IN0, IN0 + 0x10000),
                               count=1 << 12)
                _refused(rc, "unsupported config")
            for cfg in (dict(engine=T, unroll=4), dict(engine=P), dict(engine=P, block=512, unroll=mine),
                        dict(store_policy=2), dict(store_policy=4)):
                got = hiccl_amd.auto_choice(dt, 1 << 20, 3, config=cfg, out_dtype=F32, accumulate=accumulate, weighted=True)
                assert (got["engine"], got["unroll"]) in ((T, 4), (P, mine))


def _plan(dtype):
    import torch
    if not torch.cuda.is_available() or torch.cuda.device_count() < 1:
        pytest.skip("no HIP device to bind a plan to")
    h = ctypes.c_void_p()
    assert L.lib().hiccl_reduce_plan_create(ctypes.byref(h), dtype, 0) == 0, L.last_error()
    return h


@pytest.mark.parametrize("kind", E.KINDS)
def test_plan_entries_and_their_refusals(kind):
    """set_weighted / weighted / add_weighted and their refusals, with pointers
    that are not device memory (nothing is launched)."""
    lib, dt, esz = L.lib(), E.CODE[kind], E.ESZ[kind]
    vp = ctypes.c_void_p
    h = _plan(dt)
    try:
        assert lib.hiccl_reduce_plan_weighted(h) == 0
        _refused(lib.hiccl_reduce_plan_set_weighted(h, 1), "plan_set_weighted", "only a widened plan is weighted")
        assert lib.hiccl_reduce_plan_set_out_dtype(h, F32) == 0, L.last_error()
        # an unweighted plan refuses add_weighted
        _refused(lib.hiccl_reduce_plan_add_weighted(h, vp(OUT), _tab([IN0]), vp(WTS), 1, 64), "plan_add_weighted",
                 "the plan is not weighted")
        assert lib.hiccl_reduce_plan_set_weighted(h, 1) == 0, L.last_error()
        assert lib.hiccl_reduce_plan_weighted(h) == 1
        # a weighted plan refuses the plain adds
        _refused(lib.hiccl_reduce_plan_add(h, vp(OUT), _tab([IN0]), 1, 64), "plan_add", "weighted computes only")
        _refused(lib.hiccl_reduce_plan_add_unscaled(h, vp(OUT), _tab([IN0]), 1, 64), "plan_add_unscaled",
                 "weighted computes only")
        _refused(lib.hiccl_reduce_plan_add_weighted(h, vp(OUT), _tab([IN0]), vp(0), 1, 64), "weights is NULL")
        _refused(lib.hiccl_reduce_plan_add_weighted(h, vp(OUT), _tab([IN0]), vp(WTS + 2), 1, 64), "4-byte aligned")
        _refused(lib.hiccl_reduce_plan_add_weighted(h, vp(OUT), _tab([IN0]), vp(OUT + 8), 1, 64), "weights overlap the output")
        _refused(lib.hiccl_reduce_plan_add_weighted(h, vp(OUT), _tab([OUT + 4 * 64 - esz]), vp(WTS), 1, 64), "overlaps out")
        assert lib.hiccl_reduce_plan_numcomp(h) == 0
        # set_accumulate and set_scale as on a widened plan; PEER_STORES with accumulate refused from either side
        a = ctypes.c_double(1.0 / 3.0)
        assert lib.hiccl_reduce_plan_set_scale(h, ctypes.byref(a)) == 0, L.last_error()
        assert lib.hiccl_reduce_plan_set_peer(h, L.HICCL_PEER_STORES) == 0
        _refused(lib.hiccl_reduce_plan_set_accumulate(h, 1), "plan_set_accumulate", "HICCL_PEER_STORES")
        assert lib.hiccl_reduce_plan_set_peer(h, L.HICCL_PEER_LOADS) == 0
        assert lib.hiccl_reduce_plan_set_accumulate(h, 1) == 0, L.last_error()
        _refused(lib.hiccl_reduce_plan_set_peer(h, L.HICCL_PEER_STORES), "plan_set_peer", "HICCL_PEER_STORES")
        # a config that names the other family's PHASE shape is refused, never replaced
        cfg = L.ReduceConfig(engine=P, block=512, unroll=16)
        _refused(lib.hiccl_reduce_plan_set_config(h, ctypes.byref(cfg)), "plan_set_config", "unroll 8")
        cfg = L.ReduceConfig(engine=P, block=512, unroll=8)
        assert lib.hiccl_reduce_plan_set_config(h, ctypes.byref(cfg)) == 0, L.last_error()
        _refused(lib.hiccl_reduce_plan_set_accumulate(h, 0), "plan_set_accumulate", "unroll 16")
        assert lib.hiccl_reduce_plan_accumulate(h) == 1
        # an add, then the switch is refused; bytes() prices the accumulating form, the weights not counted
        assert lib.hiccl_reduce_plan_add_weighted(h, vp(OUT), _tab([IN0, IN0 + 0x10000]), vp(WTS), 2, 64) == 0, L.last_error()
        assert lib.hiccl_reduce_plan_bytes(h) == 64 * (2 * esz + 8)
        _refused(lib.hiccl_reduce_plan_set_weighted(h, 0), "plan_set_weighted", "before the first add")
        assert lib.hiccl_reduce_plan_weighted(h) == 1
        prog = ctypes.c_void_p()
        assert lib.hiccl_program_create(ctypes.byref(prog), dt, 0) == 0, L.last_error()
        try:
            _refused(lib.hiccl_program_add_plan(prog, h), "program_add_plan", "widened")
        finally:
            lib.hiccl_program_destroy(prog)
    finally:
        lib.hiccl_reduce_plan_destroy(h)


# ---------------------------------------------------------------------- AUTO

def test_auto_choice_weighted_equals_the_unweighted_answers():
    """hiccl_reduce_auto_choice_weighted answers what
    hiccl_reduce_auto_choice_widened / _accumulate answer, field for field --
    the chunks are the same (16 overwriting, 8 accumulating), so `unroll` too --
    row for row of tests/auto_table.py, refusals included."""
    import auto_table as AT
    rows = [(count, n, None) for (_, count, n), _ in AT.RULE_CASES]
    rows += [(k[1], k[2], k[3]) for k, _ in AT.all_engine_rows()] + [(k[1], k[2], k[3]) for k, _ in AT.all_store_rows()]
    rows += [(1 << 24, 3, dict(engine=P, block=512, unroll=u)) for u in (4, 8, 16)] + [(1 << 16, 100, None)]
    seen, engines = 0, set()
    for count, n, cfg in rows:
        if cfg and cfg.get("acc"):
            continue
        for dt in IN_DTYPES.values():
            for accumulate in (False, True):
                try:
                    want = hiccl_amd.auto_choice(dt, count, n, config=cfg, out_dtype=F32, accumulate=accumulate)
                except hiccl_amd.HicclError:
                    with pytest.raises(hiccl_amd.HicclError):
                        hiccl_amd.auto_choice(dt, count, n, config=cfg, out_dtype=F32, accumulate=accumulate, weighted=True)
                    continue
                got = hiccl_amd.auto_choice(dt, count, n, config=cfg, out_dtype=F32, accumulate=accumulate, weighted=True)
                assert got == want, (dt, count, n, cfg, accumulate, got, want)
                engines.add(got["engine"])
                seen += 1
    assert seen > 160 and engines == {T, P}
    with pytest.raises(ValueError, match="only a widened sum is weighted"):
        hiccl_amd.auto_choice(L.HICCL_BFLOAT16, 1024, 2, weighted=True)


# -------------------------------------------------------------- Python layer

def test_python_layer_refuses_before_any_device_work():
    import torch
    ptrs = hiccl_amd.reduce_widened_ptrs
    w = torch.ones(2, dtype=torch.float32)  # a CPU tensor
    with pytest.raises(TypeError, match="torch.float32 tensor"):
        ptrs(L.HICCL_BFLOAT16, OUT, [IN0, IN0 + 0x10000], 4, weights=[1.0, 2.0])
    with pytest.raises(TypeError, match="torch.float32 tensor"):
        ptrs(L.HICCL_BFLOAT16, OUT, [IN0, IN0 + 0x10000], 4, weights=np.ones(2, np.float32))
    with pytest.raises(TypeError, match="must be torch.float32"):
        ptrs(L.HICCL_BFLOAT16, OUT, [IN0, IN0 + 0x10000], 4, weights=w.double())
    with pytest.raises(ValueError, match="device memory"):
        ptrs(L.HICCL_BFLOAT16, OUT, [IN0, IN0 + 0x10000], 4, weights=w)
    with pytest.raises(ValueError, match="only a widened plan is weighted"):
        hiccl_amd.Compute(torch.bfloat16, device=0, weighted=True)


# ------------------------------------------------------------------ fixtures

def _manifest():
    with open(os.path.join(GOLDEN, "manifest_weighted.json")) as fh:
        return json.load(fh)


def test_weight_sets_are_the_manifest_s():
    m = _manifest()
    for name in X.WEIGHT_SETS:
        for n in X.NS:
            w = X.weights(name, n)
            assert [float(v).hex() for v in w] == m["weights"][f"{name}/n{n}"]
            assert w.dtype == np.float32 and w.shape == (n,)
    assert (X.weights("ones", 9) == 1).all() and X.weights("onezero", 9)[4] == 0 and X.weights("onezero", 1)[0] == 0
    assert np.array_equal(X.weights("extreme", 7), np.array([2.0 ** -20, 1e30, -1 / 1024, 3, 1 + 2.0 ** -23, 2.0 ** -20, 1e30],
                                                           np.float32))
    assert np.array_equal(X.weights("signs", 3), np.array([1 / 3, -(1 / 3 + 1 / 16), 1 / 3 + 2 / 16]).astype(np.float32))
    assert np.array_equal(X.weights("dequant", 6), (np.array([0.7, 0.8 / 2, 0.9 / 4, 1.0 / 8, 1.1 / 16, 1.2])).astype(np.float32))


@pytest.mark.parametrize("kind", X.KINDS)
def test_restatement_gives_the_stored_outputs(kind):
    """Every stored array against tests/weighted_expected.py, and the
    manifest's conditions recomputed: `ones` is the stored widened sum, the NaN
    cap, the fused emulation, the unweighted sum and the rotated weights all
    differ where the manifest says they do."""
    m = _manifest()
    fix, widen = load_golden(f"reduce_weighted_{kind}"), load_golden(f"reduce_widen_{kind}")
    cond, stored = m["conditions"], 0
    for n in X.NS:
        x, p, d, tag = E.inputs(kind, n), A.prior(kind, n), fix[f"n{n}"], f"{kind}/n{n}"
        plain = E.widened(kind, x)
        worst_over = worst_acc = 0.0
        for name, alpha in X.OVER_CASES:
            w, key = X.weights(name, n), f"{name}.{X.alpha_name(alpha)}"
            exp = X.weighted(kind, x, w, alpha)
            E.assert_equal(exp, d[key], f"{kind} n={n} {key}")
            E.assert_nan_cap(exp)
            worst_over = max(worst_over, float(np.isnan(exp).mean()))
            stored += 1
            if alpha is not None:
                continue
            if name == "ones":
                E.assert_equal(exp, widen[f"n{n}"]["s"], f"{kind} n={n}: all-ones weights against the stored widened sum")
                assert cond["ones"][tag] == exp.size
            else:
                assert len(E.mismatches(plain, exp)) == cond["weighted"][f"{tag}/{name}"] >= 1
            if name in ("dequant", "signs") and n >= 2:
                assert len(E.mismatches(X.fused(kind, x, w), exp)) == cond["fusion"][f"{tag}/{name}"] >= 1
            if name == "dequant" and n >= 2:
                assert len(E.mismatches(X.weighted(kind, x, X.rotated(w)), exp)) == cond["rotation"][tag] >= 1
        for name, alpha in X.ACCUM_CASES:
            w, key = X.weights(name, n), f"acc.{name}.{X.alpha_name(alpha)}"
            exp = X.accumulated(kind, x, w, p, alpha)
            E.assert_equal(exp, d[key], f"{kind} n={n} {key}")
            E.assert_nan_cap(exp)
            worst_acc = max(worst_acc, float(np.isnan(exp).mean()))
            stored += 1
        assert m["shares"][tag] == {"nan_worst_over": round(worst_over, 4), "nan_worst_accum": round(worst_acc, 4)}
        assert len(d) == len(X.OVER_CASES) + len(X.ACCUM_CASES)
    assert stored == len(X.NS) * 13
    assert all(f"{kind}/n1/{s}" not in cond["fusion"] for s in ("dequant", "signs"))  # equal by construction at n = 1
    for fname, info in m["files"].items():
        assert os.path.getsize(os.path.join(GOLDEN, fname)) == info["bytes"] < (1 << 20)


def test_fused_restatement_is_a_single_rounding():
    """weighted_expected.fused on a case worked by hand: w = 1 + 2^-23 and
    x = 1 + 2^-7 (bf16) after acc = 1: the product 1 + 2^-7 + 2^-23 + 2^-30
    rounds to 1 + 2^-7 + 2^-23 first (two roundings: the sum 2 + 2^-7 + 2^-23 is
    a tie, to even 2 + 2^-7), while the single rounding sees the 2^-30 and
    rounds up."""
    x = np.array([[0x3F80], [0x3F81]], np.uint16)
    w = np.array([1.0, 1.0 + 2.0 ** -23], np.float32)
    two = X.weighted("bf16", x, w)
    one = X.fused("bf16", x, w)
    assert two[0] == np.float32(2.0 + 2.0 ** -7) and one[0] == np.float32(2.0 + 2.0 ** -7 + 2.0 ** -22)


# ------------------------------------------------------------- the C++ layer

def _run_weighted_sum(exe, tmp_path, tag, env=None):
    n = 9
    for kind in ("bf16", "e4m3"):
        x, p = E.inputs(kind, n), A.prior(kind, n)
        d = load_golden(f"reduce_weighted_{kind}")[f"n{n}"]
        inp, wts, pri, out = (tmp_path / f"{tag}_{kind}.{s}" for s in ("in", "w", "prior", "out"))
        np.ascontiguousarray(x).tofile(inp)
        X.weights("dequant", n).tofile(wts)
        np.ascontiguousarray(p).tofile(pri)
        r = subprocess.run([str(exe), kind, str(inp), str(wts), str(pri), str(out), str(n), str(X.COUNT),
                            float(X.THIRD).hex()], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and "weighted_sum: PASSED" in r.stdout, r.stdout + r.stderr
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
        E.assert_equal(np.fromfile(str(out), np.float32), d["dequant.third"], f"WidenCompute<{kind}> weighted")
        E.assert_equal(np.fromfile(str(out) + ".accum", np.float32), d["acc.dequant.third"],
                       f"WidenCompute<{kind}> weighted, accumulating")


def test_weighted_compute_on_the_host_port(tmp_path):
    """tests/cpp/weighted_sum.cpp built with HICCL_PORT_HOST: WidenCompute<T>
    with weights for bf16 and e4m3, overwriting and accumulating, on the
    fixtures' inputs, weights and priors."""
    make(ROOT, "build/weighted_sum")
    _run_weighted_sum(os.path.join(ROOT, "build", "weighted_sum"), tmp_path, "plain")


def test_weighted_compute_host_port_under_sanitizers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined and
    run as a program (no preload), as tests/test_widen_cpu.py runs widen_sum."""
    inc = os.environ.get("MPI_INC", "/opt/conda/include")
    lib = os.environ.get("MPI_LIB", "/opt/conda/lib")
    exe = tmp_path / "weighted_sum_san"
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-DHICCL_PORT_HOST", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"), "-I", inc,
                         os.path.join(ROOT, "tests", "cpp", "weighted_sum.cpp"), "-o", str(exe),
                         os.path.join(lib, "libmpi.so"), f"-Wl,-rpath,/usr/lib/x86_64-linux-gnu:{lib}"],
                        capture_output=True, text=True)
    if cc.returncode != 0 and ("asan" in cc.stderr or "ubsan" in cc.stderr or "sanitize" in cc.stderr):
        pytest.skip("g++ has no sanitizer runtimes here: " + cc.stderr.strip()[-200:])
    assert cc.returncode == 0, cc.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    _run_weighted_sum(exe, tmp_path, "san", env)
