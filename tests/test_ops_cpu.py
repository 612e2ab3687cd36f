"""CPU tier of the MAX / MIN operators (hiccl_op_t): the C ABI's new entries
and refusals, AUTO's answers, the NumPy restatement (tests/ops_expected.py)
against the stored fixtures, and the C++ wrapper types HiCCL::maxof<U> /
minof<U> (include/hiccl/ops.h) on the host.  No test here needs a GPU or the
reference; the fixtures pin the restatement to the reference's own
reduce_kernel (tests/golden/make_golden_ops.py).
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import hiccl_amd
import hostile as H32
import hostile_f16 as H16
import ops_expected as E
from conftest import GOLDEN, ROOT, load_golden, make
from hiccl_amd import _lib as L

COUNT = 17 * 241 + 5
NS = (1, 2, 3, 8, 9, 17)
SUM, MAX, MIN = L.HICCL_OP_SUM, L.HICCL_OP_MAX, L.HICCL_OP_MIN
T, P = L.HICCL_ENGINE_TILE, L.HICCL_ENGINE_PHASE
NEW_SYMBOLS = ("hiccl_reduce_op", "hiccl_reduce_auto_choice_op", "hiccl_reduce_plan_set_op", "hiccl_reduce_plan_op",
               "hiccl_host_pipe_set_op")


def _tab(ptrs):
    return (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs)


def hostile(kind, n, count=COUNT, shift=None, seed=None):
    shift = n if shift is None else shift
    seed = n if seed is None else seed
    return H16.hostile(n, count, shift=shift, seed=seed) if kind == "f16" else H32.hostile(kind, n, count, shift, seed)


# ----------------------------------------------------------------------- ABI

def test_new_symbols_exported_and_version():
    assert (SUM, MAX, MIN) == (0, 1, 2) and (hiccl_amd.HICCL_OP_MAX, hiccl_amd.HICCL_OP_MIN) == (1, 2)
    names = L.header_functions()
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in names and hasattr(raw, name) and name in L._SIGS, name
    assert L.lib().hiccl_version() >= 300


def _reduce_op(dtype, op, cfg=None, n=1):
    ins = _tab([0x2000 + 0x1000 * k for k in range(n)])
    return L.lib().hiccl_reduce_op(dtype, op, ctypes.c_void_p(0x1000), ins, n, 4, None,
                                   ctypes.byref(cfg) if cfg is not None else None)


def test_refusals_return_invalid_value_with_a_message():
    """HICCL_BYTES and HICCL_ACC_WIDE take SUM only; an unknown op is refused:
    by the one-shot call, by auto_choice_op and (NULL handles) by the plan and
    pipe entries -- all before any device work."""
    lib = L.lib()
    wide = L.ReduceConfig(acc=L.HICCL_ACC_WIDE)
    for op in (MAX, MIN):
        assert _reduce_op(L.HICCL_BYTES, op) == 1
        assert "HICCL_BYTES" in L.last_error() and "SUM" in L.last_error()
        for dt in (L.HICCL_BFLOAT16, L.HICCL_FLOAT16, L.HICCL_FLOAT32):
            assert _reduce_op(dt, op, wide) == 1
            assert "HICCL_ACC_WIDE" in L.last_error()
        out = [ctypes.c_int() for _ in range(5)]
        refs = [ctypes.byref(v) for v in out]
        assert lib.hiccl_reduce_auto_choice_op(L.HICCL_BYTES, op, None, 1024, 1.0, 256, *refs) == 1
        assert "HICCL_BYTES" in L.last_error()
        assert lib.hiccl_reduce_auto_choice_op(L.HICCL_BFLOAT16, op, ctypes.byref(wide), 1024, 2.0, 256, *refs) == 1
        assert "HICCL_ACC_WIDE" in L.last_error()
    for bad in (-1, 3, 99):
        assert _reduce_op(L.HICCL_FLOAT32, bad) == 1
        assert "unknown op" in L.last_error()
        assert lib.hiccl_reduce_auto_choice_op(L.HICCL_FLOAT32, bad, None, 1024, 2.0, 256, None, None, None, None,
                                               None) == 1
        assert "unknown op" in L.last_error()
    assert _reduce_op(42, MAX) == 1 and "dtype" in L.last_error()
    # the checks hiccl_reduce makes still come first for a valid op
    assert lib.hiccl_reduce_op(L.HICCL_FLOAT32, MAX, ctypes.c_void_p(0), _tab([0x2000]), 1, 4, None, None) == 1
    assert "out is NULL" in L.last_error()
    assert lib.hiccl_reduce_op(L.HICCL_FLOAT32, MIN, ctypes.c_void_p(0), _tab([]), 0, 0, None, None) == 0  # count 0
    # NULL handles
    assert lib.hiccl_reduce_plan_set_op(None, MAX) == 1 and "plan is NULL" in L.last_error()
    assert lib.hiccl_reduce_plan_op(None) == -1
    assert lib.hiccl_host_pipe_set_op(None, MAX) == 1 and "pipe is NULL" in L.last_error()


def test_plan_set_op_on_a_plan():
    """set_op / op on a plan with nothing added: any time, refused for a
    HICCL_BYTES plan and against HICCL_ACC_WIDE in either order.  Creating a
    plan binds a device, so without one this is skipped."""
    lib = L.lib()
    h = ctypes.c_void_p()
    if lib.hiccl_reduce_plan_create(ctypes.byref(h), L.HICCL_BFLOAT16, 0) != 0:
        pytest.skip("no HIP device to bind a plan to: " + L.last_error())
    try:
        assert lib.hiccl_reduce_plan_op(h) == SUM
        assert lib.hiccl_reduce_plan_set_op(h, MAX) == 0 and lib.hiccl_reduce_plan_op(h) == MAX
        assert lib.hiccl_reduce_plan_set_op(h, 7) == 1 and "unknown op" in L.last_error()
        assert lib.hiccl_reduce_plan_op(h) == MAX
        assert lib.hiccl_reduce_plan_set_acc(h, L.HICCL_ACC_WIDE) == 1 and "HICCL_ACC_WIDE" in L.last_error()
        wide = L.ReduceConfig(acc=L.HICCL_ACC_WIDE)
        assert lib.hiccl_reduce_plan_set_config(h, ctypes.byref(wide)) == 1 and "HICCL_ACC_WIDE" in L.last_error()
        assert lib.hiccl_reduce_plan_set_op(h, SUM) == 0
        assert lib.hiccl_reduce_plan_set_acc(h, L.HICCL_ACC_WIDE) == 0
        assert lib.hiccl_reduce_plan_set_op(h, MIN) == 1 and "HICCL_ACC_WIDE" in L.last_error()
        assert lib.hiccl_reduce_plan_op(h) == SUM
    finally:
        lib.hiccl_reduce_plan_destroy(h)
    b = ctypes.c_void_p()
    assert lib.hiccl_reduce_plan_create(ctypes.byref(b), L.HICCL_BYTES, 0) == 0
    try:
        assert lib.hiccl_reduce_plan_set_op(b, MAX) == 1 and "HICCL_BYTES" in L.last_error()
        assert lib.hiccl_reduce_plan_set_op(b, SUM) == 0
    finally:
        lib.hiccl_reduce_plan_destroy(b)


def _rows():
    import auto_table as A
    rows = [(dt, count, n, None) for (dt, count, n), _ in A.RULE_CASES]
    rows += [k for k, _ in A.all_engine_rows()] + [k for k, _ in A.all_store_rows()]
    return rows


def test_auto_choice_op_sum_is_auto_choice_ex():
    """With HICCL_OP_SUM the new entry answers as hiccl_reduce_auto_choice_ex
    does, on every row of tests/auto_table.py."""
    lib = L.lib()
    for dt, count, n, cfg in _rows():
        c = ctypes.byref(L.ReduceConfig(**cfg)) if cfg else None
        a, b = [ctypes.c_int() for _ in range(5)], [ctypes.c_int() for _ in range(5)]
        ra = lib.hiccl_reduce_auto_choice_ex(dt, c, count, float(n), 256, *[ctypes.byref(v) for v in a])
        rb = lib.hiccl_reduce_auto_choice_op(dt, SUM, c, count, float(n), 256, *[ctypes.byref(v) for v in b])
        assert ra == rb == 0 and [v.value for v in a] == [v.value for v in b], (dt, count, n, cfg)
        assert hiccl_amd.auto_choice(dt, count, n, config=cfg, op=SUM) == hiccl_amd.auto_choice(dt, count, n, config=cfg)


def test_auto_choice_op_max_min_pick_only_shapes_the_ops_have():
    """MAX and MIN are untuned: on every row AUTO answers TILE at unroll 4 or
    PHASE at the type's default chunk, nt or write-through stores; a tuned
    shape asked for by name is refused, as hiccl_reduce_op would refuse it."""
    for op in (MAX, MIN):
        seen = set()
        for dt, count, n, cfg in _rows():
            if dt == L.HICCL_BYTES or (cfg and cfg.get("unroll") not in (None, 4)):
                continue
            got = hiccl_amd.auto_choice(dt, count, n, config=cfg, op=op)
            chunk = 8 if dt == L.HICCL_INT32 else 16
            assert (got["engine"], got["unroll"]) in ((T, 4), (P, chunk)), (dt, count, n, cfg, got)
            assert got["store_policy"] in (2, 4)
            seen.add(got["engine"])
        assert seen == {T, P}
        for cfg in (dict(engine=T, unroll=2), dict(engine=T, unroll=8), dict(engine=T, block=512, unroll=4),
                    dict(engine=P, block=1024, unroll=4), dict(nontemporal=1), dict(store_policy=1)):
            with pytest.raises(hiccl_amd.HicclError):
                hiccl_amd.auto_choice(L.HICCL_FLOAT32, 1 << 20, 3, config=cfg, op=op)
        # n > 64: the plan kernel's default shapes
        got = hiccl_amd.auto_choice(L.HICCL_FLOAT32, 1 << 16, 100, op=op)
        assert (got["engine"], got["unroll"]) in ((T, 4), (P, 16))
        # the wide-tile and half-tile rules are SUM's alone
        assert hiccl_amd.auto_choice(L.HICCL_FLOAT32, 1 << 28, 2)["unroll"] == 16
        assert hiccl_amd.auto_choice(L.HICCL_FLOAT32, 1 << 28, 2, op=op)["unroll"] in (4, 16)
        assert hiccl_amd.auto_choice(L.HICCL_FLOAT32, 1 << 28, 2, op=op)["engine"] == P
        assert hiccl_amd.auto_choice(L.HICCL_FLOAT32, 5 << 18, 2.4)["unroll"] == 2
        assert hiccl_amd.auto_choice(L.HICCL_FLOAT32, 5 << 18, 2.4, op=op)["unroll"] == 4


def test_python_layer_refuses_int64_under_max():
    import torch
    with pytest.raises(TypeError, match="unsigned"):
        hiccl_amd.compute._check_op(MAX, torch.int64)
    hiccl_amd.compute._check_op(SUM, torch.int64)
    hiccl_amd.compute._check_op(MIN, torch.uint64)


# ----------------------------------------------- restatement against fixtures

def test_manifest_records_files_and_nan_share():
    with open(os.path.join(GOLDEN, "manifest_ops.json")) as fh:
        m = json.load(fh)
    import hashlib
    for fname, info in m["files"].items():
        path = os.path.join(GOLDEN, fname)
        assert os.path.getsize(path) == info["bytes"] < (1 << 20)
        assert hashlib.sha256(open(path, "rb").read()).hexdigest() == info["sha256"]
        assert 0.0 <= info["nan_share_max"] <= 1.0 / 16
    assert m["files"]["reduce_ops_f32.npz"]["nan_share_max"] > 0  # the one_nan class is there


@pytest.mark.parametrize("kind", list(E.FLOATS))
def test_restatement_gives_the_stored_hostile_outputs(kind):
    """tests/ops_expected.py fold on the stored inputs = the stored outputs
    (the reference's reduce_kernel on maxof / minof), and the stored inputs
    are the hostile generators' as they stand.  At most 1/16 of a case's
    outputs are NaN, all of them in the one_nan class."""
    cases = load_golden(f"reduce_ops_{kind}")
    assert sorted(cases) == sorted(f"hostile_n{n}" for n in NS)
    for n in NS:
        d = cases[f"hostile_n{n}"]
        x = hostile(kind, n)
        assert np.array_equal(E.bits_of(kind, d["in"]), E.bits_of(kind, x))
        one_nan = H32.class_of(COUNT, n) == H32.CLASSES.index("one_nan")
        for name, op in E.OPS.items():
            got = E.fold(kind, op, d["in"])
            assert E.bits_equal(kind, got, d[name]), f"{kind} n={n} {name}: {E.first_mismatch(kind, got, d[name])}"
            nan = E.is_nan(kind, d[name])
            assert np.array_equal(nan, one_nan) and nan.sum() <= 242 and nan.mean() <= 1.0 / 16


def test_restatement_gives_the_stored_integer_outputs():
    cases = load_golden("reduce_ops_int")
    for kind in E.INTS:
        for n in NS:
            d = cases[f"{kind}_n{n}"]
            assert np.array_equal(d["in"], E.int_cases(kind, n, d["in"].shape[1], seed=n))
            for name, op in E.OPS.items():
                got = E.fold(kind, op, d["in"])
                assert got.dtype == d[name].dtype and np.array_equal(got, d[name]), f"{kind} n={n} {name}"
    # the identities and the top bit: the compare is signed for int32, unsigned for uint64
    assert E.fold("i32", E.MAX, np.array([[-1], [1]], np.int32))[0] == 1
    assert E.fold("u64", E.MAX, np.array([[1 << 63], [1]], np.uint64))[0] == 1 << 63
    assert E.fold("i32", E.MAX, np.zeros((0, 2), np.int32)).tolist() == [-(1 << 31)] * 2
    assert E.fold("u64", E.MIN, np.zeros((0, 2), np.uint64)).tolist() == [(1 << 64) - 1] * 2


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_restatement_gives_the_stored_pattern_outputs(kind):
    """Every 16-bit pattern folded with each of 16 addends; the NaN addend's
    rows are all NaN."""
    d = load_golden("reduce_ops_patterns")[kind]
    assert np.array_equal(d["addends"], E.ADDENDS[kind])
    for a, addend in enumerate(d["addends"]):
        x = np.stack([E.ALL_PATTERNS, np.full(1 << 16, addend, np.uint16)])
        for name, op in E.OPS.items():
            exp = E.patterns_expected(kind, addend, d[f"{name}_sel"][a])
            got = E.fold(kind, op, x)
            assert E.bits_equal(kind, got, exp), f"{kind} {name} addend {a}: {E.first_mismatch(kind, got, exp)}"
            assert E.is_nan(kind, exp).all() if a == 15 else E.nan_share(kind, exp) <= 1.0 / 16


def test_restatement_on_the_plain_statements():
    """What the semantics say in so many words, on single elements."""
    f = lambda *v: np.array([[e] for e in v], np.float32)  # noqa: E731
    bits = lambda a: a.view(np.uint32)[0]  # noqa: E731
    assert bits(E.fold("f32", E.MAX, f(-0.0, 0.0))) == 0x00000000 and bits(E.fold("f32", E.MAX, f(0.0, -0.0))) == 0
    assert bits(E.fold("f32", E.MIN, f(-0.0, 0.0))) == 0x80000000 and bits(E.fold("f32", E.MIN, f(0.0, -0.0))) == 0x80000000
    assert bits(E.fold("f32", E.MAX, f(-0.0, -0.0, -0.0))) == 0x80000000  # SUM gives +0 here
    assert np.isnan(E.fold("f32", E.MAX, f(1.0, np.nan, np.inf))[0]) and np.isnan(E.fold("f32", E.MIN, f(np.nan))[0])
    assert bits(E.fold("f32", E.MAX, np.zeros((0, 1), np.float32))) == 0xff800000
    assert bits(E.fold("f32", E.MIN, np.zeros((0, 1), np.float32))) == 0x7f800000
    tiny = np.array([[1], [0x80000001]], np.uint32).view(np.float32)  # +-smallest subnormal
    assert bits(E.fold("f32", E.MAX, tiny)) == 1 and bits(E.fold("f32", E.MIN, tiny)) == 0x80000001
    assert E.fold("bf16", E.MAX, np.zeros((0, 1), np.uint16))[0] == 0xff80
    assert E.fold("f16", E.MIN, np.zeros((0, 1), np.uint16))[0] == 0x7c00
    assert E.fold("f64", E.MAX, np.array([[-np.inf], [-1e308]]))[0] == -1e308


# ----------------------------------------------------------------------- C++

def _check_table(path):
    got = np.fromfile(path, np.uint16).reshape(2, 2, 16, 1 << 16)
    for t, kind in enumerate(("f16", "bf16")):
        for o, (name, op) in enumerate(E.OPS.items()):
            for a, addend in enumerate(E.ADDENDS[kind]):
                x = np.stack([E.ALL_PATTERNS, np.full(1 << 16, addend, np.uint16)])
                # T acc = x; acc += a: the fold of the two from acc, i.e. without the identity step
                exp = E.fold(kind, op, x)
                assert E.bits_equal(kind, got[t, o, a], exp), \
                    f"{name}of<{kind}> += {int(addend):#06x}: {E.first_mismatch(kind, got[t, o, a], exp)}"


def _check_folds(exe, tmp_path, env=None):
    for kind in ("f32", "f64"):
        for n in (0, 1, 3, 9, 17):
            x = hostile(kind, n) if n else np.zeros((0, COUNT), E.carrier(kind))
            _fold_case(exe, tmp_path, kind, x, env)
    for kind in E.INTS:
        for n in (0, 2, 9):
            _fold_case(exe, tmp_path, kind, E.int_cases(kind, n, COUNT, seed=n), env)


def _fold_case(exe, tmp_path, kind, x, env):
    inp, out = tmp_path / "fold_in.bin", tmp_path / "fold_out.bin"
    np.ascontiguousarray(x).tofile(inp)
    for name, op in E.OPS.items():
        p = subprocess.run([str(exe), "fold", kind, name, str(inp), str(out), str(x.shape[0]), str(x.shape[1])],
                           capture_output=True, text=True, env=env)
        assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, \
            p.stdout + p.stderr
        got, exp = np.fromfile(out, E.carrier(kind)), E.fold(kind, op, x, count=x.shape[1])
        assert E.bits_equal(kind, got, exp), f"{name}of<{kind}> n={x.shape[0]}: {E.first_mismatch(kind, got, exp)}"


def test_cpp_ops_add_against_the_restatement(tmp_path):
    """tests/cpp/ops_add.cpp: maxof / minof `+=` of f16 and bf16 on every
    pattern x 16 addends, and the reference's loop on the float, double, int32
    and uint64 wrappers over the hostile classes, give the restatement's words.
    Sizes, dtype_of, op_of and the identities are checked inside the program."""
    make(ROOT, "build/ops_add")
    exe, out = os.path.join(ROOT, "build", "ops_add"), tmp_path / "table.bin"
    p = subprocess.run([exe, "table", str(out)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    _check_table(out)
    _check_folds(exe, tmp_path)


def test_cpp_ops_add_under_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined and run as a
    stand-alone binary: no report, the same words."""
    exe, out = tmp_path / "ops_add_san", tmp_path / "table.bin"
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-Wno-unknown-pragmas", "-DHICCL_PORT_HOST", "-I", os.path.join(ROOT, "include"),
                         "-I", os.environ.get("MPI_INC", "/opt/conda/include"),
                         os.path.join(ROOT, "tests", "cpp", "ops_add.cpp"), "-o", str(exe),
                         os.path.join(os.environ.get("MPI_LIB", "/opt/conda/lib"), "libmpi.so"),
                         "-Wl,-rpath,/usr/lib/x86_64-linux-gnu:" + os.environ.get("MPI_LIB", "/opt/conda/lib")],
                        capture_output=True, text=True)
    if cc.returncode != 0 and ("asan" in cc.stderr or "ubsan" in cc.stderr or "sanitize" in cc.stderr):
        pytest.skip("g++ has no sanitizer runtimes here: " + cc.stderr.strip()[-200:])
    assert cc.returncode == 0, cc.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(exe), "table", str(out)], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr
    _check_table(out)
    _check_folds(exe, tmp_path, env)


def test_cpp_wrappers_refuse_other_integer_types(tmp_path):
    """maxof<int64_t> and minof<uint32_t> fail a static_assert that says why
    (the dtype they would run as compares with the other signedness)."""
    for typ, word in (("int64_t", "UNSIGNED"), ("uint32_t", "SIGNED"), ("int16_t", "4 or 8 bytes")):
        src = tmp_path / f"bad_{typ}.cpp"
        src.write_text(f'#include "hiccl/ops.h"\nHiCCL::maxof<{typ}> x = 0;\nint main() {{ return 0; }}\n')
        cc = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                            capture_output=True, text=True)
        assert cc.returncode != 0 and "static assertion failed" in cc.stderr and word in cc.stderr, cc.stderr
    ok = tmp_path / "ok.cpp"
    ok.write_text('#include "hiccl/ops.h"\nHiCCL::maxof<int> a = 0; HiCCL::minof<unsigned long long> b = 0;\n'
                  'HiCCL::maxof<float> c = 0; HiCCL::minof<HiCCL::bf16> d = 0;\nint main() { return 0; }\n')
    cc = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(ok)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr


def ops_compute_inputs(tmp_path, n=3):
    xf, xb = hostile("f32", n, shift=3, seed=3), hostile("bf16", n, shift=5, seed=5)
    paths = [tmp_path / name for name in ("in_f32.bin", "out_f32.bin", "in_bf16.bin", "out_bf16.bin")]
    xf.tofile(paths[0])
    xb.tofile(paths[2])
    return xf, xb, paths


def check_ops_compute(exe, tmp_path, timeout=None):
    n = 3
    xf, xb, paths = ops_compute_inputs(tmp_path, n)
    cmd = [str(exe)] + [str(p) for p in paths] + [str(n), str(COUNT)]
    if timeout:
        cmd = ["timeout", "-k", "5", str(timeout)] + cmd
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0 and "ops_compute: PASSED" in p.stdout, p.stdout + p.stderr
    gf, gb = np.fromfile(paths[1], np.float32), np.fromfile(paths[3], np.uint16)
    ef, eb = E.fold("f32", E.MAX, xf), E.fold("bf16", E.MIN, xb)
    assert E.nan_share("f32", ef) <= 1.0 / 16 and E.nan_share("bf16", eb) <= 1.0 / 16
    assert E.bits_equal("f32", gf, ef), "maxof<float>: " + E.first_mismatch("f32", gf, ef)
    assert E.bits_equal("bf16", gb, eb), "minof<bf16>: " + E.first_mismatch("bf16", gb, eb)
    return gf, gb


def test_cpp_compute_ops_host_port(tmp_path):
    """Compute<maxof<float>> and Compute<minof<HiCCL::bf16>> on the host port
    (tests/cpp/ops_compute.cpp built with HICCL_PORT_HOST), misaligned inputs
    and output: the restatement's words.  tests/test_ops_gpu.py runs the same
    program's GPU build on the same inputs."""
    make(ROOT, "build/ops_compute_host")
    check_ops_compute(os.path.join(ROOT, "build", "ops_compute_host"), tmp_path)
