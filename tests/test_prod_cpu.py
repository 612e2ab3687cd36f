"""CPU tier of the PROD / BAND / BOR / BXOR operators (hiccl_op_t): the ABI
values and refusals, AUTO's answers, the NumPy restatement
(tests/prod_expected.py) against the stored fixtures and the pattern hashes,
and the C++ wrapper types HiCCL::prodof / bandof / borof / bxorof
(include/hiccl/ops.h) on the host.  No test here needs a GPU or the reference;
the fixtures pin the restatement to the reference's own reduce_kernel
(tests/golden/make_golden_prod.py).
"""
import ctypes
import hashlib
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hiccl_amd
import hostile_prod as HP
import prod_expected as E
from conftest import GOLDEN, ROOT, load_golden, make
from hiccl_amd import _lib as L

COUNT = 17 * 241 + 5
INT_COUNT = 17 * 61 + 5
NS = (1, 2, 3, 8, 9, 17)
NEW_OPS = {"PROD": 16, "BAND": 17, "BOR": 18, "BXOR": 19}
PROD, BAND, BOR, BXOR = 16, 17, 18, 19
BITWISE = (BAND, BOR, BXOR)
FLOAT_DTYPES = (L.HICCL_FLOAT32, L.HICCL_FLOAT64, L.HICCL_BFLOAT16, L.HICCL_FLOAT16)
T, P = L.HICCL_ENGINE_TILE, L.HICCL_ENGINE_PHASE


def _tab(ptrs):
    return (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs)


# ----------------------------------------------------------------------- ABI

def test_op_values_in_the_header_the_bindings_and_the_package():
    header = open(os.path.join(ROOT, "include", "hiccl_reduce.h")).read()
    for name, value in NEW_OPS.items():
        assert re.search(rf"\bHICCL_OP_{name} = {value}\b", header), name
        assert getattr(L, f"HICCL_OP_{name}") == value and getattr(hiccl_amd, f"HICCL_OP_{name}") == value
    assert (L.HICCL_OP_SUM, L.HICCL_OP_MAX, L.HICCL_OP_MIN) == (0, 1, 2)
    assert L.lib().hiccl_version() >= 400


def _reduce_op(dtype, op, cfg=None, n=1):
    ins = _tab([0x2000 + 0x1000 * k for k in range(n)])
    return L.lib().hiccl_reduce_op(dtype, op, ctypes.c_void_p(0x1000), ins, n, 4, None,
                                   ctypes.byref(cfg) if cfg is not None else None)


def _auto_op(dtype, op, cfg=None):
    out = [ctypes.c_int() for _ in range(5)]
    return L.lib().hiccl_reduce_auto_choice_op(dtype, op, ctypes.byref(cfg) if cfg is not None else None, 1024, 2.0, 256,
                                               *[ctypes.byref(v) for v in out])


def test_refusals_return_invalid_value_with_a_message():
    """Bitwise on a floating dtype, any new op with HICCL_BYTES or
    HICCL_ACC_WIDE: refused by the one-shot call and by auto_choice_op, before
    any device work, each with its message."""
    wide = L.ReduceConfig(acc=L.HICCL_ACC_WIDE)
    for op in BITWISE:
        for dt in FLOAT_DTYPES:
            for rc in (_reduce_op(dt, op), _auto_op(dt, op)):
                assert rc == 1
                assert "HICCL_INT32" in L.last_error() and "HICCL_UINT64" in L.last_error(), L.last_error()
        for dt in (L.HICCL_INT32, L.HICCL_UINT64):
            assert _auto_op(dt, op) == 0, L.last_error()
    for op in NEW_OPS.values():
        for rc in (_reduce_op(L.HICCL_BYTES, op), _auto_op(L.HICCL_BYTES, op)):
            assert rc == 1 and "HICCL_BYTES" in L.last_error() and "SUM" in L.last_error()
        for dt in (L.HICCL_BFLOAT16, L.HICCL_FLOAT16, L.HICCL_INT32):
            for rc in (_reduce_op(dt, op, wide), _auto_op(dt, op, wide)):
                assert rc == 1 and "HICCL_ACC_WIDE" in L.last_error()
    # the holes of the enum stay unknown
    for bad in (3, 15, 20):
        assert _reduce_op(L.HICCL_FLOAT32, bad) == 1 and "unknown op" in L.last_error()
    assert _reduce_op(42, PROD) == 1 and "dtype" in L.last_error()
    # the checks hiccl_reduce makes still come first for a valid op; count 0 is a no-op
    lib = L.lib()
    assert lib.hiccl_reduce_op(L.HICCL_FLOAT32, PROD, ctypes.c_void_p(0), _tab([0x2000]), 1, 4, None, None) == 1
    assert "out is NULL" in L.last_error()
    assert lib.hiccl_reduce_op(L.HICCL_INT32, BXOR, ctypes.c_void_p(0), _tab([]), 0, 0, None, None) == 0
    assert lib.hiccl_reduce_plan_set_op(None, PROD) == 1 and "plan is NULL" in L.last_error()
    assert lib.hiccl_host_pipe_set_op(None, BAND) == 1 and "pipe is NULL" in L.last_error()


def test_plan_set_op_refusals_on_a_plan():
    """A plan takes the new operators and honours the refusals.  Creating a
    plan binds a device, so without one this is skipped."""
    lib = L.lib()
    h = ctypes.c_void_p()
    if lib.hiccl_reduce_plan_create(ctypes.byref(h), L.HICCL_BFLOAT16, 0) != 0:
        pytest.skip("no HIP device to bind a plan to: " + L.last_error())
    try:
        assert lib.hiccl_reduce_plan_set_op(h, PROD) == 0 and lib.hiccl_reduce_plan_op(h) == PROD
        for op in BITWISE:
            assert lib.hiccl_reduce_plan_set_op(h, op) == 1 and "HICCL_INT32" in L.last_error()
        assert lib.hiccl_reduce_plan_op(h) == PROD
        assert lib.hiccl_reduce_plan_set_acc(h, L.HICCL_ACC_WIDE) == 1 and "HICCL_ACC_WIDE" in L.last_error()
        assert lib.hiccl_reduce_plan_set_op(h, L.HICCL_OP_SUM) == 0
        assert lib.hiccl_reduce_plan_set_acc(h, L.HICCL_ACC_WIDE) == 0
        assert lib.hiccl_reduce_plan_set_op(h, PROD) == 1 and "HICCL_ACC_WIDE" in L.last_error()
    finally:
        lib.hiccl_reduce_plan_destroy(h)
    for dt, ops in ((L.HICCL_BYTES, ()), (L.HICCL_INT32, NEW_OPS.values()), (L.HICCL_UINT64, NEW_OPS.values())):
        b = ctypes.c_void_p()
        assert lib.hiccl_reduce_plan_create(ctypes.byref(b), dt, 0) == 0
        try:
            for op in NEW_OPS.values():
                if op in ops:
                    assert lib.hiccl_reduce_plan_set_op(b, op) == 0 and lib.hiccl_reduce_plan_op(b) == op
                else:
                    assert lib.hiccl_reduce_plan_set_op(b, op) == 1 and "HICCL_BYTES" in L.last_error()
        finally:
            lib.hiccl_reduce_plan_destroy(b)


def _rows():
    import auto_table as A
    rows = [(dt, count, n, None) for (dt, count, n), _ in A.RULE_CASES]
    rows += [k for k, _ in A.all_engine_rows()] + [k for k, _ in A.all_store_rows()]
    return rows


def test_auto_choice_op_picks_only_shapes_the_untuned_ops_have():
    """The new operators are untuned: on every row of tests/auto_table.py AUTO
    answers TILE at unroll 4 or PHASE at the type's default chunk, nt or
    write-through stores, without a device; a tuned shape asked for by name is
    refused."""
    for op in NEW_OPS.values():
        seen = set()
        for dt, count, n, cfg in _rows():
            if dt == L.HICCL_BYTES or (cfg and cfg.get("unroll") not in (None, 4)):
                continue
            if op in BITWISE and dt not in (L.HICCL_INT32, L.HICCL_UINT64):
                with pytest.raises(hiccl_amd.HicclError):
                    hiccl_amd.auto_choice(dt, count, n, config=cfg, op=op)
                dt = L.HICCL_INT32 if hiccl_amd.lib().hiccl_dtype_size(dt) <= 4 else L.HICCL_UINT64
                if cfg and cfg.get("acc"):
                    continue
            got = hiccl_amd.auto_choice(dt, count, n, config=cfg, op=op)
            chunk = 8 if dt == L.HICCL_INT32 else 16
            assert (got["engine"], got["unroll"]) in ((T, 4), (P, chunk)), (op, dt, count, n, cfg, got)
            assert got["store_policy"] in (2, 4)
            seen.add(got["engine"])
        assert seen == {T, P}
        dt = L.HICCL_FLOAT32 if op == PROD else L.HICCL_INT32
        for cfg in (dict(engine=T, unroll=2), dict(engine=T, unroll=8), dict(engine=T, block=512, unroll=4),
                    dict(engine=P, block=1024, unroll=4), dict(nontemporal=1), dict(store_policy=1)):
            with pytest.raises(hiccl_amd.HicclError):
                hiccl_amd.auto_choice(dt, 1 << 20, 3, config=cfg, op=op)
        got = hiccl_amd.auto_choice(dt, 1 << 16, 100, op=op)  # n > 64: the plan kernel's default shapes
        assert (got["engine"], got["unroll"]) in ((T, 4), (P, 8 if dt == L.HICCL_INT32 else 16))
    # the wide-tile and half-tile rules stay SUM's alone
    assert hiccl_amd.auto_choice(L.HICCL_FLOAT32, 1 << 28, 2)["unroll"] == 16
    assert hiccl_amd.auto_choice(L.HICCL_FLOAT32, 1 << 28, 2, op=PROD)["engine"] == P
    assert hiccl_amd.auto_choice(L.HICCL_FLOAT32, 5 << 18, 2.4)["unroll"] == 2
    assert hiccl_amd.auto_choice(L.HICCL_FLOAT32, 5 << 18, 2.4, op=PROD)["unroll"] == 4


def test_python_layer_checks_the_op_before_any_device_work():
    import torch
    check = hiccl_amd.compute._check_op
    for op in NEW_OPS.values():
        check(op, torch.int64)  # the same bits for either signedness
        check(op, torch.int32)
    with pytest.raises(TypeError, match="unsigned"):
        check(L.HICCL_OP_MAX, torch.int64)
    for op in BITWISE:
        for dt in (torch.float32, torch.float64, torch.bfloat16, torch.float16):
            with pytest.raises(TypeError, match="integer"):
                check(op, dt)
    check(PROD, torch.bfloat16)


# ----------------------------------------------- restatement against fixtures

def _manifest():
    with open(os.path.join(GOLDEN, "manifest_prod.json")) as fh:
        return json.load(fh)


def test_manifest_records_files_and_nan_share():
    m = _manifest()
    for fname, info in m["files"].items():
        path = os.path.join(GOLDEN, fname)
        assert os.path.getsize(path) == info["bytes"] < (1 << 20)
        assert hashlib.sha256(open(path, "rb").read()).hexdigest() == info["sha256"]
        assert 0.0 <= info["nan_share_max"] <= 1.0 / 8
    assert m["files"]["reduce_prod_f32.npz"]["nan_share_max"] > 0  # the NaN classes are there
    assert set(m["patterns"]) == {"f16", "bf16"}


@pytest.mark.parametrize("kind", list(E.FLOATS))
def test_restatement_gives_the_stored_hostile_outputs(kind):
    """prod_expected.fold on the stored inputs = the stored outputs (the
    reference's reduce_kernel on prodof), and the stored inputs are the
    generator's as it stands.  Only one_nan and inf_times_zero yield NaN, at
    most 1/8 of a case; every near_one output is finite, normal and nonzero."""
    cases = load_golden(f"reduce_prod_{kind}")
    assert sorted(cases) == sorted(f"hostile_n{n}" for n in NS)
    K = HP.KINDS[kind]
    for n in NS:
        d = cases[f"hostile_n{n}"]
        x = HP.hostile(kind, n, COUNT, shift=n, seed=n)
        assert np.array_equal(E.bits_of(kind, d["in"]), E.bits_of(kind, x))
        got = E.fold(kind, E.PROD, d["in"])
        assert E.bits_equal(kind, got, d["prod"]), f"{kind} n={n}: {E.first_mismatch(kind, got, d['prod'])}"
        cls = HP.class_of(COUNT, n)
        nan = E.is_nan(kind, d["prod"])
        allowed = np.isin(cls, [HP.CLASSES.index(c) for c in HP.NAN_CLASSES])
        assert not nan[~allowed].any() and nan.mean() <= 1.0 / 8
        assert nan[cls == HP.CLASSES.index("one_nan")].all()
        u = E.bits_of(kind, d["prod"][cls == 0]).astype(np.uint64)
        top = (1 << (K["bits"] - 1 - K["mant"])) - 1
        e = (u >> np.uint64(K["mant"])) & np.uint64(top)
        assert ((e != 0) & (e != top)).all(), "a near_one output that is not finite, normal and nonzero"


def test_restatement_gives_the_stored_integer_outputs():
    cases = load_golden("reduce_prod_int")
    for kind in E.INTS:
        for n in NS:
            d = cases[f"{kind}_n{n}"]
            assert d["in"].shape == (n, INT_COUNT)
            assert np.array_equal(d["in"], E.int_cases(kind, n, INT_COUNT, seed=n))
            for name, op in E.OPS.items():
                got = E.fold(kind, op, d["in"])
                assert got.dtype == d[name].dtype and np.array_equal(got, d[name]), f"{kind} n={n} {name}"
    # the plain statements: wrap-around, identities
    assert E.fold("i32", E.PROD, np.array([[-(1 << 31)], [-1]], np.int32))[0] == -(1 << 31)
    assert E.fold("i32", E.PROD, np.array([[65536], [65536]], np.int32))[0] == 0
    assert E.fold("u64", E.PROD, np.array([[(1 << 64) - 1], [(1 << 64) - 1]], np.uint64))[0] == 1
    assert E.fold("i32", E.PROD, np.zeros((0, 2), np.int32)).tolist() == [1, 1]
    assert E.fold("i32", E.BAND, np.zeros((0, 2), np.int32)).tolist() == [-1, -1]
    assert E.fold("u64", E.BAND, np.zeros((0, 1), np.uint64)).tolist() == [(1 << 64) - 1]
    assert E.fold("u64", E.BOR, np.zeros((0, 1), np.uint64)).tolist() == [0]
    assert E.fold("u64", E.BXOR, np.array([[5], [5], [9]], np.uint64))[0] == 9


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_restatement_gives_the_stored_pattern_hash(kind):
    """Every 16-bit pattern times each of 16 multipliers: the restatement's
    words hash to what the reference's did; the NaN multiplier's row is all
    NaN."""
    words = E.patterns_expected(kind)
    assert E.patterns_hash(kind, words) == _manifest()["patterns"][kind]["sha256"]
    assert E.is_nan(kind, words[15]).all() and E.nan_share(kind, words[:15]) <= 1.0 / 8


def test_restatement_on_the_plain_statements():
    f = lambda *v: np.array([[e] for e in v], np.float32)  # noqa: E731
    bits = lambda a: a.view(np.uint32)[0]  # noqa: E731
    assert bits(E.fold("f32", E.PROD, np.zeros((0, 1), np.float32))) == 0x3f800000
    assert bits(E.fold("f32", E.PROD, f(-0.0))) == 0x80000000  # 1 x -0 = -0
    assert bits(E.fold("f32", E.PROD, f(-0.0, -2.0))) == 0
    assert np.isnan(E.fold("f32", E.PROD, f(np.inf, 0.0))[0]) and np.isnan(E.fold("f32", E.PROD, f(2.0, np.nan))[0])
    tiny = np.array([[1], [0x40000000]], np.uint32).view(np.float32)  # the smallest subnormal times 2
    assert bits(E.fold("f32", E.PROD, tiny)) == 2
    assert E.fold("bf16", E.PROD, np.zeros((0, 1), np.uint16))[0] == 0x3f80
    assert E.fold("f16", E.PROD, np.zeros((0, 1), np.uint16))[0] == 0x3c00
    # bf16 rounds after the f32 multiply: (1 + 2^-7) x 1.5 = 1.5 + 1.5 x 2^-7 is a tie, to even
    assert E.fold("bf16", E.PROD, np.array([[0x3f81], [0x3fc0]], np.uint16))[0] == 0x3fc2
    # and after EVERY multiply: 2^-126 x 2^-9 rounds to zero, which 2^9 does not bring back
    assert E.fold("bf16", E.PROD, np.array([[0x0080], [0x3b00], [0x4400]], np.uint16))[0] == 0


# ----------------------------------------------------------------------- C++

def test_cpp_prod_add_plain_and_under_sanitizers(tmp_path):
    """tests/cpp/prod_add.cpp, a stand-alone program: prodof<bf16> / prodof<f16>
    `+=` on every pattern x 16 multipliers against the exact product in double
    rounded once, the integer wrappers at the wrap-around extremes, the three
    bitwise wrappers.  Built plainly and with -fsanitize=address,undefined;
    both binaries are run."""
    make(ROOT, "build/prod_add")
    p = subprocess.run([os.path.join(ROOT, "build", "prod_add")], capture_output=True, text=True)
    assert p.returncode == 0 and "prod_add: PASSED" in p.stdout, p.stdout + p.stderr
    exe = tmp_path / "prod_add_san"
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "prod_add.cpp"),
                         "-o", str(exe)], capture_output=True, text=True)
    if cc.returncode != 0 and ("asan" in cc.stderr or "ubsan" in cc.stderr or "sanitize" in cc.stderr):
        pytest.skip("g++ has no sanitizer runtimes here: " + cc.stderr.strip()[-200:])
    assert cc.returncode == 0, cc.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "prod_add: PASSED" in p.stdout, p.stdout + p.stderr
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr


def test_cpp_wrappers_static_asserts(tmp_path):
    """prodof takes the six types and any signedness of 4- and 8-byte
    integers; the bitwise wrappers take 4- and 8-byte integers only."""
    inc = os.path.join(ROOT, "include")
    ok = tmp_path / "ok.cpp"
    ok.write_text('#include "hiccl/ops.h"\nusing namespace HiCCL;\n'
                  "prodof<float> a = 0; prodof<double> b = 0; prodof<bf16> c = 0; prodof<f16> d = 0;\n"
                  "prodof<int32_t> e = 0; prodof<uint32_t> f = 0; prodof<int64_t> g = 0; prodof<uint64_t> h = 0;\n"
                  "bandof<int32_t> i = 0; borof<uint32_t> j = 0; bxorof<int64_t> k = 0; bxorof<uint64_t> l = 0;\n"
                  "int main() { return 0; }\n")
    cc = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", inc, str(ok)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    for decl in ("prodof<int16_t>", "bandof<float>", "bxorof<HiCCL::bf16>", "borof<int16_t>", "bandof<double>"):
        src = tmp_path / "bad.cpp"
        src.write_text(f'#include "hiccl/ops.h"\nusing namespace HiCCL;\n{decl} x = 0;\nint main() {{ return 0; }}\n')
        cc = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", inc, str(src)], capture_output=True, text=True)
        assert cc.returncode != 0 and "static assertion failed" in cc.stderr and "4 or 8 bytes" in cc.stderr, decl + cc.stderr


def prod_compute_case(n=3):
    """The inputs and stored outputs tests/cpp/prod_compute.cpp runs on: the
    fixtures' hostile_n<n> cases of f32 and bf16."""
    df, db = load_golden("reduce_prod_f32")[f"hostile_n{n}"], load_golden("reduce_prod_bf16")[f"hostile_n{n}"]
    return df, db


def check_prod_compute(exe, tmp_path, timeout=None, n=3):
    df, db = prod_compute_case(n)
    paths = [tmp_path / name for name in ("in_f32.bin", "out_f32.bin", "in_bf16.bin", "out_bf16.bin")]
    np.ascontiguousarray(df["in"]).tofile(paths[0])
    np.ascontiguousarray(db["in"]).tofile(paths[2])
    cmd = [str(exe)] + [str(p) for p in paths] + [str(n), str(COUNT)]
    if timeout:
        cmd = ["timeout", "-k", "5", str(timeout)] + cmd
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0 and "prod_compute: PASSED" in p.stdout, p.stdout + p.stderr
    gf, gb = np.fromfile(paths[1], np.float32), np.fromfile(paths[3], np.uint16)
    assert E.bits_equal("f32", gf, df["prod"]), "prodof<float>: " + E.first_mismatch("f32", gf, df["prod"])
    assert E.bits_equal("bf16", gb, db["prod"]), "prodof<bf16>: " + E.first_mismatch("bf16", gb, db["prod"])


def test_cpp_compute_prod_host_port(tmp_path):
    """Compute<prodof<float>> and Compute<prodof<HiCCL::bf16>> on the host port
    (tests/cpp/prod_compute.cpp built with HICCL_PORT_HOST), misaligned inputs
    and output, against the fixtures.  tests/test_prod_gpu.py runs the same
    program's GPU build on the same inputs."""
    make(ROOT, "build/prod_compute_host")
    check_prod_compute(os.path.join(ROOT, "build", "prod_compute_host"), tmp_path)


def run_prod_comm(exe, env=None, timeout=None, count=4099):
    mpirun = shutil.which("mpirun") or "/opt/conda/bin/mpirun"
    if not os.path.exists(mpirun):
        pytest.skip("no mpirun")
    cmd = [mpirun, "-np", "2", str(exe), str(count)]
    if timeout:
        cmd = ["timeout", "-k", "10", str(timeout)] + cmd
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd="/tmp")
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-3000:]
    assert "prodof<float> reduce to root: PASSED" in out and "bxorof<uint64_t> reduce to root: PASSED" in out, out[-3000:]


def test_cpp_comm_prod_host_port():
    """Comm<prodof<float>> and Comm<bxorof<uint64_t>> reduce to root under MPI
    with 2 ranks on the host port; the contributions' product is exact in any
    order."""
    make(ROOT, "build/prod_comm_host")
    run_prod_comm(os.path.join(ROOT, "build", "prod_comm_host"))
