"""CPU tier of the fp16 element type (HICCL_FLOAT16): the ABI's host side,
AUTO's rules (bf16's, unchanged), the hostile inputs and the NumPy
restatement the GPU tier expects (tests/hostile_f16.py), the fixture, and
HiCCL::f16's arithmetic on every bit pattern.  No GPU.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import auto_table as A
import hostile_f16 as H
from conftest import ROOT, load_golden, make
from hiccl_amd import _lib as L

F16, BF16 = L.HICCL_FLOAT16, L.HICCL_BFLOAT16
NS = [1, 2, 3, 8, 9, 17]
COUNT = 17 * 241 + 5


# ------------------------------------------------------------------- the ABI

def test_dtype_size_and_version():
    lib = L.lib()
    assert F16 == 6 and L.DTYPE_OF_TORCH[torch.float16] == 6
    assert lib.hiccl_dtype_size(6) == 2
    assert [lib.hiccl_dtype_size(d) for d in range(6)] == [4, 8, 2, 8, 4, 1]
    assert lib.hiccl_dtype_size(7) == 0
    assert lib.hiccl_version() > 100  # 0.1.0 had no HICCL_FLOAT16
    header = open(L.HEADER_PATH).read()
    assert "HICCL_FLOAT16 = 6" in header and "HICCL_NUM_DTYPES = 7" in header


def _tab(ptrs):
    return (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs)


def test_host_argument_checks():
    lib = L.lib()
    assert "hiccl_reduce_f16" in L.header_functions() and "hiccl_reduce_f16" in L._SIGS
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "hiccl_reduce_f16")
    # an output one byte off a half boundary, through either entry
    assert lib.hiccl_reduce(F16, ctypes.c_void_p(0x1001), _tab([0x2000]), 1, 4, None) == 1
    assert "element-aligned" in L.last_error()
    assert lib.hiccl_reduce_f16(ctypes.c_void_p(0x1001), _tab([0x2000]), 1, 4, None) == 1
    assert "element-aligned" in L.last_error()
    # a misaligned input, a partial overlap; count 0 is a no-op
    assert lib.hiccl_reduce_f16(ctypes.c_void_p(0x1000), _tab([0x2001]), 1, 4, None) == 1
    assert lib.hiccl_reduce_f16(ctypes.c_void_p(0x1000), _tab([0x1002]), 1, 4, None) == 1
    assert "overlaps" in L.last_error()
    assert lib.hiccl_reduce_f16(ctypes.c_void_p(0), _tab([]), 0, 0, None) == 0
    # fill_uniform names the type it now takes
    assert lib.hiccl_fill_uniform(L.HICCL_INT32, ctypes.c_void_p(0x1000), 4, 1, 0, 0, None) == 1
    assert "FLOAT16" in L.last_error() and "BFLOAT16" in L.last_error()
    assert lib.hiccl_bucket_stride(F16, 1 << 20) == lib.hiccl_bucket_stride(BF16, 1 << 20) == (2 << 20) + (64 << 10)


# ---------------------------------------------------------- AUTO: bf16's rules

def _choice(dtype, cfg, count, n, cus=256):
    out = [ctypes.c_int(-1) for _ in range(5)]
    c = L.ReduceConfig(**cfg)
    rc = L.lib().hiccl_reduce_auto_choice_ex(dtype, ctypes.byref(c), count, float(n), cus, *[ctypes.byref(v) for v in out])
    return (rc,) + tuple(v.value for v in out)  # rc, engine, unroll, blocks per CU, dynamic, store form


def _auto_rows():
    """Every bf16 row of tests/auto_table.py as it stands, and every f32 row
    at its own element count (half the bytes) and at twice it (the same
    bytes); each with the row's config."""
    rows = [(k, None) for k, _ in A.RULE_CASES] + [(k[:3], k[3]) for k, _ in A.all_engine_rows() + A.all_store_rows()]
    out = []
    for (dt, count, n), cfg in rows:
        if dt == A.BF16:
            out.append((count, n, cfg))
        elif dt == A.F32:
            out += [(count, n, cfg), (2 * count, n, cfg)]
    assert sum(dt == A.BF16 for (dt, _, _), _ in rows) >= 8 and len(out) >= 60
    return out


@pytest.mark.parametrize("acc", [L.HICCL_ACC_NATIVE, L.HICCL_ACC_WIDE], ids=["native", "wide"])
def test_auto_takes_bf16s_rules(acc):
    """hiccl_reduce_auto_choice(_ex) answers for HICCL_FLOAT16 exactly what it
    answers for HICCL_BFLOAT16: engine, unroll, workgroups per CU, schedule
    and store form (or the same refusal), on 256 and on 64 CUs."""
    engines = set()
    for count, n, cfg in _auto_rows():
        for cus in (256, 64):
            c = dict(cfg or {}, acc=acc)
            got, want = _choice(F16, c, count, n, cus), _choice(BF16, c, count, n, cus)
            assert got == want, f"count={count} n={n} cfg={c} cus={cus}: f16 {got}, bf16 {want}"
            if cfg is None and got[0] == 0:
                plain = [ctypes.c_int(-1) for _ in range(4)]
                assert L.lib().hiccl_reduce_auto_choice(F16, acc, count, float(n), cus,
                                                        *[ctypes.byref(v) for v in plain]) == 0
                assert tuple(v.value for v in plain) == got[1:5]
            engines.add(got[1:3])
    P = 16 if acc == L.HICCL_ACC_NATIVE else 8  # phase_p follows the accumulator's width
    assert (L.HICCL_ENGINE_PHASE, P) in engines and (L.HICCL_ENGINE_TILE, 4) in engines
    if acc == L.HICCL_ACC_NATIVE:  # the headline type's shapes: wide tiles, half tiles
        assert {(L.HICCL_ENGINE_TILE, u) for u in (2, 8, 16)} <= engines


def test_tuned_shapes_exist_for_native_only():
    """The native op has bf16's full table (TILE 256 x 1..16, 512 x 1..4);
    the f32 accumulator runs the default shapes only."""
    for block, unroll, native, wide in ((256, 1, 0, 1), (256, 16, 0, 1), (512, 2, 0, 1), (256, 4, 0, 0), (128, 4, 1, 1)):
        for acc, want in ((L.HICCL_ACC_NATIVE, native), (L.HICCL_ACC_WIDE, wide)):
            cfg = dict(engine=L.HICCL_ENGINE_TILE, block=block, unroll=unroll, acc=acc)
            assert _choice(F16, cfg, 1 << 20, 3)[0] == want == _choice(BF16, cfg, 1 << 20, 3)[0], cfg


# ------------------------------------------------------- hostile_f16 self-test

def f(bits):
    return H.to_f32(bits)


def test_hostile_classes_are_what_they_say():
    n, count = 9, 17 * 40
    x = H.hostile(n, count, shift=0, seed=3)
    assert x.dtype == np.uint16 and x.shape == (n, count) and not x.flags.writeable
    cls = H.class_of(count)
    col = lambda name: x[:, cls == H.CLASSES.index(name)]  # noqa: E731
    exp = H.native_sum(x)
    ecol = lambda name: exp[cls == H.CLASSES.index(name)]  # noqa: E731
    assert (col("neg_zeros") == 0x8000).all() and (ecol("neg_zeros") == 0).all()
    assert (col("pos_then_neg_zero")[0] == 0).all() and (col("pos_then_neg_zero")[1:] == 0x8000).all()
    assert (H.is_nan(col("one_nan")).sum(axis=0) == 1).all() and H.is_nan(ecol("one_nan")).all()
    c = col("inf_minus_inf")
    assert ((c == 0x7C00).sum(axis=0) == 1).all() and ((c == 0xFC00).sum(axis=0) == 1).all()
    assert H.is_nan(ecol("inf_minus_inf")).all()
    assert (ecol("pos_inf") == 0x7C00).all() and (ecol("neg_inf") == 0xFC00).all()
    c = col("subnormals")
    assert ((c & 0x7FFF) <= 7).all() and (c & 0x7FFF).max() == 7          # -7..7 units of 2^-24
    assert ((ecol("subnormals") & 0x7C00) == 0).all()                     # a subnormal (or zero) sum
    assert np.array_equal(f(ecol("subnormals")), f(c).astype(np.float64).sum(axis=0).astype(np.float32))  # exact
    c = col("into_subnormal")
    assert ((c == 0x0400).sum(axis=0) == 1).all() and ((c == 0x8003).sum(axis=0) == 1).all()
    assert (ecol("into_subnormal") == 0x03FD).all()                       # 2^-14 - 3 units
    assert ((col("max_alone") == 0x7BFF).sum(axis=0) == 1).all() and (ecol("max_alone") == 0x7BFF).all()
    assert (col("max_max_negmax")[:3].T == [0x7BFF, 0x7BFF, 0xFBFF]).all() and (ecol("max_max_negmax") == 0x7C00).all()
    c = col("big_cancel")
    assert ((c == 0x7400).sum(axis=0) == 1).all() and ((c == 0xF400).sum(axis=0) == 1).all()  # +-2^14
    assert ((c == 0x3C00).sum(axis=0) == n - 2).all()
    assert len(set(ecol("big_cancel").tolist())) > 1                      # the order decides: several sums
    assert np.float16(16384.0) + np.float16(1.0) == np.float16(16384.0)   # 2^14 + 1 is not a half
    assert (col("ties_to_even")[0] == 0x6800).all() and (ecol("ties_to_even") == 0x6800).all()  # 2^11 + 1s: stays
    assert (f(col("ties_round_up")[0]) == 2050.0).all()
    assert (f(ecol("ties_round_up")) == 2052.0).all()                     # the first tie rounds up, the later ones down
    c = col("max_plus_half_ulp")
    assert (c[0] == 0x7BFF).all() and (f(c[1]) == 16.0).all() and (ecol("max_plus_half_ulp") == 0x7C00).all()
    w = f(col("wide_random"))
    assert np.isfinite(w).all() and np.abs(w).max() < 2.0 ** 13 and np.abs(w).min() >= 2.0 ** -12
    assert np.abs(w).max() > 2.0 ** 9 and np.abs(w).min() < 2.0 ** -9
    u = f(col("uniform"))
    assert (u >= -1).all() and (u < 1).all() and len(np.unique(u)) > u.size // 2
    c = col("exact_cancel")
    assert ((c == 0x3C00).sum(axis=0) == 1).all() and ((c == 0xBC00).sum(axis=0) == 1).all()
    assert (ecol("exact_cancel") == 0).all()
    # the wide restatement differs where the f32 accumulator does not round: ties and the cancel
    wide = H.wide_sum(x)
    assert (f(wide[cls == H.CLASSES.index("ties_to_even")]) == 2048.0 + 8).all()
    assert (f(wide[cls == H.CLASSES.index("big_cancel")]) == 7.0).all()


@pytest.mark.parametrize("n", NS)
def test_hostile_nan_cap_and_output_shares(n):
    x = H.hostile(n, COUNT, shift=n, seed=n)
    for wide in (False, True):
        exp = H.expected(x, wide)
        H.assert_nan_cap(exp)
        s = H.shares(exp)
        assert s["nan"] <= 2 / 17 + 1e-3, s  # only one_nan and inf_minus_inf yield NaN
        assert s["inf"] > 0 and s["zero"] > 0 and s["sub"] > 0, s
    for near in (False, True):
        t = H.tamed_bits(n, COUNT, seed=n, near=near)
        for wide in (False, True):
            s = H.shares(H.expected(t, wide))
            assert s["nan"] <= 0.08, (n, near, wide, s)  # untamed: 0.25-0.42 at n >= 9
    assert (((H.tamed_bits(n, COUNT, seed=n)[:, 1:8] >> 10) & 0x1F) < 29).all()
    assert (((H.tamed_bits(17, COUNT, seed=1)[:, ::8] >> 10) & 0x1F) == 31).any()  # every eighth column is left raw


def test_tamed_outputs_keep_inf_and_subnormals():
    s = H.shares(np.concatenate([H.native_sum(H.tamed_bits(n, COUNT, seed=n, near=near)) for n in NS for near in (0, 1)]))
    assert s["inf"] > 0 and s["sub"] > 0, s


def test_hostile_is_deterministic_and_shift_moves_classes():
    a, b = H.hostile(9, 500, shift=3, seed=5), H.hostile(9, 500, shift=3, seed=5)
    assert a is b  # cached
    H._hostile.cache_clear()
    c = H.hostile(9, 500, shift=3, seed=5)
    assert c is not a and np.array_equal(a, c)
    assert not np.array_equal(a, H.hostile(9, 500, shift=3, seed=6))
    assert np.array_equal(H.class_of(500, 3), (np.arange(500) + 3) % 17)
    zeros = lambda x: np.nonzero((x == 0x8000).all(axis=0))[0]  # noqa: E731  (the neg_zeros columns)
    assert zeros(H.hostile(9, 500, shift=0, seed=5))[0] == 0 and zeros(H.hostile(9, 500, shift=3, seed=5))[0] == 14
    assert np.array_equal(H.hostile(9, 500, shift=20, seed=5), a)  # shift is taken modulo 17
    assert np.array_equal(H.tamed_bits(9, 500, seed=2), H.tamed_bits(9, 500, seed=2))
    assert H.hostile(0, 5).shape == (0, 5) and (H.native_sum(H.hostile(0, 5), count=5) == 0).all()


def test_bits_equal_takes_nan_by_nan_ness_only():
    a = np.array([0x7E00, 0x3C00, 0x8000, 0x7C00], np.uint16)
    assert H.bits_equal(a, np.array([0xFE01, 0x3C00, 0x8000, 0x7C00], np.uint16))
    assert not H.bits_equal(a, np.array([0x7E00, 0x3C00, 0x0000, 0x7C00], np.uint16))  # -0 is not +0
    assert not H.bits_equal(a, np.array([0x7E00, 0x3C00, 0x8000, 0x7C01], np.uint16))  # Inf is not NaN
    assert "first at 2" in H.first_mismatch(a, np.array([0x7E00, 0x3C00, 0x0000, 0x7C00], np.uint16))


# ---------------------------------------------------------------- the fixture

def test_numpy_restatement_equals_the_fixture():
    """Every expected array of reduce_f16.npz (the reference's reduce_kernel
    instantiated for _Float16) is NumPy's in-order float16 sum, and the
    stored inputs are what tests/hostile_f16.py builds today."""
    cases = load_golden("reduce_f16")
    assert sorted(cases) == sorted([f"hostile_n{n}" for n in NS] + ["every_pattern"] +
                                   [f"tamed_n{n}{s}" for n in (2, 9, 17) for s in ("", "_near")])
    for name, c in cases.items():
        assert c["in"].dtype == np.uint16 and c["out"].dtype == np.uint16
        H.assert_nan_cap(c["out"])
        got = H.native_sum(c["in"])
        assert H.bits_equal(got, c["out"]), f"{name}: {H.first_mismatch(got, c['out'])}"
    for n in NS:
        assert np.array_equal(cases[f"hostile_n{n}"]["in"], H.hostile(n, COUNT, shift=n, seed=n))
    for n in (2, 9, 17):
        assert np.array_equal(cases[f"tamed_n{n}_near"]["in"], H.tamed_bits(n, COUNT, seed=n, near=True))
    assert np.array_equal(cases["every_pattern"]["in"][0], np.arange(1 << 16))
    for fname in ("reduce_f16.npz", "reduce_f16.part2.npz", "manifest_f16.json"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", fname)) < (1 << 20)


def test_fixture_manifest_hashes():
    import hashlib
    import json
    with open(os.path.join(ROOT, "tests", "golden", "manifest_f16.json")) as fh:
        man = json.load(fh)
    assert man["generator"] == "tests/golden/make_golden_f16.py" and set(man["files"]) == {"reduce_f16.npz",
                                                                                          "reduce_f16.part2.npz"}
    for fname, meta in man["files"].items():
        with open(os.path.join(ROOT, "tests", "golden", fname), "rb") as fh:
            assert hashlib.sha256(fh.read()).hexdigest() == meta["sha256"], fname


# ------------------------------------------------------------------ HiCCL::f16

def _expected_adds():
    allp = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    with np.errstate(all="ignore"):
        return np.stack([(allp.view(np.float16) + np.full(1 << 16, a, np.uint16).view(np.float16))
                         .astype(np.float16).view(np.uint16) for a in H.ADDENDS])


def _check_adds(path):
    got = np.fromfile(path, np.uint16).reshape(16, 1 << 16)
    exp = _expected_adds()
    assert 0.02 < H.shares(exp)["nan"] < 0.12  # the NaN patterns, the NaN addend, Inf - Inf
    for a in range(16):
        assert H.bits_equal(got[a], exp[a]), f"x += {int(H.ADDENDS[a]):#06x}: {H.first_mismatch(got[a], exp[a])}"


def test_cpp_f16_add_every_pattern(tmp_path):
    """tests/cpp/f16_add.cpp: `acc += a` of HiCCL::f16 for all 65,536 patterns
    and 16 addends gives NumPy's half add bit for bit (a NaN by NaN-ness);
    float -> f16 -> float round trips and `T acc = 0` are checked inside."""
    make(ROOT, "build/f16_add")
    out = tmp_path / "adds.bin"
    p = subprocess.run([os.path.join(ROOT, "build", "f16_add"), str(out)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    _check_adds(out)


def test_cpp_f16_add_under_sanitizers(tmp_path):
    """The same program built with -fsanitize=undefined,address and run as a
    stand-alone binary: no report, the same bits."""
    exe, out = tmp_path / "f16_add_san", tmp_path / "adds.bin"
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all",
                         "-Wno-unknown-pragmas", "-DHICCL_PORT_HOST", "-I", os.path.join(ROOT, "include"),
                         "-I", os.environ.get("MPI_INC", "/opt/conda/include"),
                         os.path.join(ROOT, "tests", "cpp", "f16_add.cpp"), "-o", str(exe),
                         os.path.join(os.environ.get("MPI_LIB", "/opt/conda/lib"), "libmpi.so"),
                         "-Wl,-rpath,/usr/lib/x86_64-linux-gnu:" + os.environ.get("MPI_LIB", "/opt/conda/lib")],
                        capture_output=True, text=True)
    if cc.returncode != 0 and ("asan" in cc.stderr or "ubsan" in cc.stderr or "sanitize" in cc.stderr):
        pytest.skip("g++ has no sanitizer runtimes here: " + cc.stderr.strip()[-200:])
    assert cc.returncode == 0, cc.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(exe), str(out)], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr
    _check_adds(out)


def test_cpp_compute_f16_host_port(tmp_path):
    """Compute<HiCCL::f16> on the host port (tests/cpp/f16_compute.cpp built
    with HICCL_PORT_HOST): add / start / wait on one hostile compute of n = 3
    gives NumPy's in-order half sum.  tests/test_f16_gpu.py runs the same
    program's GPU build on the same inputs."""
    make(ROOT, "build/f16_compute_host")
    x = H.hostile(3, COUNT, shift=3, seed=3)
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    x.tofile(inp)
    p = subprocess.run([os.path.join(ROOT, "build", "f16_compute_host"), str(inp), str(out), "3", str(COUNT)],
                       capture_output=True, text=True)
    assert p.returncode == 0 and "f16_compute: PASSED" in p.stdout, p.stdout + p.stderr
    got, exp = np.fromfile(out, np.uint16), H.native_sum(x)
    H.assert_nan_cap(exp)
    assert H.bits_equal(got, exp), H.first_mismatch(got, exp)
