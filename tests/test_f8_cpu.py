"""CPU tier of the OCP FP8 element types (HICCL_FLOAT8_E4M3 = 16,
HICCL_FLOAT8_E5M2 = 17): the ABI values, the refusals that precede any device
work, AUTO's answers, the bucket layout, and the C++ layer on the host
(HiCCL::f8e4m3 / f8e5m2 and Compute<T> on the host port) against torch's own
conversions (tests/f8_expected.py).  No test here needs a GPU.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import f8_expected as E
import hiccl_amd
from conftest import ROOT, make
from hiccl_amd import _lib as L

F8 = (L.HICCL_FLOAT8_E4M3, L.HICCL_FLOAT8_E5M2)
TILE, PHASE = L.HICCL_ENGINE_TILE, L.HICCL_ENGINE_PHASE


def _tab(ptrs):
    return (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs)


def _cfg(**kw):
    return ctypes.byref(L.ReduceConfig(**kw))


# ------------------------------------------------------------------- the ABI

def test_abi_values_sizes_and_version():
    lib = L.lib()
    assert F8 == (16, 17) and tuple(E.CODE.values()) == F8
    assert [lib.hiccl_dtype_size(d) for d in F8] == [1, 1]
    assert [lib.hiccl_dtype_size(d) for d in range(7, 16)] == [0] * 9  # the values are sparse
    assert lib.hiccl_dtype_size(18) == 0
    assert lib.hiccl_version() >= 600  # 0.5.0 had no FP8
    header = open(L.HEADER_PATH).read()
    assert "HICCL_FLOAT8_E4M3 = 16" in header and "HICCL_FLOAT8_E5M2 = 17" in header
    assert "HICCL_NUM_DTYPES = 7" in header and "dense block" in header
    assert L.DTYPE_OF_TORCH[torch.float8_e4m3fn] == 16 and L.DTYPE_OF_TORCH[torch.float8_e5m2] == 17
    assert hiccl_amd.HICCL_FLOAT8_E4M3 == 16 and hiccl_amd.HICCL_FLOAT8_E5M2 == 17


# -------------------------------------------------------------- the refusals

@pytest.mark.parametrize("dt", F8)
def test_refusals_precede_device_work(dt):
    """Each returns hipErrorInvalidValue (1) with a message; the pointers are
    no device memory, so none of these calls may reach the device."""
    lib = L.lib()
    out, a, b = 0x10000, 0x20000, 0x30000
    for op, word in ((L.HICCL_OP_PROD, "HICCL_OP_PROD"), (L.HICCL_OP_BAND, "integer types only"),
                     (L.HICCL_OP_BOR, "integer types only"), (L.HICCL_OP_BXOR, "integer types only")):
        assert lib.hiccl_reduce_op(dt, op, out, _tab([a, b]), 2, 64, None, None) == 1
        assert word in L.last_error(), L.last_error()
        assert lib.hiccl_reduce_auto_choice_op(dt, op, None, 1 << 20, 2.0, 256, None, None, None, None, None) == 1
        assert word in L.last_error(), L.last_error()
    for op in (L.HICCL_OP_MAX, L.HICCL_OP_MIN):
        assert lib.hiccl_reduce_op(dt, op, out, _tab([a, b]), 2, 64, None, _cfg(acc=L.HICCL_ACC_WIDE)) == 1
        assert "HICCL_ACC_WIDE" in L.last_error(), L.last_error()
    for alpha in (float("inf"), float("nan"), 1e300):
        assert lib.hiccl_reduce_scaled(dt, alpha, out, _tab([a, b]), 2, 64, None, None) == 1
        assert "finite" in L.last_error(), L.last_error()
    # a byte-overlapping pair: one byte is an element, so any offset but 0 overlaps partially
    for shift in (1, 15, 63):
        assert lib.hiccl_reduce(dt, out, _tab([a, out + shift]), 2, 64, None) == 1
        assert "partially overlaps" in L.last_error(), L.last_error()
        assert lib.hiccl_reduce_scaled(dt, 0.5, out, _tab([out - shift]), 1, 64, None, None) == 1
        assert "partially overlaps" in L.last_error(), L.last_error()
    # a shape the FP8 kernels lack is refused, never replaced
    for cfg in (dict(engine=TILE, unroll=2), dict(engine=TILE, unroll=8), dict(engine=PHASE, block=1024, unroll=4),
                dict(engine=TILE, nontemporal=1)):
        assert lib.hiccl_reduce_auto_choice_ex(dt, _cfg(**cfg), 1 << 20, 2.0, 256, None, None, None, None, None) == 1, cfg
        assert "no kernel" in L.last_error(), L.last_error()


def test_python_refusals():
    for dtype in (torch.float8_e4m3fn, torch.float8_e5m2):
        from hiccl_amd.compute import _check_op, _check_scale
        with pytest.raises(TypeError, match="PROD"):
            _check_op(L.HICCL_OP_PROD, dtype)
        for op in (L.HICCL_OP_BAND, L.HICCL_OP_BOR, L.HICCL_OP_BXOR):
            with pytest.raises(TypeError, match="integer types only"):
                _check_op(op, dtype)
        for op in (L.HICCL_OP_SUM, L.HICCL_OP_MAX, L.HICCL_OP_MIN):
            _check_op(op, dtype)
        assert _check_scale(0.25, dtype) == 0.25 and _check_scale(0.25, L.DTYPE_OF_TORCH[dtype]) == 0.25
        with pytest.raises(ValueError, match="finite"):
            _check_scale(float("inf"), dtype)
        with pytest.raises(ValueError, match="only sums"):
            _check_scale(0.5, dtype, L.HICCL_OP_MAX)


# ------------------------------------------------------------- host answers

SIZES = [1 << s for s in range(8, 31, 2)] + [3 * (1 << 22) + 40, 5 * (1 << 25)]  # bytes per input


@pytest.mark.parametrize("dt", F8)
def test_auto_choice_is_f64s_and_names_default_shapes_only(dt):
    """AUTO treats the FP8 types as it treats f64, the other untuned 16-packet
    type: the same answer for the same bytes, under SUM, MAX and the scaled
    sums; never a tuned row (TILE unroll 1, 2, 8, 16)."""
    for nbytes in SIZES:
        for n in (1, 2, 3, 4, 5, 8, 17, 64, 65):
            for kw in (dict(), dict(op=L.HICCL_OP_MAX), dict(scale=True)):
                got = hiccl_amd.auto_choice(dt, nbytes, n, **kw)
                assert got == hiccl_amd.auto_choice(L.HICCL_FLOAT64, nbytes // 8, n, **kw), (nbytes, n, kw)
                assert (got["engine"], got["unroll"]) in ((TILE, 4), (PHASE, 16)), (nbytes, n, kw, got)
            wide = hiccl_amd.auto_choice(dt, nbytes, n, config=dict(acc=L.HICCL_ACC_WIDE))
            assert (wide["engine"], wide["unroll"]) in ((TILE, 4), (PHASE, 8)), (nbytes, n, wide)
            scaled_wide = hiccl_amd.auto_choice(dt, nbytes, n, config=dict(acc=L.HICCL_ACC_WIDE), scale=True)
            assert scaled_wide == wide, (nbytes, n)
    with pytest.raises(hiccl_amd.HicclError, match="no kernel"):
        hiccl_amd.auto_choice(dt, 1 << 24, 8, config=dict(engine=TILE, unroll=2))
    with pytest.raises(hiccl_amd.HicclError, match="no kernel"):
        hiccl_amd.auto_choice(dt, 1 << 24, 8, config=dict(engine=PHASE, unroll=8))  # native chunks are 16 packets


def test_bucket_stride():
    lib = L.lib()
    g = 64 << 10
    for dt in F8:
        assert lib.hiccl_bucket_stride(dt, 0) == 0
        for count in (1, g - 1, g, g + 1, (1 << 30) + 5):
            assert lib.hiccl_bucket_stride(dt, count) == -(-count // g) * g + g
            assert lib.hiccl_bucket_stride(dt, count) == lib.hiccl_bucket_stride(L.HICCL_BYTES, count)
    assert lib.hiccl_bucket_stride(7, 100) == 0


# --------------------------------------------------- the restatement itself

@pytest.mark.parametrize("fmt", E.FORMATS)
def test_restatement_says_what_the_definition_says(fmt):
    """A few words of the definition, on torch alone."""
    top = 0x7E if fmt == "e4m3" else 0x7B  # the largest finite value
    u8 = lambda *b: torch.tensor(b, dtype=torch.uint8)  # noqa: E731
    assert float(E.widen(u8(top), fmt)) == E.MAX[fmt]
    assert E.fold_sum([u8(0x80), u8(0x80)], fmt).tolist() == [0x00]           # -0 + -0 from +0
    assert E.fold_sum([u8(top), u8(top)], fmt).tolist() == [top]              # saturates
    assert E.fold_sum([], fmt, count=3).tolist() == [0, 0, 0]
    assert E.fold_mm([], fmt, True, count=1).tolist() == [E.MAX_ID[fmt]]
    assert E.fold_mm([], fmt, False, count=1).tolist() == [E.MIN_ID[fmt]]
    assert E.fold_mm([u8(0x80), u8(0x00)], fmt, True).tolist() == [0x00]      # -0 < +0
    assert E.fold_mm([u8(0x00), u8(0x80)], fmt, False).tolist() == [0x80]
    assert bool(E.is_nan(E.fold_mm([u8(0x7F), u8(0x01)], fmt, True), fmt)[0])
    inf = torch.tensor([float("inf"), float("-inf"), float("nan"), 1e30, -1e30, 5.3e-23], dtype=torch.float32)
    r = E.round_f(inf, fmt)
    assert r[3:].tolist() == [top, 0x80 | top, 0x00]
    assert bool(E.is_nan(r, fmt)[2])
    if fmt == "e5m2":
        assert r[:2].tolist() == [0x7C, 0xFC]
        assert bool(E.is_nan(E.fold_sum([u8(0x7C), u8(0xFC)], fmt), fmt)[0])  # Inf + -Inf
    else:
        assert E.is_nan(r, fmt)[:2].all()
    # the wide sum rounds once: 1 + 32 x 2^-6 is 1.5 wide and 1 native (1 + 2^-6 rounds back to 1 every time)
    one, small = int(E.round_f(torch.tensor([1.0]), fmt)), int(E.round_f(torch.tensor([2.0 ** -6]), fmt))
    ins = [u8(one)] + [u8(small)] * 32
    assert float(E.widen(E.fold_sum(ins, fmt, wide=True), fmt)) == 1.5
    assert float(E.widen(E.fold_sum(ins, fmt), fmt)) == 1.0


# ---------------------------------------------------------------- C++ layer

def _check_tables(outdir):
    a, b = E.pair_table()
    i = torch.arange(1 << 20, dtype=torch.int32)
    words = torch.cat([i << 12, (i << 12) | 1]).view(torch.float32)
    for fmt in E.FORMATS:
        load = lambda name, dt=np.uint8: torch.from_numpy(np.fromfile(os.path.join(outdir, f"{name}_{fmt}.bin"), dt))  # noqa: E731
        E.assert_equal(load("add"), E.round_f(E.widen(a, fmt) + E.widen(b, fmt), fmt), fmt, f"{fmt} +=")
        E.assert_equal(load("round"), E.round_f(words, fmt), fmt, f"{fmt} round")
        got, exp = load("widen", np.float32), E.widen(E.ALL_BYTES, fmt)
        nan = torch.isnan(exp)
        assert torch.equal(torch.isnan(got), nan), f"{fmt} operator float: NaNs"
        assert torch.equal(got[~nan].view(torch.int32), exp[~nan].view(torch.int32)), f"{fmt} operator float"
        assert load("ident").tolist() == [E.MAX_ID[fmt], E.MIN_ID[fmt], 0x00, 0x00, 0x80], f"{fmt} identities"


def test_f8_types_against_torch(tmp_path):
    """tests/cpp/f8_add.cpp, a stand-alone host program: `+=` on all 65,536
    operand pairs, round on 2,097,152 f32 patterns (every i << 12 and every
    (i << 12) | 1), operator float on all 256 bytes and the maxof / minof
    identities, compared here with torch's conversions.  Built plainly and with
    -fsanitize=address,undefined; both binaries are run."""
    make(ROOT, "build/f8_add")
    plain = tmp_path / "plain"
    plain.mkdir()
    p = subprocess.run([os.path.join(ROOT, "build", "f8_add"), str(plain)], capture_output=True, text=True)
    assert p.returncode == 0 and "f8_add: WROTE" in p.stdout, p.stdout + p.stderr
    _check_tables(str(plain))
    exe = tmp_path / "f8_add_san"
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "f8_add.cpp"),
                         "-o", str(exe)], capture_output=True, text=True)
    if cc.returncode != 0 and ("asan" in cc.stderr or "ubsan" in cc.stderr or "sanitize" in cc.stderr):
        pytest.skip("g++ has no sanitizer runtimes here: " + cc.stderr.strip()[-200:])
    assert cc.returncode == 0, cc.stderr
    san = tmp_path / "san"
    san.mkdir()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(exe), str(san)], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "f8_add: WROTE" in p.stdout, p.stdout + p.stderr
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr
    _check_tables(str(san))


def test_cpp_surface_compiles_and_refuses(tmp_path):
    """dtype_of, set_scale and maxof / minof take the FP8 types; prodof and the
    bitwise wrappers fail to compile with a message."""
    inc = ["-I", os.path.join(ROOT, "include"), "-I", "/opt/conda/include", "-DHICCL_PORT_HOST"]
    ok = tmp_path / "ok.cpp"
    ok.write_text('#include "hiccl/compute.h"\nusing namespace HiCCL;\n'
                  "static_assert(dtype_of<f8e4m3>() == 16 && dtype_of<f8e5m2>() == 17, \"\");\n"
                  "static_assert(dtype_of<maxof<f8e4m3>>() == 16 && op_of<minof<f8e5m2>>() == 2, \"\");\n"
                  "void f() { Compute<f8e4m3> a; a.set_scale(0.5); a.clear_scale(); Compute<f8e5m2> b; b.set_scale(2);\n"
                  "           Compute<maxof<f8e5m2>> c; (void)c; }\nint main() { return 0; }\n")
    cc = subprocess.run(["g++", "-std=c++17", "-fsyntax-only"] + inc + [str(ok)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    for t in ("prodof<f8e4m3>", "prodof<f8e5m2>", "bandof<f8e4m3>", "bxorof<f8e5m2>"):
        bad = tmp_path / "bad.cpp"
        bad.write_text(f'#include "hiccl/compute.h"\nusing namespace HiCCL;\n{t} x;\nint main() {{ return 0; }}\n')
        cc = subprocess.run(["g++", "-std=c++17", "-fsyntax-only"] + inc + [str(bad)], capture_output=True, text=True)
        assert cc.returncode != 0 and "static assertion failed" in cc.stderr and "FP8 types" in cc.stderr, t + cc.stderr[-2000:]


def test_compute_cpp_on_the_host_port(tmp_path):
    """Compute<f8e4m3> and Compute<f8e5m2> on the host port
    (tests/cpp/f8_compute.cpp built with HICCL_PORT_HOST), misaligned inputs
    and output, plain and with set_scale: the bits the GPU gives
    (tests/test_f8_gpu.py runs the same program's GPU build)."""
    make(ROOT, "build/f8_compute_host")
    n, count, alpha = 5, 4099, 1.0 / 3.0
    paths, data = {}, {}
    for fmt in E.FORMATS:
        data[fmt] = E.hostile_bytes(fmt, 2, count, seed=51) + E.tame_bytes(fmt, n - 2, count, seed=52)
        paths[fmt] = (tmp_path / f"in_{fmt}.bin", tmp_path / f"out_{fmt}.bin")
        torch.stack(data[fmt]).numpy().tofile(paths[fmt][0])
    cmd = [os.path.join(ROOT, "build", "f8_compute_host")]
    for fmt in E.FORMATS:
        cmd += [str(p) for p in paths[fmt]]
    p = subprocess.run(cmd + [str(n), str(count), float(alpha).hex()], capture_output=True, text=True)
    assert p.returncode == 0 and "f8_compute: PASSED" in p.stdout, p.stdout + p.stderr
    for fmt in E.FORMATS:
        for suffix, a in (("", alpha), (".plain", None)):
            got = torch.from_numpy(np.fromfile(str(paths[fmt][1]) + suffix, np.uint8))
            E.assert_equal(got, E.expected(data[fmt], fmt, alpha=a), fmt, f"Compute<{fmt}>{suffix}")
