"""CPU tier of the scaled sums (hiccl_reduce_scaled and its kin): the ABI and
its refusals, AUTO's answers, the NumPy restatement (tests/scale_expected.py)
against the stored fixtures and the pattern hashes, the f16 every-pattern check
that keeps two-step and one-step rounding apart, and the C++ layer on the host
(HiCCL::scale_finish, Compute<T>::set_scale on the host port).  No test here
needs a GPU or the reference; the fixtures pin the restatement to the
reference's own reduce_kernel, finished by the generator
(tests/golden/make_golden_scale.py).
"""
import ctypes
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import hiccl_amd
import scale_expected as E
from conftest import GOLDEN, ROOT, load_golden, make
from hiccl_amd import _lib as L

FLOAT_DTYPES = {"f32": L.HICCL_FLOAT32, "f64": L.HICCL_FLOAT64, "bf16": L.HICCL_BFLOAT16, "f16": L.HICCL_FLOAT16}
REFUSED_DTYPES = (L.HICCL_INT32, L.HICCL_UINT64, L.HICCL_BYTES)
NEW_SYMBOLS = ("hiccl_reduce_scaled", "hiccl_reduce_auto_choice_scaled", "hiccl_reduce_plan_set_scale",
               "hiccl_reduce_plan_scale", "hiccl_host_pipe_set_scale")
T, P = L.HICCL_ENGINE_TILE, L.HICCL_ENGINE_PHASE


def _tab(ptrs):
    return (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs)


def _scaled(dtype, alpha, cfg=None, n=1, out=0x1000):
    ins = _tab([0x2000 + 0x1000 * k for k in range(n)])
    return L.lib().hiccl_reduce_scaled(dtype, alpha, ctypes.c_void_p(out), ins, n, 4, None,
                                       ctypes.byref(cfg) if cfg is not None else None)


def _auto_scaled(dtype, cfg=None):
    out = [ctypes.c_int() for _ in range(5)]
    return L.lib().hiccl_reduce_auto_choice_scaled(dtype, ctypes.byref(cfg) if cfg is not None else None, 1024, 2.0, 256,
                                                   *[ctypes.byref(v) for v in out])


# ----------------------------------------------------------------------- ABI

def test_new_symbols_are_declared_bound_and_exported():
    declared = L.header_functions()
    for name in NEW_SYMBOLS:
        assert name in declared and name in L._SIGS and hasattr(L.lib(), name), name
    assert L.lib().hiccl_version() >= 500
    # the internal operator of a scaled sum is no hiccl_op_t value
    header = open(os.path.join(ROOT, "include", "hiccl_reduce.h")).read()
    values = sorted(int(v) for v in re.findall(r"\bHICCL_OP_[A-Z]+ = (\d+)", header))
    assert values == [0, 1, 2, 16, 17, 18, 19]
    ins = _tab([0x2000])
    for bad in (3, 7, 9, 15, 20, 99, 0x100, 256):
        rc = L.lib().hiccl_reduce_op(L.HICCL_FLOAT32, bad, ctypes.c_void_p(0x1000), ins, 1, 4, None, None)
        assert rc == 1 and "unknown op" in L.last_error(), bad


def test_refusals_return_invalid_value_with_a_message():
    """An integer or HICCL_BYTES dtype, a non-finite alpha, an alpha that is
    infinite as a float for the 4- and 2-byte types: refused by the one-shot
    call (and the dtype by auto_choice_scaled) before any device work -- the
    pointers here are not device memory -- each with its message."""
    for dt in REFUSED_DTYPES:
        for rc in (_scaled(dt, 0.5), _auto_scaled(dt)):
            assert rc == 1 and "floating types only" in L.last_error(), L.last_error()
    assert _scaled(42, 0.5) == 1 and "unknown dtype" in L.last_error()
    for dt in FLOAT_DTYPES.values():
        for bad in (float("inf"), float("-inf"), float("nan")):
            assert _scaled(dt, bad) == 1 and "alpha must be finite" in L.last_error(), (dt, bad)
        assert _auto_scaled(dt) == 0, L.last_error()
    for kind, dt in FLOAT_DTYPES.items():
        if kind != "f64":
            assert _scaled(dt, 1e300) == 1 and "finite as a float" in L.last_error(), kind
            assert _scaled(dt, -3.5e38) == 1 and "finite as a float" in L.last_error(), kind
    # the checks hiccl_reduce_ex makes still come for a valid alpha; count 0 is a no-op
    lib = L.lib()
    assert _scaled(L.HICCL_FLOAT32, 0.5, out=0) == 1 and "out is NULL" in L.last_error()
    assert lib.hiccl_reduce_scaled(L.HICCL_FLOAT64, 1e300, ctypes.c_void_p(0), _tab([]), 0, 0, None, None) == 0
    assert lib.hiccl_reduce_scaled(L.HICCL_FLOAT32, 0.0, ctypes.c_void_p(0), _tab([]), 0, 0, None, None) == 0
    assert lib.hiccl_reduce_scaled(L.HICCL_FLOAT32, 1e-60, ctypes.c_void_p(0), _tab([]), 0, 0, None, None) == 0
    bad_acc = L.ReduceConfig(acc=7)
    assert _scaled(L.HICCL_BFLOAT16, 0.5, bad_acc) == 1 and "bad acc mode" in L.last_error()
    a = ctypes.c_double(0.5)
    assert lib.hiccl_reduce_plan_set_scale(None, ctypes.byref(a)) == 1 and "plan is NULL" in L.last_error()
    assert lib.hiccl_reduce_plan_scale(None, ctypes.byref(a)) == -1
    assert lib.hiccl_host_pipe_set_scale(None, ctypes.byref(a)) == 1 and "pipe is NULL" in L.last_error()


def test_plan_set_scale_and_its_refusals_on_a_plan():
    """A plan takes, reports and clears a scale; refusals by dtype, alpha and
    operator.  Creating a plan binds a device, so without one this is skipped."""
    import torch
    lib = L.lib()
    if not torch.cuda.is_available() or torch.cuda.device_count() < 1:
        pytest.skip("no HIP device to bind a plan to")
    h = ctypes.c_void_p()
    assert lib.hiccl_reduce_plan_create(ctypes.byref(h), L.HICCL_BFLOAT16, 0) == 0, L.last_error()
    a, got = ctypes.c_double(1.0 / 3.0), ctypes.c_double(-1.0)
    try:
        assert lib.hiccl_reduce_plan_scale(h, ctypes.byref(got)) == 0 and got.value == -1.0
        assert lib.hiccl_reduce_plan_set_scale(h, ctypes.byref(a)) == 0
        assert lib.hiccl_reduce_plan_scale(h, ctypes.byref(got)) == 1 and got.value == 1.0 / 3.0
        assert lib.hiccl_reduce_plan_scale(h, None) == 1
        assert lib.hiccl_reduce_plan_set_acc(h, L.HICCL_ACC_WIDE) == 0  # the acc field is honoured
        assert lib.hiccl_reduce_plan_set_op(h, L.HICCL_OP_SUM) == 0
        assert lib.hiccl_reduce_plan_set_acc(h, L.HICCL_ACC_NATIVE) == 0
        for op in (L.HICCL_OP_MAX, L.HICCL_OP_PROD):
            assert lib.hiccl_reduce_plan_set_op(h, op) == 1 and "scaled plan" in L.last_error()
        assert lib.hiccl_reduce_plan_op(h) == L.HICCL_OP_SUM
        bad = ctypes.c_double(float("nan"))
        assert lib.hiccl_reduce_plan_set_scale(h, ctypes.byref(bad)) == 1 and "finite" in L.last_error()
        assert lib.hiccl_reduce_plan_scale(h, ctypes.byref(got)) == 1 and got.value == 1.0 / 3.0  # kept
        assert lib.hiccl_reduce_plan_set_scale(h, None) == 0 and lib.hiccl_reduce_plan_scale(h, None) == 0
        assert lib.hiccl_reduce_plan_set_op(h, L.HICCL_OP_MAX) == 0
        assert lib.hiccl_reduce_plan_set_scale(h, ctypes.byref(a)) == 1 and "HICCL_OP_SUM" in L.last_error()
        assert lib.hiccl_reduce_plan_set_scale(h, None) == 0  # clearing is always allowed
        # a config whose shape only the tuned sums have is refused by set_scale, and by set_config on a scaled plan
        assert lib.hiccl_reduce_plan_set_op(h, L.HICCL_OP_SUM) == 0
        for unroll in (1, 2, 8, 16):
            tuned, plain = L.ReduceConfig(engine=T, unroll=unroll), L.ReduceConfig(engine=T, unroll=4)
            assert lib.hiccl_reduce_plan_set_config(h, ctypes.byref(tuned)) == 0, L.last_error()
            assert lib.hiccl_reduce_plan_set_scale(h, ctypes.byref(a)) == 1
            assert "plan_set_scale" in L.last_error() and "shape the scaled kernels lack" in L.last_error()
            assert lib.hiccl_reduce_plan_scale(h, None) == 0
            assert lib.hiccl_reduce_plan_set_config(h, ctypes.byref(plain)) == 0
            assert lib.hiccl_reduce_plan_set_scale(h, ctypes.byref(a)) == 0
            assert lib.hiccl_reduce_plan_set_config(h, ctypes.byref(tuned)) == 1 and "plan_set_config" in L.last_error()
            assert lib.hiccl_reduce_plan_set_scale(h, None) == 0
    finally:
        lib.hiccl_reduce_plan_destroy(h)
    for dt in REFUSED_DTYPES:
        b = ctypes.c_void_p()
        assert lib.hiccl_reduce_plan_create(ctypes.byref(b), dt, 0) == 0
        try:
            assert lib.hiccl_reduce_plan_set_scale(b, ctypes.byref(a)) == 1 and "floating types only" in L.last_error()
            assert lib.hiccl_reduce_plan_scale(b, None) == 0
        finally:
            lib.hiccl_reduce_plan_destroy(b)


def _rows():
    import auto_table as A
    rows = [(dt, count, n, None) for (dt, count, n), _ in A.RULE_CASES]
    rows += [k for k, _ in A.all_engine_rows()] + [k for k, _ in A.all_store_rows()]
    return rows


def test_auto_choice_scaled_is_an_untuned_operators_answer():
    """The scaled kernels have no tuning table: on every row of
    tests/auto_table.py with a floating dtype, hiccl_reduce_auto_choice_scaled
    answers what hiccl_reduce_auto_choice_op answers for MAX, an untuned
    operator of the same dtype (under HICCL_ACC_WIDE, which MAX refuses: what
    SUM answers, WIDE being untuned already); a shape the scaled kernels lack is
    refused, never replaced."""
    seen, rows = set(), 0
    for dt, count, n, cfg in _rows():
        if dt not in FLOAT_DTYPES.values():
            continue
        wide = bool(cfg and cfg.get("acc")) and dt in (L.HICCL_BFLOAT16, L.HICCL_FLOAT16)
        other = dict(op=L.HICCL_OP_SUM) if wide else dict(op=L.HICCL_OP_MAX)
        if cfg and cfg.get("acc") and not wide:
            continue  # MAX refuses WIDE on any dtype, and f32 / f64 under SUM may be tuned
        try:
            want = hiccl_amd.auto_choice(dt, count, n, config=cfg, **other)
        except hiccl_amd.HicclError:
            with pytest.raises(hiccl_amd.HicclError):
                hiccl_amd.auto_choice(dt, count, n, config=cfg, scale=True)
            continue
        got = hiccl_amd.auto_choice(dt, count, n, config=cfg, scale=True)
        assert got == want, (dt, count, n, cfg, got, want)
        chunk = 8 if wide else 16
        assert (got["engine"], got["unroll"]) in ((T, 4), (P, chunk)) and got["store_policy"] in (2, 4)
        seen.add(got["engine"])
        rows += 1
    assert seen == {T, P} and rows > 20
    for cfg in (dict(engine=T, unroll=2), dict(engine=T, unroll=8), dict(engine=T, block=512, unroll=4),
                dict(engine=P, block=1024, unroll=4), dict(nontemporal=1), dict(store_policy=1)):
        with pytest.raises(hiccl_amd.HicclError, match="no kernel"):
            hiccl_amd.auto_choice(L.HICCL_FLOAT32, 1 << 20, 3, config=cfg, scale=True)
    got = hiccl_amd.auto_choice(L.HICCL_FLOAT32, 1 << 16, 100, scale=True)  # n > 64: the plan kernel's default shapes
    assert (got["engine"], got["unroll"]) in ((T, 4), (P, 16))
    # the wide-tile and half-tile rules stay the unscaled SUM's alone
    assert hiccl_amd.auto_choice(L.HICCL_FLOAT32, 1 << 28, 2)["unroll"] == 16
    assert hiccl_amd.auto_choice(L.HICCL_FLOAT32, 1 << 28, 2, scale=True)["engine"] == P
    assert hiccl_amd.auto_choice(L.HICCL_FLOAT32, 5 << 18, 2.4, scale=True)["unroll"] == 4


def test_python_layer_checks_the_scale_before_any_device_work():
    import torch
    check = hiccl_amd.compute._check_scale
    for dt in (torch.float32, torch.float64, torch.bfloat16, torch.float16):
        assert check(0.5, dt) == 0.5 and check(3, dt) == 3.0 and check(0.0, dt) == 0.0
    for dt in (torch.int32, torch.int64, torch.uint64, torch.uint8, L.HICCL_INT32, L.HICCL_BYTES):
        with pytest.raises(TypeError, match="floating"):
            check(0.5, dt)
    with pytest.raises(ValueError, match="only sums"):
        check(0.5, torch.float32, L.HICCL_OP_MAX)
    for bad in (float("inf"), float("nan")):
        with pytest.raises(ValueError, match="finite"):
            check(bad, torch.float32)
    for bad in ("1", None, True, np.bool_(True), 1j, torch.tensor([0.5, 0.5]), torch.tensor(True)):
        with pytest.raises(TypeError, match="real number"):
            check(bad, torch.float32)
    # any real scalar: numpy's, a 0-d tensor, a Fraction
    import fractions
    for ok in (np.float32(0.5), np.float64(0.5), np.int64(2), torch.tensor(0.5), fractions.Fraction(1, 2), 1 / np.float32(2)):
        assert check(ok, torch.float32) == float(ok)
    with pytest.raises(ValueError, match="finite"):
        check(np.float32("inf"), torch.float32)
    with pytest.raises(TypeError, match="floating"):
        hiccl_amd.reduce_ptrs(L.HICCL_INT32, 0x1000, [0x2000], 4, scale=0.5)
    with pytest.raises(ValueError, match="finite"):
        hiccl_amd.reduce_ptrs(L.HICCL_FLOAT32, 0x1000, [0x2000], 4, scale=float("inf"))
    with pytest.raises(TypeError, match="floating"):
        hiccl_amd.auto_choice(torch.int32, 1024, 2, scale=True)


# ----------------------------------------------- restatement against fixtures

def _manifest():
    with open(os.path.join(GOLDEN, "manifest_scale.json")) as fh:
        return json.load(fh)


def test_manifest_records_files_inputs_and_alphas():
    m = _manifest()
    assert len(m["files"]) >= 4
    for fname, info in m["files"].items():
        path = os.path.join(GOLDEN, fname)
        assert os.path.getsize(path) == info["bytes"] < (1 << 20)
        assert hashlib.sha256(open(path, "rb").read()).hexdigest() == info["sha256"]
    assert [[name, float(a).hex()] for name, a in E.ALPHAS] == m["alphas"]
    assert [a for _, a in E.ALPHAS] == [1.0, 0.5, 0.7, 0.1, 1 / 3, -1 / 1024, 3.0, 1 + 2.0 ** -24, 2.0 ** -20, 1e30, 0.0]
    for kind in E.KINDS:
        for n in E.NS:  # the inputs are not stored: the generators must still give what the fixtures were made from
            assert E.array_hash(E.hostile(kind, n)) == m["inputs"][f"{kind}/hostile_n{n}"], (kind, n)
    assert set(m["patterns"]) == {"f16", "f16_wide", "bf16", "bf16_wide"}


@pytest.mark.parametrize("kind", E.KINDS)
def test_restatement_gives_the_stored_outputs(kind):
    """scale_expected.scaled on the generated inputs = the stored outputs, for
    every n, alpha and accumulator; a finite nonzero alpha gives NaN exactly
    where the plain sum has one, alpha = 0 exactly where it is NaN or
    infinite; alpha = 1 gives the plain sum's words."""
    cases = load_golden(f"reduce_scale_{kind}")
    assert sorted(cases) == sorted(f"hostile_n{n}" for n in E.NS)
    modes = (False, True) if kind in E.HALVES else (False,)
    for n in E.NS:
        d, x = cases[f"hostile_n{n}"], E.hostile(kind, n)
        assert sorted(d) == sorted(f"{'w' if w else 'a'}{i}" for w in modes for i in range(len(E.ALPHAS)))
        for wide in modes:
            acc = E.acc_sum(kind, x, wide)
            f = acc if kind in ("f32", "f64") or wide else E.widen(kind, acc)
            for i, (name, alpha) in enumerate(E.ALPHAS):
                want = d[f"{'w' if wide else 'a'}{i}"]
                got = E.scaled(kind, x, alpha, wide)
                assert E.bits_equal(kind, got, want), f"{kind} n={n} {name} wide={wide}: {E.first_mismatch(kind, got, want)}"
                nan = E.is_nan(kind, want)
                assert np.array_equal(nan, ~np.isfinite(f) if alpha == 0.0 else np.isnan(f)), (kind, n, name)
            assert E.bits_equal(kind, d[f"{'w' if wide else 'a'}0"], E.plain_sum(kind, x, wide))
        assert 0 < E.is_nan(kind, d["a0"]).mean() <= 0.25, "the hostile inputs' NaN classes are there, a minority"


def test_alpha_one_is_the_existing_sum_fixtures_words():
    """reduce_f16's hostile cases hold the same inputs: their stored sums are
    the a0 outputs."""
    old, new = load_golden("reduce_f16"), load_golden("reduce_scale_f16")
    for n in E.NS:
        d = old[f"hostile_n{n}"]
        assert np.array_equal(d["in"], E.hostile("f16", n))
        assert E.bits_equal("f16", d["out"], new[f"hostile_n{n}"]["a0"])


@pytest.mark.parametrize("kind", E.HALVES)
def test_restatement_gives_the_stored_pattern_hashes(kind):
    m = _manifest()["patterns"]
    for wide in (False, True):
        words = E.patterns_expected(kind, wide)
        assert words.shape == (len(E.ALPHAS), 1 << 16)
        assert E.words_hash(kind, words) == m[f"{kind}{'_wide' if wide else ''}"]
    # alpha 1 gives the plain sum of one input: every pattern but -0, which 0 + x makes +0
    assert E.bits_equal(kind, words[0], E.plain_sum(kind, E.ALL_PATTERNS[None, :]))
    assert words[0][0x8000] == 0 and np.array_equal(np.delete(words[0], 0x8000)[:0x7C00], np.arange(0x7C00))


def test_f16_two_step_words_differ_from_one_step_words():
    """The definition is two roundings.  Over all 65,536 half patterns the
    two-step words differ from one rounding of the exact product on 1,946
    finite patterns at alpha 0.7 and on 206 at alpha 0.1, and from a half
    multiply by (half)alpha on many more: the fixture tells them apart."""
    x = E.ALL_PATTERNS
    finite = (x & 0x7C00) != 0x7C00
    words = E.patterns_expected("f16")
    for alpha, count in ((0.7, 1946), (0.1, 206)):
        i = [a for _, a in E.ALPHAS].index(alpha)
        two = E.finish("f16", x, alpha)
        # the n = 1 sum is the pattern itself, but for -0 (0 + -0 = +0)
        assert E.bits_equal("f16", np.delete(two, 0x8000), np.delete(words[i], 0x8000))
        one = E.one_step(x, alpha)
        assert int((two != one)[finite].sum()) == count, alpha
        assert int((two != E.half_multiply(x, alpha))[finite].sum()) > count
    # one worked example: 0x0423 * 0.7f
    s, a = np.float64(np.array([0x0423], np.uint16).view(np.float16)[0]), np.float64(np.float32(0.7))
    assert E.finish("f16", np.array([0x0423], np.uint16), 0.7)[0] == np.float32(s * a).astype(np.float16).view(np.uint16)


def test_restatement_on_the_plain_statements():
    f = lambda *v: np.array([[e] for e in v], np.float32)  # noqa: E731
    bits = lambda a: a.view(np.uint32)[0]  # noqa: E731
    assert bits(E.scaled("f32", np.zeros((0, 1), np.float32), -2.0, count=1)) == 0x80000000  # finish(+0, alpha)
    assert bits(E.scaled("f32", np.zeros((0, 1), np.float32), 0.0, count=1)) == 0
    assert np.isnan(E.scaled("f32", f(np.inf), 0.0)[0])  # Inf * 0
    assert bits(E.scaled("f32", f(-0.0), 3.0)) == 0  # the sum of -0 from +0 is +0
    tiny = np.array([[2]], np.uint32).view(np.float32)  # a subnormal times 0.5 stays one
    assert bits(E.scaled("f32", tiny, 0.5)) == 1
    # a32 of 1 + 2^-24 is 1.0f: f32 keeps the word, f64 multiplies by the double itself
    a = 1.0 + 2.0 ** -24
    assert bits(E.scaled("f32", f(3.0), a)) == bits(f(3.0)[0])
    assert E.scaled("f64", np.array([[3.0]]), a)[0] == 3.0 * a != 3.0
    assert E.scaled("f16", np.array([[0x7BFF]], np.uint16), 1e30)[0] == 0x7C00  # overflow in the narrowing
    assert E.scaled("bf16", np.array([[0x3F80]], np.uint16), 1e30)[0] == E.bf16_round(np.array([1e30], np.float32))[0]
    # wide: 1 + 2^-9 + 2^-9 summed in f32, scaled by 3, rounded once
    x = np.array([[0x3F80], [0x3B00], [0x3B00]], np.uint16)
    assert E.scaled("bf16", x, 3.0, wide=True)[0] == E.bf16_round(np.array([(1 + 2.0 ** -8) * 3], np.float32))[0]
    assert E.scaled("bf16", x, 3.0)[0] == 0x4040  # native: both small addends round away first


# ----------------------------------------------------------------------- C++

def test_cpp_scale_finish_plain_and_under_sanitizers(tmp_path):
    """tests/cpp/scale_finish.cpp, a stand-alone host program: scale_finish<T>
    on every bf16 / f16 pattern times every alpha against the exact product in
    double rounded twice, float and double on random words; it also counts
    where one rounding would differ (f16, alpha 0.7 and 0.1).  Built plainly
    and with -fsanitize=address,undefined; both binaries are run."""
    make(ROOT, "build/scale_finish")
    args = [float(a).hex() for _, a in E.ALPHAS]
    p = subprocess.run([os.path.join(ROOT, "build", "scale_finish")] + args, capture_output=True, text=True)
    assert p.returncode == 0 and "scale_finish: PASSED (11 alphas)" in p.stdout, p.stdout + p.stderr
    counts = dict(re.findall(r"f16 alpha (\S+) one-step differs on (\d+) finite patterns", p.stdout))
    assert {float.fromhex(k): int(v) for k, v in counts.items()} == {0.7: 1946, 0.1: 206}, p.stdout
    exe = tmp_path / "scale_finish_san"
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "scale_finish.cpp"),
                         "-o", str(exe)], capture_output=True, text=True)
    if cc.returncode != 0 and ("asan" in cc.stderr or "ubsan" in cc.stderr or "sanitize" in cc.stderr):
        pytest.skip("g++ has no sanitizer runtimes here: " + cc.stderr.strip()[-200:])
    assert cc.returncode == 0, cc.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(exe)] + args[:4], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "scale_finish: PASSED" in p.stdout, p.stdout + p.stderr
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr


def test_cpp_set_scale_static_asserts(tmp_path):
    """Compute<T>::set_scale takes float, double, bf16, f16 (and _Float16);
    an integer T and an operator wrapper fail to compile with a message."""
    inc = ["-I", os.path.join(ROOT, "include"), "-I", "/opt/conda/include"]
    body = ('#define HICCL_PORT_HOST\n#include "hiccl/compute.h"\nusing namespace HiCCL;\n'
            "void f() {{ Compute<{t}> c; c.set_scale(0.5); c.clear_scale(); }}\nint main() {{ return 0; }}\n")
    for t in ("float", "double", "bf16", "f16", "_Float16"):
        src = tmp_path / "ok.cpp"
        src.write_text(body.format(t=t))
        cc = subprocess.run(["g++", "-std=c++17", "-fsyntax-only"] + inc + [str(src)], capture_output=True, text=True)
        if t == "_Float16" and cc.returncode != 0 and "_Float16" in cc.stderr and "static assertion" not in cc.stderr:
            continue  # a compiler without _Float16
        assert cc.returncode == 0, t + cc.stderr
    for t, word in (("int32_t", "floating element types only"), ("uint64_t", "floating element types only"),
                    ("maxof<float>", "only sums are scaled"), ("prodof<bf16>", "only sums are scaled")):
        src = tmp_path / "bad.cpp"
        src.write_text(body.format(t=t))
        cc = subprocess.run(["g++", "-std=c++17", "-fsyntax-only"] + inc + [str(src)], capture_output=True, text=True)
        assert cc.returncode != 0 and "static assertion failed" in cc.stderr and word in cc.stderr, t + cc.stderr[-2000:]


ALPHA = 1.0 / 3.0
ALPHA_INDEX = 4


def check_scale_compute(exe, tmp_path, timeout=None, n=3):
    """Runs tests/cpp/scale_compute.cpp's program on the fixtures' hostile_n<n>
    inputs of f32 and bf16 with alpha = 1/3: scaled, scaled by 2/3 after a
    launch, and after clear_scale."""
    assert E.ALPHAS[ALPHA_INDEX][1] == ALPHA
    xf, xb = E.hostile("f32", n), E.hostile("bf16", n)
    paths = [tmp_path / name for name in ("in_f32.bin", "out_f32.bin", "in_bf16.bin", "out_bf16.bin")]
    np.ascontiguousarray(xf).tofile(paths[0])
    np.ascontiguousarray(xb).tofile(paths[2])
    cmd = [str(exe)] + [str(p) for p in paths] + [str(n), str(E.COUNT), float(ALPHA).hex()]
    if timeout:
        cmd = ["timeout", "-k", "5", str(timeout)] + cmd
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0 and "scale_compute: PASSED" in p.stdout, p.stdout + p.stderr
    for kind, x, path in (("f32", xf, paths[1]), ("bf16", xb, paths[3])):
        stored = load_golden(f"reduce_scale_{kind}")[f"hostile_n{n}"][f"a{ALPHA_INDEX}"]
        for suffix, want in (("", stored), (".twice", E.scaled(kind, x, 2.0 * ALPHA)), (".plain", E.plain_sum(kind, x))):
            got = np.fromfile(str(path) + suffix, E.carrier(kind))
            assert E.bits_equal(kind, got, want), f"Compute<{kind}>{suffix}: " + E.first_mismatch(kind, got, want)


def test_cpp_compute_set_scale_host_port(tmp_path):
    """Compute<float> and Compute<HiCCL::bf16> with set_scale / clear_scale on
    the host port (tests/cpp/scale_compute.cpp built with HICCL_PORT_HOST),
    misaligned inputs and output, against the fixtures: the same bits as the
    GPU gives.  tests/test_scale_gpu.py runs the same program's GPU build."""
    make(ROOT, "build/scale_compute_host")
    check_scale_compute(os.path.join(ROOT, "build", "scale_compute_host"), tmp_path)
