"""CPU tier: the generated code of the OCP FP8 kernels (reduce_f8.hip, compiled
into the library's last code object, next to the scaled sums').

As tests/test_scale_isa.py does, this test takes the fat binary apart, finds
the code object that holds the FP8 kernels and points the helpers of
test_kernel_isa / test_f16_isa at it.  For both formats it checks the default
one-shot and plan kernels (both engines, nt and write-through stores) of the
native sum, the f32-accumulating sum, MAX and both scaled sums, and the program
kernel of the native sum and of MAX.  Each must

  * pass the descriptor checks the SUM kernels pass (buffer loads, the
    v_readfirstlane bound, no waterfall loop around a buffer op);
  * contain the packed widen of its format (v_cvt_pk_f32_fp8 / v_cvt_pk_f32_bf8)
    and the packed round (v_cvt_pk_fp8_f32 / v_cvt_pk_bf8_f32), and none of the
    other format's;
  * have no private segment (private_segment_fixed_size == 0).

The VGPR counts are printed (DESIGN.md records them), not asserted.  It skips
when the library is not built or the LLVM tools are not installed.
"""
import pytest

import test_f16_isa as f16isa
import test_kernel_isa as isa
import test_ops_isa as opsisa

NS = isa.NS
FMT = {"e4m3": (0, "fp8"), "e5m2": (1, "bf8")}  # format -> (the ops' template argument, the ISA's name)


def ops_of(f):
    """name -> (demangled op, scaled kernel?, PHASE packets per lane, has a program kernel?)"""
    return {
        "sum": (f"OpF8<{f}>", False, 16, True),
        "wide": (f"OpF8Wide<{f}>", False, 8, False),
        "max": (f"OpF8MM<true, {f}>", False, 16, True),
        "scaled": (f"OpF8Scaled<{NS}OpF8<{f}>, {f}>", True, 16, False),
        "scaled-wide": (f"OpF8Scaled<{NS}OpF8Wide<{f}>, {f}>", True, 8, False),
    }


def kernels_of(op, scaled, p, prog):
    tail = "_scaled" if scaled else ""
    names = ([f"k_reduce_single{tail}<{NS}{op}, {s}>" for s in opsisa.shapes(p)] +
             [f"k_reduce_plan{tail}<{NS}{op}, {s}>" for s in opsisa.shapes(p)])
    return names + ([f"k_program<{NS}{op}, 4>"] if prog else [])


CASES = [pytest.param(fmt, name, i, id=f"{fmt}-{name}-{i}")
         for fmt, (f, _) in FMT.items() for name, (_, _, _, prog) in ops_of(f).items() for i in range(8 + prog)]


@pytest.fixture(scope="module")
def f8_code_object():
    f16isa.code_object_or_skip()
    original = isa.code_object
    found = None
    try:
        for co in opsisa.code_objects():
            isa.code_object = lambda co=co: (co, "")
            opsisa.clear_caches()
            if any("OpF8<" in name for name in isa.kernel_symbols()):
                found = co
                break
        assert found, "no code object of the library holds the FP8 kernels"
        yield found
    finally:
        isa.code_object = original
        opsisa.clear_caches()


@pytest.mark.parametrize("fmt,name,i", CASES)
def test_f8_kernels(f8_code_object, fmt, name, i):
    f, word = FMT[fmt]
    other = "bf8" if word == "fp8" else "fp8"
    kernel = kernels_of(*ops_of(f)[name])[i]
    ins = isa.instructions(kernel)
    ops = [o for _, o, _ in ins]
    # the descriptor checks of test_kernel_isa.test_descriptors_stay_scalar
    assert any(o.startswith("buffer_load_dwordx4") for o in ops), f"{kernel}: no buffer loads found"
    rfl = sum(o.startswith("v_readfirstlane") for o in ops)
    assert rfl <= isa.MAX_READFIRSTLANE, f"{kernel}: {rfl} v_readfirstlane"
    bad = isa.waterfalls(ins)
    assert not bad, f"{kernel}: {len(bad)} buffer ops inside a waterfall loop, first at {bad[0]:#x}"
    meta = f16isa.metadata_of(kernel)
    print(f"{kernel}: {meta['vgpr_count']} VGPRs, {len(ops)} instructions")
    assert meta["private_segment_fixed_size"] == 0, f"{kernel}: scratch {meta['private_segment_fixed_size']} B"
    assert any(o.startswith(f"v_cvt_pk_f32_{word}") for o in ops), f"{kernel}: no packed widen v_cvt_pk_f32_{word}"
    assert any(o.startswith(f"v_cvt_pk_{word}_f32") for o in ops), f"{kernel}: no packed round v_cvt_pk_{word}_f32"
    wrong = sorted({o for o in ops if o.startswith((f"v_cvt_pk_f32_{other}", f"v_cvt_pk_{other}_f32"))})
    assert not wrong, f"{kernel}: the other format's conversions {wrong}"
