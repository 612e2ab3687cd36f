"""CPU tier: the generated code of the scaled-sum kernels (reduce_scale.hip).

The library holds four gfx950 code objects, one per kernel translation unit.
As tests/test_ops_isa.py does for MAX / MIN, this test takes the fat binary
apart, finds the code object that holds the scaled kernels and points the
helpers of test_kernel_isa / test_f16_isa at it.  For the default one-shot and
plan kernels (k_reduce_single_scaled, k_reduce_plan_scaled; both engines, nt
and write-through stores) of the six ops it checks that each

  * passes the descriptor checks the SUM kernels pass (buffer loads, scalar
    descriptors, no waterfall loop around a buffer op) and has no private
    segment;
  * falls into no lower occupancy step than the SUM kernel of the same shape
    (waves per SIMD from the VGPR allocation: 512 registers per lane in steps
    of 8, at most 8 waves);
  * f32 and f64: contains a multiply (v_pk_mul_f32 / v_mul_f32, v_mul_f64)
    and no fused multiply-add on floats -- the multiply follows the last add
    and must not fuse with it;
  * native f16: contains no v_fma_mix* and no v_pk_mul_f16 (the finishing step
    is widen, f32 multiply, narrow: two roundings), but the f32 multiply and
    both conversions;
  * bf16: contains an f32 multiply and v_cvt_pk_bf16_f32.

It skips when the library is not built or the LLVM tools are not installed.
"""
import pytest

import test_f16_isa as f16isa
import test_kernel_isa as isa
import test_ops_isa as opsisa
from test_prod_isa import fused_float

NS = isa.NS

# name -> (the scaled op's demangled name, the SUM op of the same accumulator, PHASE packets per lane, what it is)
OPS = {
    "f32": ("OpFloatScaled<(anonymous namespace)::OpF32, float>", "OpF32", 16, "fmul32"),
    "f64": ("OpFloatScaled<(anonymous namespace)::OpF64, double>", "OpF64", 16, "fmul64"),
    "bf16": ("OpBF16Scaled<(anonymous namespace)::OpBF16>", "OpBF16", 16, "bf16"),
    "bf16-wide": ("OpBF16Scaled<(anonymous namespace)::OpBF16Wide>", "OpBF16Wide", 8, "bf16"),
    "f16": ("OpF16Scaled<(anonymous namespace)::OpF16>", "OpF16", 16, "f16"),
    "f16-wide": ("OpF16Scaled<(anonymous namespace)::OpF16Wide>", "OpF16Wide", 8, "f16-wide"),
}

CASES = [pytest.param(name, i, id=f"{name}-{i}") for name in OPS for i in range(8)]


def kernels_of(op, p, scaled):
    """Demangled-name fragments of an op's default one-shot and plan kernels."""
    tail = "_scaled" if scaled else ""
    return ([f"k_reduce_single{tail}<{NS}{op}, {s}>" for s in opsisa.shapes(p)] +
            [f"k_reduce_plan{tail}<{NS}{op}, {s}>" for s in opsisa.shapes(p)])


def waves_per_simd(vgprs):
    """Occupancy from the VGPR allocation alone: a SIMD has 512 registers per
    lane, allocated in steps of 8, and runs at most 8 waves."""
    alloc = -(-max(vgprs, 1) // 8) * 8
    return min(8, 512 // alloc)


@pytest.fixture(scope="module")
def scale_code_object():
    """Points the helpers at the scaled-sum code object for this module;
    yields the VGPR counts of the SUM kernels (first code object)."""
    f16isa.code_object_or_skip()
    sum_vgprs = {}
    for _, sum_op, p, _ in OPS.values():
        for k in kernels_of(sum_op, p, False):
            sum_vgprs[k] = f16isa.metadata_of(k)["vgpr_count"]
    original = isa.code_object
    found = None
    try:
        objects = opsisa.code_objects()
        for co in objects:
            isa.code_object = lambda co=co: (co, "")
            opsisa.clear_caches()
            if any("k_reduce_single_scaled" in name for name in isa.kernel_symbols()):
                found = co
                break
        assert found, "no code object of the library holds the scaled-sum kernels"
        assert found == objects[-1] and len(objects) == 4, "the scaled unit is the fourth, linked last"
        yield sum_vgprs
    finally:
        isa.code_object = original
        opsisa.clear_caches()


@pytest.mark.parametrize("name,i", CASES)
def test_scaled_kernels(scale_code_object, name, i):
    op, sum_op, p, what = OPS[name]
    kernel = kernels_of(op, p, True)[i]
    ins = isa.instructions(kernel)
    ops = [o for _, o, _ in ins]
    # the descriptor checks of test_kernel_isa.test_descriptors_stay_scalar
    assert any(o.startswith("buffer_load_dwordx4") for o in ops), f"{kernel}: no buffer loads found"
    rfl = sum(o.startswith("v_readfirstlane") for o in ops)
    assert rfl <= isa.MAX_READFIRSTLANE, f"{kernel}: {rfl} v_readfirstlane"
    bad = isa.waterfalls(ins)
    assert not bad, f"{kernel}: {len(bad)} buffer ops inside a waterfall loop, first at {bad[0]:#x}"
    meta = f16isa.metadata_of(kernel)
    sum_kernel = kernels_of(sum_op, p, False)[i]
    sum_v = scale_code_object[sum_kernel]
    print(f"{kernel}: {meta['vgpr_count']} VGPRs ({sum_op}: {sum_v}), {len(ops)} instructions")
    assert meta["private_segment_fixed_size"] == 0, f"{kernel}: scratch {meta['private_segment_fixed_size']} B"
    assert waves_per_simd(meta["vgpr_count"]) >= waves_per_simd(sum_v), \
        f"{kernel}: {meta['vgpr_count']} VGPRs is a lower occupancy step than {sum_kernel}'s {sum_v}"
    f32mul = any(o.startswith(("v_mul_f32", "v_pk_mul_f32")) for o in ops)
    if what in ("fmul32", "fmul64"):
        assert f32mul if what == "fmul32" else any(o.startswith("v_mul_f64") for o in ops), f"{kernel}: no multiply"
        fused = sorted({o for o in ops if fused_float(o)})
        assert not fused, f"{kernel}: fused multiply-adds {fused}"
    elif what == "bf16":
        assert f32mul, f"{kernel}: no f32 multiply"
        assert "v_cvt_pk_bf16_f32" in ops, f"{kernel}: no v_cvt_pk_bf16_f32"
        fused = sorted({o for o in ops if fused_float(o)})
        assert not fused, f"{kernel}: fused multiply-adds {fused}"
    else:
        mix = sorted({o for o in ops if o.startswith(("v_fma_mix", "v_mad_mix"))})
        assert not mix, f"{kernel}: {mix}: the finishing multiply merged with a conversion"
        assert f32mul, f"{kernel}: no f32 multiply"
        assert any(o.startswith(("v_cvt_f16_f32", "v_cvt_pk_f16_f32", "v_cvt_pkrtz")) for o in ops), f"{kernel}: no narrowing"
        assert not any(o.startswith("v_cvt_pkrtz") for o in ops), f"{kernel}: a round-toward-zero narrowing"
        if what == "f16":
            assert "v_pk_mul_f16" not in ops, f"{kernel}: a half multiply in the finishing step"
            assert "v_pk_add_f16" in ops, f"{kernel}: the sum is not the native half add"
            assert any(o.startswith("v_cvt_f32_f16") for o in ops), f"{kernel}: no widening"
